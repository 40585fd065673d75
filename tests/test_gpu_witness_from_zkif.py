"""Witness ingest on the device (otti_witness_from_zkif, k_wit_ingest.hip) against the host pair, zkif_load on the three files followed by the
upload: the same resident witness — z, inputs, small_fraction, proof bytes — for the product writer's files and for shapes it never writes; the host
pair's error code for every single-defect and two-defect file and for the first 200 mutants the sanitizer run (tests/test_zkif_wit_walk_host.py)
has already read on the CPU; the kept rows and products of a device-ingested witness under its mutators; the AUTO rule; and a served request.
Nothing here is expected to fault: every file is read through the bounds-checked reader the CPU run has exercised on the same bytes."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import otti_amd as oa
import orc
import zkif_ingest_cases as zc
import zkif_witness_cases as wc
from otti_amd.serve import SPZK, SpzkServer
from witness_cases import Q, bytes32, case, values, z_of

pytestmark = pytest.mark.gpu
SEED = b"\x2a" * 32
LABEL = b"nizk_example"
ACCEPTED = wc.accepted_cases()


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(scope="module")
def work():
    d = tempfile.mkdtemp(prefix="zkif-witness-")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _host_pair(inst, paths):
    """the reference: zkif_load on the three files, then the upload.  (witness, assignment)"""
    a = oa.zkif_load(*paths)
    return oa.Witness(inst, oa.VarsAssignment.new(a["vars"]), oa.InputsAssignment.new(a["inputs"])), a


def _host_pair_code(inst, paths):
    try:
        _host_pair(inst, paths)
    except oa.api.SpartanError as e:
        return e.code
    return 0


def _code(inst, paths, mode):
    """(error code or 0, (witness handle value, inputs pointer set) afterwards) through the C call: both outputs must stay what they were on an error"""
    h, rp = ctypes.c_void_p(0x1234), ctypes.POINTER(oa.api._R1CS)()
    rc = oa.lib.otti_witness_from_zkif(inst._h, os.fsencode(paths[1]), os.fsencode(paths[2]), oa.api.INGEST_MODES[mode], ctypes.byref(h), ctypes.byref(rp))
    if rc == 0:
        oa.lib.otti_r1cs_free(rp); oa.lib.otti_witness_free(h)
        return 0, None
    return rc, (h.value, bool(rp))


def _assert_same_witness(inst, got, got_inputs, want, a):
    zg, sg = z_of(got)
    zw, sw = z_of(want)
    assert _same(zg, zw), "z differs from the upload's"
    assert got.info[1:] == want.info[1:] and sg == sw, (got.info, want.info)
    assert _same(got_inputs, a["inputs"])
    assert got.diff(inst, a["vars"], max_indices=4)[0] == 0              # the host loader's vector changes nothing of the device-ingested witness


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name,case", ACCEPTED, ids=[n for n, _ in ACCEPTED])
def test_shapes_the_products_writer_does_not_produce(work, name, case):
    paths = wc.write_case(work, name, case)
    inst, _ = oa.Instance.from_zkif(*paths, mode="host")                    # (with the witness file: the loader wants every declared id accounted for in bytes)
    want, a = _host_pair(inst, paths)
    assert _same(a["vars"], case["vars"])
    for mode in ("device", "host"):
        got, inputs = oa.Witness.from_zkif(inst, paths[1], paths[2], mode=mode)
        info = got.ingest_info()
        assert info["on_device"] == (mode == "device") and info["witness_bytes"] == os.path.getsize(paths[2])
        _assert_same_witness(inst, got, inputs, want, a)
    rep = got.check_sat(inst, max_rows=4)
    assert rep.n_unsat == 0


@pytest.mark.parametrize("name,n,ni,compiler", [("u48", 48, 3, False), ("c48", 48, 3, True), ("u1000", 1000, 10, False), ("c1000", 1000, 10, True)])
def test_nizk_proof_bytes_are_the_uploads_and_the_oracles(work, name, n, ni, compiler):
    paths, r = zc.product_triple(work, name, n, ni, compiler)
    inst, _ = oa.Instance.from_zkif(paths[0], paths[1], mode="device")
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    want, a = _host_pair(inst, paths)
    got, inputs = oa.Witness.from_zkif(inst, paths[1], paths[2], mode="device")
    _assert_same_witness(inst, got, inputs, want, a)
    print(f"{name}: witness {got.ingest_info()['witness_bytes']} B, small_fraction {got.info[2]:.4f}, laps (ms) {tuple(round(x, 3) for x in got.ingest_info()['ms'])}")
    proofs = [oa.NIZK.prove(inst, w, None, gens, LABEL, SEED) for w in (got, want)]
    oi, og = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"]), orc.OGens(r["num_cons"], r["num_vars"], r["num_inputs"])
    oracle, _ = orc.nizk_prove(oi, r["vars"], r["inputs"], og, LABEL, SEED)
    assert proofs[0].bytes == proofs[1].bytes == oracle
    proofs[0].verify(inst, oa.InputsAssignment.new(inputs), gens, LABEL)


def test_snark_proof_bytes_are_the_uploads(work):
    paths, r = zc.product_triple(work, "s200", 200, 3, compiler=True)
    inst, a = oa.Instance.from_zkif(*paths, mode="host")
    nnz = max(a["nA"], a["nB"], a["nC"])
    sg = oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nnz)
    comm = oa.ComputationCommitment.encode(inst, sg)
    want, _ = _host_pair(inst, paths)
    got, _ = oa.Witness.from_zkif(inst, paths[1], paths[2], mode="device")
    proofs = [oa.SNARK.prove(inst, comm, w, None, sg, b"snark_example", SEED).bytes for w in (got, want)]
    assert proofs[0] == proofs[1]


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_refusals_carry_the_host_pairs_code_and_the_context_stays_usable(work):
    base = wc.write_case(work, "base", wc._case(wc.fb.witness(wc.BASE_IDS, wc.BASE_VALS)))
    inst, _ = oa.Instance.from_zkif(*base, mode="host")
    assert _code(inst, base, "device") == (0, None)
    for name, case, code in wc.defect_cases() + wc.two_defect_cases():
        paths = wc.write_case(work, "bad_" + name, case)
        host, dev = _code(inst, paths, "host"), _code(inst, paths, "device")
        assert dev == host == (code, (0x1234, False)), (name, code, host, dev)
        if code != wc.BAD_ARG:                                             # (files of other dimensions: the host pair knows no such refusal)
            assert _host_pair_code(inst, paths) == code, name
    # the same process, the same context: a valid pair of files ingests and proves
    paths, r = zc.product_triple(work, "after", 300, 4)
    inst2, _ = oa.Instance.from_zkif(paths[0], paths[1], mode="device")
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    wit, inputs = oa.Witness.from_zkif(inst2, paths[1], paths[2], mode="device")
    oa.NIZK.prove(inst2, wit, None, gens, LABEL, SEED).verify(inst2, oa.InputsAssignment.new(inputs), gens, LABEL)
    # the first 200 mutants of the corpus the sanitizer run reads on the CPU: verdict and code equal the host pair's for each
    mb = wc.mutant_base()
    mpaths = wc.write_case(work, "mutant_base", mb)
    minst, _ = oa.Instance.from_zkif(*mpaths, mode="host")
    verdicts = {}
    for i, m in enumerate(wc.mutants(mb["witness"], 200)):
        p = os.path.join(work, "mutant.wit.zkif")
        with open(p, "wb") as f:
            f.write(m)
        trio = (mpaths[0], mpaths[1], p)
        want = _host_pair_code(minst, trio)
        host, dev = _code(minst, trio, "host"), _code(minst, trio, "device")
        assert dev[0] == host[0] == want and dev == host, (i, want, host, dev)
        verdicts[want] = verdicts.get(want, 0) + 1
    print("mutant verdicts (code: files):", verdicts)
    assert verdicts.get(0, 0) > 0 and len(verdicts) > 1
    oa.NIZK.prove(inst2, oa.Witness.from_zkif(inst2, paths[1], paths[2], mode="device")[0], None, gens, LABEL, SEED).verify(inst2, oa.InputsAssignment.new(inputs), gens, LABEL)


# ------------------------------------------------------------------------------------------------ 3. dependent state
def test_kept_rows_and_products_follow_the_mutators_of_a_device_ingested_witness(work, monkeypatch):
    """the circuit every assignment satisfies (witness_cases.Case), so that the oracle judges the proof after each change"""
    monkeypatch.setenv("OTTI_MSM_WINDOW", "9")                     # a narrow table, whose width does not depend on what else ran in this process
    c = case(10)
    rng = np.random.default_rng(20260303)
    cur = values(rng, c.V)
    paths = tuple(os.path.join(work, "kept" + ext) for ext in (".zkif", ".inp.zkif", ".wit.zkif"))
    nv, _, ni, A, B, C = c.args
    oa.zkif_write(dict(num_cons=nv, num_vars=nv, num_inputs=ni, A=A, B=B, C=C, vars=bytes32(cur), inputs=c.inputs32), *paths)
    wit, inputs = oa.Witness.from_zkif(c.inst, paths[1], paths[2], mode="device")
    assert wit.ingest_info()["on_device"] and _same(inputs, c.inputs32)
    wit.keep_rows(c.inst, c.gens)
    wit.keep_products(c.inst)
    c.check(wit, cur, b"ingested")
    idx = np.array([3, 500, 999], dtype=np.uint64)
    new = np.array([7, 2 ** 40 + 1, 12345], dtype=np.uint64)
    wit.scatter(c.inst, idx, new)
    for i, v in zip(idx, new):
        cur[int(i)] = int(v)
    c.check(wit, cur, b"scattered")
    cur[17], cur[640] = Q - 2, (cur[640] + 1) % Q
    assert wit.assign(c.inst, bytes32(cur)) == 2
    fresh = c.host_witness(cur)
    assert _same(z_of(wit)[0], z_of(fresh)[0]) and wit.info[2] == fresh.info[2]
    assert wit.rows_info()[0] and wit.scatter_info()[0] == 1 and wit.assign_info()[:2] == (1, 2)
    assert wit.check_sat(c.inst, max_rows=4).n_unsat == 0
    c.check(wit, cur, b"assigned")
    wit.update(c.inst, 100, bytes32([5, 6, 7]))
    cur[100:103] = [5, 6, 7]
    new_inputs = bytes32([Q - 1, 4])
    wit.set_inputs(c.inst, new_inputs)
    c.check(wit, cur, b"updated", inputs32=new_inputs)


# ------------------------------------------------------------------------------------------------ 4. AUTO
def test_auto_takes_the_host_or_the_device_by_the_witness_files_size(work, monkeypatch):
    paths, _ = zc.product_triple(work, "auto", 1024, 10)
    inst, _ = oa.Instance.from_zkif(paths[0], paths[1], mode="host")
    mb = os.path.getsize(paths[2]) / 1048576.0
    monkeypatch.setenv("OTTI_INGEST_WIT_MIN_MB", repr(mb * 1.01))
    assert not oa.Witness.from_zkif(inst, paths[1], paths[2])[0].ingest_info()["on_device"]
    monkeypatch.setenv("OTTI_INGEST_WIT_MIN_MB", repr(mb * 0.99))
    assert oa.Witness.from_zkif(inst, paths[1], paths[2], mode="auto")[0].ingest_info()["on_device"]
    monkeypatch.setenv("OTTI_INGEST_WIT_MIN_MB", "0")
    assert oa.Witness.from_zkif(inst, paths[1], paths[2])[0].ingest_info()["on_device"]
    monkeypatch.delenv("OTTI_INGEST_WIT_MIN_MB")
    assert oa.Witness.from_zkif(inst, paths[1], paths[2])[0].ingest_info()["on_device"] == (mb >= oa.lib.otti_witness_ingest_min_mb())


# ------------------------------------------------------------------------------------------------ 5. served
def test_served_request_ingests_the_witness_on_the_device(work):
    env = dict(os.environ, OTTI_MSM_WINDOW="10", OTTI_MSM_TABLE_GB="1")
    env.pop("SPZK_SERVER", None)
    pre = os.path.join(work, "served")
    assert subprocess.run([SPZK, "synth", "1024", pre, "3", "2"], capture_output=True, timeout=120).returncode == 0
    with open(pre + ".wit.zkif", "rb") as f:
        good = f.read()
    body = bytearray(good[4:])
    at = wc.locate(body)
    last = at["vals"] + 4 + 32 * (zc._u32(body, at["ids"]) - 1)
    body[last:last + 32] = b"\xff" * 32                                     # the last value is 2^256 - 1
    with open(pre + ".bad.wit.zkif", "wb") as f:
        f.write(good[:4] + bytes(body))
    argv = ["verify", "--nizk", "served.zkif", "served.inp.zkif", "served.wit.zkif", "--seed", "2a" * 32, "--proof-out"]
    bad_argv = ["verify", "--nizk", "served.zkif", "served.inp.zkif", "served.bad.wit.zkif", "--seed", "2a" * 32]
    one = subprocess.run([SPZK] + argv + ["served.one"], cwd=work, env=env, capture_output=True, text=True, timeout=120)
    one_bad = subprocess.run([SPZK] + bad_argv, cwd=work, env=env, capture_output=True, text=True, timeout=120)
    assert one.returncode == 0, one.stderr
    assert one_bad.returncode == 1 and "(-5)" in one_bad.stderr, one_bad.stdout + one_bad.stderr
    srv = SpzkServer(socket_path=os.path.join(work, "sock"), jobs=1, idle_exit=300, env=dict(env, OTTI_INGEST_MIN_MB="0", OTTI_INGEST_WIT_MIN_MB="0"), start_timeout=120)
    srv.start()
    try:
        via = srv.run(argv + ["served.via"], cwd=work, timeout=120)
        via_bad = srv.run(bad_argv, cwd=work, timeout=120)
        again = srv.run(argv + ["served.again"], cwd=work, timeout=120)
    finally:
        status = srv.close(timeout=120)
    assert status == 0 and srv.abnormal_end is None

    def normal(stdout):
        return [re.sub(r"[0-9.]+ ms", "N ms", "<start or served>" if l.startswith(("* process start to main()", "* served:")) else l) for l in stdout.splitlines()]
    for v, name in ((via, "served.via"), (again, "served.again")):
        assert v.returncode == 0 and v.stderr == one.stderr and normal(v.stdout) == normal(one.stdout), v.stdout + v.stderr
        assert open(os.path.join(work, name), "rb").read() == open(os.path.join(work, "served.one"), "rb").read()
        served = [l for l in v.stdout.splitlines() if l.startswith("* served:")]
        assert len(served) == 1 and "witness device" in served[0] and served[0].endswith(", ingest device"), served
    assert (via_bad.returncode, via_bad.stderr, normal(via_bad.stdout)) == (one_bad.returncode, one_bad.stderr, normal(one_bad.stdout)), via_bad.stdout + via_bad.stderr
