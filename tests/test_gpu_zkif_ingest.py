"""Circuit ingest on the device (otti_instance_from_zkif, k_ingest.hip) against the host path: the same instance — dimensions, entries in file
order, sparse-kernel variants, products, verdicts, proof and commitment bytes — for the product writer's files and for layouts it never writes;
the host path's error code for every single-defect file and for the first 200 mutants the sanitizer run (tests/test_zkif_walk_host.py) has already
walked on the CPU; the AUTO rule; the lazy download under a concurrent proof; and a served request.  Nothing here is expected to fault: every file
is read through the bounds-checked walker the CPU run has exercised on the same bytes."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import otti_amd as oa
import orc
import zkif_ingest_cases as zc
from otti_amd.serve import SPZK, SpzkServer

pytestmark = pytest.mark.gpu
K = oa.kernels
SEED = b"\x2a" * 32
LABEL = b"nizk_example"


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(scope="module")
def work():
    d = tempfile.mkdtemp(prefix="zkif-ingest-")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _pair(paths):
    (hi, ha), (di, da) = oa.Instance.from_zkif(*paths, mode="host"), oa.Instance.from_zkif(*paths, mode="device")
    assert not hi.ingest_info()["on_device"] and di.ingest_info()["on_device"]
    return hi, ha, di, da


def _code(paths, mode):
    """(error code or 0, instance handle value afterwards) through the C call: *inst must stay what it was on an error"""
    h, rp = ctypes.c_void_p(0x1234), ctypes.POINTER(oa.api._R1CS)()
    rc = oa.lib.otti_instance_from_zkif(*(None if p is None else os.fsencode(p) for p in paths), oa.api.INGEST_MODES[mode], ctypes.byref(h), ctypes.byref(rp))
    if rc == 0:
        oa.lib.otti_r1cs_free(rp); oa.lib.otti_instance_free(h)
        return 0, None
    return rc, (h.value, bool(rp))


def _assert_same_instance(hi, ha, di, da):
    assert di.dims == hi.dims
    for k, name in enumerate("ABC"):
        assert da["n" + name] == ha["n" + name]
    for by_col in (False, True):                                           # before anything asks for the host lists: counts come from stored numbers
        assert di.device_info(by_col) == hi.device_info(by_col), by_col
    for k in range(3):
        assert _same(di.entries(k), hi.entries(k)), "ABC"[k]
    assert (da["num_cons"], da["num_vars"], da["num_inputs"]) == (ha["num_cons"], ha["num_vars"], ha["num_inputs"])
    assert _same(da["vars"], ha["vars"]) and _same(da["inputs"], ha["inputs"])


@pytest.mark.parametrize("name,n,ni,compiler", [("u1024", 1024, 10, False), ("c5000", 5000, 3, True), ("u65573", 65536 + 37, 10, False)])
def test_parity_with_the_host_path(work, name, n, ni, compiler):
    paths, _ = zc.product_triple(work, name, n, ni, compiler)
    hi, ha, di, da = _pair(paths)
    _assert_same_instance(hi, ha, di, da)
    info = di.ingest_info()
    total = sum(da["n" + x] for x in "ABC")
    print(f"{name}: circuit {info['circuit_bytes']} B, kept entries {info['hbm_entry_bytes']} B, laps (ms) {tuple(round(x, 3) for x in info['ms'])}")
    assert info["circuit_bytes"] == os.path.getsize(paths[0]) and info["hbm_entry_bytes"] == 40 * total
    ncp, nvp, _ = di.dims
    z = np.zeros((2 * nvp, 32), dtype=np.uint8)
    z[:da["vars"].shape[0]] = da["vars"]; z[nvp, 0] = 1; z[nvp + 1:nvp + 1 + ni] = da["inputs"]
    zm = K.from_canonical(z)
    for got, want in zip(K.multiply_vec(di, zm)[:3], K.multiply_vec(hi, zm)[:3]):
        assert _same(got, want)
    bad = da["vars"].copy(); bad[n // 3, 0] ^= 1                           # one variable off: some rows fail, the same ones through both instances
    for v in (da["vars"], bad):
        reps = [oa.Witness(inst, oa.VarsAssignment.new(v), oa.InputsAssignment.new(da["inputs"])).check_sat(inst, max_rows=16) for inst in (di, hi)]
        assert reps[0].n_unsat == reps[1].n_unsat and reps[0].rows.tolist() == reps[1].rows.tolist() and _same(reps[0].values, reps[1].values)
        assert (reps[0].n_unsat == 0) == (v is da["vars"])


def test_proof_bytes_are_the_host_paths_and_the_oracles(work):
    paths, r = zc.product_triple(work, "p1024", 1024, 10)
    hi, ha, di, da = _pair(paths)
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    proofs = [oa.NIZK.prove(inst, oa.VarsAssignment.new(a["vars"]), oa.InputsAssignment.new(a["inputs"]), gens, LABEL, SEED) for inst, a in ((di, da), (hi, ha))]
    oi, og = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"]), orc.OGens(r["num_cons"], r["num_vars"], r["num_inputs"])
    want, _ = orc.nizk_prove(oi, r["vars"], r["inputs"], og, LABEL, SEED)
    assert proofs[0].bytes == proofs[1].bytes == want
    proofs[0].verify(di, oa.InputsAssignment.new(da["inputs"]), gens, LABEL)


def test_computation_commitment_is_the_host_paths(work):
    """SNARK encode reads the host lists: the lazy download, in file order"""
    paths, r = zc.product_triple(work, "c200", 200, 3, compiler=True)
    hi, ha, di, da = _pair(paths)
    nnz = max(da["nA"], da["nB"], da["nC"])
    gens = oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nnz)
    assert oa.ComputationCommitment.encode(di, gens).bytes == oa.ComputationCommitment.encode(hi, gens).bytes


@pytest.mark.parametrize("name,circuit", zc.shaped_cases(), ids=[n for n, _ in zc.shaped_cases()])
def test_layouts_the_products_writer_does_not_produce(work, name, circuit):
    paths = zc.write_case(work, name, circuit)
    hi, ha, di, da = _pair(paths)
    _assert_same_instance(hi, ha, di, da)
    want = oa.zkif_load(*paths)
    for k, x in enumerate("ABC"):
        assert _same(di.entries(k), want[x])
    if name not in ("absent_table", "zero_ids") and want["num_cons"]:      # (a row without its B is not satisfied by the tiny system's assignment)
        assert di.is_sat(oa.VarsAssignment.new(da["vars"]), oa.InputsAssignment.new(da["inputs"]))


def test_refusals_carry_the_host_paths_code_and_the_context_stays_usable(work):
    for name, circuit in zc.defect_cases():
        paths = zc.write_case(work, "bad_" + name, circuit)
        host, dev = _code(paths, "host"), _code(paths, "device")
        assert host[0] != 0 and dev == host and dev[1] == (0x1234, False), (name, host, dev)
    # the same process, the same context: a valid file ingests and proves
    paths, r = zc.product_triple(work, "after", 300, 4)
    inst, a = oa.Instance.from_zkif(*paths, mode="device")
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    proof = oa.NIZK.prove(inst, oa.VarsAssignment.new(a["vars"]), oa.InputsAssignment.new(a["inputs"]), gens, LABEL, SEED)
    proof.verify(inst, oa.InputsAssignment.new(a["inputs"]), gens, LABEL)
    # the first 200 mutants of the corpus the sanitizer run walks on the CPU: verdict and code equal the host's for each
    base, _ = zc.product_triple(work, "uniform48", 48, 3)
    with open(base[0], "rb") as f:
        circuit = f.read()
    verdicts = {}
    for i, m in enumerate(zc.mutants(circuit, 200)):
        p = os.path.join(work, "mutant.zkif")
        with open(p, "wb") as f:
            f.write(m)
        host, dev = _code((p, base[1], base[2]), "host"), _code((p, base[1], base[2]), "device")
        assert dev == host, (i, host, dev)
        verdicts[host[0]] = verdicts.get(host[0], 0) + 1
    print("mutant verdicts (code: files):", verdicts)
    assert verdicts.get(0, 0) > 0 and len(verdicts) > 1


def test_a_coefficient_l_is_reported_behind_a_defective_witness(work):
    """instance_new finds a coefficient >= l only once zkif_load has finished, and zkif_load checks the assignment behind the constraints"""
    paths = zc.write_case(work, "l_and_witness", dict(zc.defect_cases())["coefficient_l"])
    with open(paths[2], "wb") as f:
        f.write(zc.fb.witness([2, 1], [3, 9]))                             # id 1 is the instance variable
    host, dev = _code(paths, "host"), _code(paths, "device")
    assert host[0] == -6 and dev == host, (host, dev)


def test_more_entries_than_32_bit_counts_hold_are_refused(work):
    """aliased offsets: 2^19 constraints sharing one table of 2^13 ids are 2^32 entries per matrix from 2.4 MB.  The 32-bit scan would wrap to a
    total of zero and an empty instance; the 64-bit sum of the count pass says so.  (The host loader has no such limit and would need 200 GB.)"""
    paths = zc.write_case(work, "too_many", zc.too_many_entries())
    dev = _code(paths, "device")
    assert dev == (-21, (0x1234, False)), dev
    paths, r = zc.product_triple(work, "after_many", 300, 4)               # the context is as usable as before
    inst, a = oa.Instance.from_zkif(*paths, mode="device")
    assert all(_same(inst.entries(k), r["ABC"[k]]) for k in range(3))


def test_auto_takes_the_host_or_the_device_by_the_files_size(work, monkeypatch):
    paths, _ = zc.product_triple(work, "auto", 1024, 10)
    oa.Instance.from_zkif(*paths, mode="device")                           # the runtime is up
    monkeypatch.setenv("OTTI_INGEST_GB", "0")
    monkeypatch.setenv("OTTI_INGEST_MIN_MB", "0")
    host, _ = oa.Instance.from_zkif(*paths, mode="auto")
    assert not host.ingest_info()["on_device"]
    monkeypatch.delenv("OTTI_INGEST_GB")
    dev, _ = oa.Instance.from_zkif(*paths)
    assert dev.ingest_info()["on_device"]
    for k in range(3):
        assert _same(dev.entries(k), host.entries(k))
    monkeypatch.setenv("OTTI_INGEST_MIN_MB", "1000000")
    assert not oa.Instance.from_zkif(*paths)[0].ingest_info()["on_device"]


def test_first_entries_call_beside_a_proof(work):
    paths, r = zc.product_triple(work, "threads", 4096, 5)
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    ref_inst, a = oa.Instance.from_zkif(*paths, mode="host")
    v, i = oa.VarsAssignment.new(a["vars"]), oa.InputsAssignment.new(a["inputs"])
    want = oa.NIZK.prove(ref_inst, v, i, gens, LABEL, SEED).bytes
    inst, _ = oa.Instance.from_zkif(*paths, mode="device")
    inst.prepare_device(gens)
    out = {}
    def prover():
        out["proof"] = oa.NIZK.prove(inst, v, i, gens, LABEL, SEED).bytes
    def reader():
        out["A"] = inst.entries(0)
    th = [threading.Thread(target=prover), threading.Thread(target=reader)]
    [t.start() for t in th]; [t.join(timeout=120) for t in th]
    assert out["proof"] == want and _same(out["A"], ref_inst.entries(0))


def test_served_request_ingests_on_the_device(work):
    env = dict(os.environ, OTTI_MSM_WINDOW="10", OTTI_MSM_TABLE_GB="1")
    env.pop("SPZK_SERVER", None)
    pre = os.path.join(work, "served")
    assert subprocess.run([SPZK, "synth", "1024", pre, "3", "2"], capture_output=True, timeout=120).returncode == 0
    argv = ["verify", "--nizk", "served.zkif", "served.inp.zkif", "served.wit.zkif", "--seed", "2a" * 32, "--proof-out"]
    one = subprocess.run([SPZK] + argv + ["served.one"], cwd=work, env=env, capture_output=True, text=True, timeout=120)
    assert one.returncode == 0, one.stderr
    srv = SpzkServer(socket_path=os.path.join(work, "sock"), jobs=1, idle_exit=300, env=dict(env, OTTI_INGEST_MIN_MB="0"), start_timeout=120)
    srv.start()
    try:
        via = srv.run(argv + ["served.via"], cwd=work, timeout=120)
    finally:
        status = srv.close(timeout=120)
    assert status == 0 and srv.abnormal_end is None

    def normal(stdout):
        return [re.sub(r"[0-9.]+ ms", "N ms", "<start or served>" if l.startswith(("* process start to main()", "* served:")) else l) for l in stdout.splitlines()]
    assert via.returncode == 0 and via.stderr == one.stderr and normal(via.stdout) == normal(one.stdout), via.stdout + via.stderr
    assert open(os.path.join(work, "served.via"), "rb").read() == open(os.path.join(work, "served.one"), "rb").read()
    served = [l for l in via.stdout.splitlines() if l.startswith("* served:")]
    assert len(served) == 1 and served[0].endswith(", ingest device"), served
