"""SNARK mode and sharded proofs from a device-ingested instance: the decommitment fill and the shard filter read the entry lists the ingest keeps
in HBM, so encode, attach and a sharded upload leave the host lists unmade (otti_instance_host_lists_info) and give the host instance's bytes; served
SNARK requests go through the device ingest.  Nothing here is expected to fault: both kernels write only positions below lengths the host has
checked (N, and the count the scan returned)."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import uuid

import numpy as np
import pytest

import otti_amd as oa
import zkif_ingest_cases as zc
from otti_amd.serve import SPZK, SpzkServer
from shard_worker import SEED, LABEL, make_r1cs

pytestmark = pytest.mark.gpu
K = oa.kernels
HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "shard_zkif_worker.py")
L = oa.L_ORDER


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(scope="module")
def work():
    d = tempfile.mkdtemp(prefix="snark-dev-")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _values(rng, n):
    """n canonical integers below l, the first ones 0, 1 and l - 1"""
    out = [0, 1, L - 1][:n]
    while len(out) < n:
        out.append(int.from_bytes(rng.bytes(32), "little") % L)
    return out


# ------------------------------------------------------------------------------------------------ the fill kernel against Python integers
@pytest.mark.parametrize("n,N,pad_to", [(0, 2, 0), (0, 2, 2), (1, 2, 2), (64, 64, 64), (65, 128, 65), (1000, 1024, 1000)])
def test_fill_kernel_against_python_integers(n, N, pad_to):
    rng = np.random.default_rng(100 + n + pad_to)
    row, col = rng.integers(0, 2 ** 31, n, dtype=np.uint32), rng.integers(0, 2 ** 31, n, dtype=np.uint32)
    if n > 3:
        row[1], col[2] = 0, 0                                               # a real entry at address 0
        row[3], col[3] = 2 ** 31 - 1, 2 ** 31 - 1
    vals = _values(rng, n)
    pad_col = 12345
    ru, cu, rf, cf, vf, ms = K.decomm_entries(row, col, oa.fr_from_ints(vals), N, pad_to=pad_to, pad_col=pad_col)
    want_row = [int(row[i]) if i < n else (i if i < pad_to else 0) for i in range(N)]
    want_col = [int(col[i]) if i < n else (pad_col if i < pad_to else 0) for i in range(N)]
    want_val = [vals[i] if i < n else 0 for i in range(N)]
    assert ru.tolist() == want_row and cu.tolist() == want_col
    assert [int.from_bytes(x.tobytes(), "little") for x in K.to_canonical(rf)] == want_row
    assert [int.from_bytes(x.tobytes(), "little") for x in K.to_canonical(cf)] == want_col
    assert vf.tobytes() == oa.fr_from_ints(want_val).tobytes()             # the Montgomery words themselves
    assert rf.tobytes() == oa.fr_from_ints(want_row).tobytes() and cf.tobytes() == oa.fr_from_ints(want_col).tobytes()
    print(f"fill n={n} N={N} pad_to={pad_to}: kernel {ms * 1e3:.1f} us")


# ------------------------------------------------------------------------------------------------ the filter kernel against numpy
@pytest.fixture(scope="module")
def filter_lists():
    """per n: (row, col, val) — made once, left alone.  The values are any 32 bytes: the filter only moves them."""
    rng = np.random.default_rng(7)
    return {n: (rng.integers(0, 2 ** 31, n, dtype=np.uint32), rng.integers(0, 2 ** 31, n, dtype=np.uint32), rng.integers(0, 256, (n, 32), dtype=np.uint8))
            for n in (0, 1, 63, 64, 65, 5000)}


def _filter_want(row, col, val, g, k, by_col):
    key = col if by_col else row
    sel = key % g == k
    return (row[sel] if by_col else row[sel] // g), (col[sel] // g if by_col else col[sel]), val[sel]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5000])
def test_filter_kernel_against_numpy(filter_lists, n):
    row, col, val = filter_lists[n]
    for g in (1, 2, 8):
        for k in range(g):
            for by_col in (False, True):
                r, c, v, _ = K.shard_filter(row, col, val, g, k, by_col)
                wr, wc, wv = _filter_want(row, col, val, g, k, by_col)
                assert r.tolist() == wr.tolist() and c.tolist() == wc.tolist() and v.tobytes() == wv.tobytes(), (n, g, k, by_col)


def test_filter_kernel_when_none_or_all_match():
    rng = np.random.default_rng(8)
    n = 300
    row = (rng.integers(0, 2 ** 27, n, dtype=np.uint32) * 8 + 3).astype(np.uint32)     # every row is 3 mod 8
    col = (rng.integers(0, 2 ** 27, n, dtype=np.uint32) * 8 + 5).astype(np.uint32)     # every column 5 mod 8
    val = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for k in range(8):
        for by_col in (False, True):
            r, c, v, _ = K.shard_filter(row, col, val, 8, k, by_col)
            wr, wc, wv = _filter_want(row, col, val, 8, k, by_col)
            assert r.size == (n if k == (5 if by_col else 3) else 0)
            assert r.tolist() == wr.tolist() and c.tolist() == wc.tolist() and v.tobytes() == wv.tobytes(), (k, by_col)


# ------------------------------------------------------------------------------------------------ encode and attach without host lists
@pytest.fixture(scope="module")
def circuits(work):
    """c200 and u1024: files, the host instance, generators, and the host instance's commitment and proof bytes — made once, left alone"""
    out = {}
    for name, n, ni, compiler in (("c200", 200, 3, True), ("u1024", 1024, 10, False)):
        paths, r = zc.product_triple(work, name, n, ni, compiler)
        hi, ha = oa.Instance.from_zkif(*paths, mode="host")
        gens = oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], max(ha["nA"], ha["nB"], ha["nC"]))
        comm = oa.ComputationCommitment.encode(hi, gens)
        proof = oa.SNARK.prove(hi, comm, oa.VarsAssignment.new(ha["vars"]), oa.InputsAssignment.new(ha["inputs"]), gens, LABEL, SEED)
        out[name] = dict(paths=paths, gens=gens, comm=comm.bytes, proof=proof.bytes, asg=ha)
    return out


@pytest.mark.parametrize("name", ["c200", "u1024"])
@pytest.mark.parametrize("how", ["encode", "attach"])
def test_encode_and_attach_leave_the_host_lists_unmade(circuits, name, how):
    c = circuits[name]
    di, da = oa.Instance.from_zkif(*c["paths"], mode="device")
    assert di.host_lists_info() == {"materialised": False, "host_bytes": 0}
    if how == "encode":
        comm = oa.ComputationCommitment.encode(di, c["gens"])
        assert comm.bytes == c["comm"]
    else:
        comm = oa.ComputationCommitment.from_bytes(c["comm"])
        comm.attach(di, c["gens"], verify=True)
    inputs = oa.InputsAssignment.new(da["inputs"])
    proof = oa.SNARK.prove(di, comm, oa.VarsAssignment.new(da["vars"]), inputs, c["gens"], LABEL, SEED)
    assert proof.bytes == c["proof"]
    proof.verify(oa.ComputationCommitment.from_bytes(c["comm"]), inputs, c["gens"], LABEL)
    assert di.host_lists_info() == {"materialised": False, "host_bytes": 0}
    di.entries(0)
    assert di.host_lists_info() == {"materialised": True, "host_bytes": 40 * (da["nA"] + da["nB"] + da["nC"])}


def test_a_commitment_of_another_circuit_is_still_refused_by_attach(circuits, work):
    paths, _ = zc.product_triple(work, "c200_other", 200, 3, True, seed=2)
    di, _ = oa.Instance.from_zkif(*paths, mode="device")
    comm = oa.ComputationCommitment.from_bytes(circuits["c200"]["comm"])
    with pytest.raises(oa.SpartanError):
        comm.attach(di, circuits["c200"]["gens"], verify=True)


def test_the_host_fill_switch_is_unchanged(circuits, work):
    """OTTI_DECOMM_HOST=1 (read once per process: a child): the A/B path still reads the host lists, and gives the same bytes"""
    out = os.path.join(work, "decomm_host.bin")
    res = subprocess.run([sys.executable, WORKER, "encode", out, os.path.join(work, "c200")], env=dict(os.environ, OTTI_DECOMM_HOST="1"), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert open(out, "rb").read() == circuits["c200"]["comm"]
    assert json.loads(res.stdout.splitlines()[-1])["materialised"] is True


def _c200_without_C(work):
    """A and B as in c200, C empty: matrices of different lengths, one of them empty (not satisfiable: encode only).  The product's writer, as
    product_triple uses it — write_case's tiny system has four variable ids."""
    r = oa.synth_r1cs_compiler_like(200, 3, 1)
    r = dict(r, C=r["C"][:0])
    paths = tuple(os.path.join(work, "c200_no_C" + ext) for ext in (".zkif", ".inp.zkif", ".wit.zkif"))
    oa.zkif_write(r, *paths)
    return paths


@pytest.mark.parametrize("shape", ["c200_no_C", "one_constraint", "no_constraints"])
def test_shapes_too_small_or_too_odd_for_a_proof_encode_alike(work, shape):
    paths = _c200_without_C(work) if shape == "c200_no_C" else zc.write_case(work, "shape_" + shape, dict(zc.shaped_cases())[shape])
    hi, ha = oa.Instance.from_zkif(*paths, mode="host")
    di, da = oa.Instance.from_zkif(*paths, mode="device")
    assert (da["nA"], da["nB"], da["nC"]) == (ha["nA"], ha["nB"], ha["nC"])
    if shape == "c200_no_C":
        assert da["nC"] == 0 and da["nA"] != da["nB"] and min(da["nA"], da["nB"]) > 0
    gens = oa.SNARKGens.new(ha["num_cons"], ha["num_vars"], ha["num_inputs"], max(ha["nA"], ha["nB"], ha["nC"]))
    assert oa.ComputationCommitment.encode(di, gens).bytes == oa.ComputationCommitment.encode(hi, gens).bytes
    # without a single entry there is nothing in HBM to read: that one instance goes the host-list way, as ever
    assert di.host_lists_info()["materialised"] == (da["nA"] + da["nB"] + da["nC"] == 0)


# ------------------------------------------------------------------------------------------------ a sharded proof from device-ingested instances
def _run_ranks(args_of_rank, world, timeout):
    env = dict(os.environ, OTTI_SHARD_TIMEOUT_S="60", OTTI_DEVICE="0")
    procs = [subprocess.Popen([sys.executable, WORKER] + args_of_rank(r), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            outs.append(o.decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r])
    return outs


def _write_r1cs(work, name, lg, dist, ni):
    r = make_r1cs(lg, dist, ni)
    prefix = os.path.join(work, name)
    oa.zkif_write(r, prefix + ".zkif", prefix + ".inp.zkif", prefix + ".wit.zkif")
    return prefix, r


def test_sharded_nizk_proof_from_device_ingested_instances(work, tmp_path):
    prefix, r = _write_r1cs(work, "shard_u10", 10, "uniform", 4)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    single = oa.NIZK.prove(inst, oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"]), gens, LABEL, SEED).bytes
    seg = "otti-test-" + uuid.uuid4().hex
    outs = _run_ranks(lambda k: ["prove", seg, str(k), "2", str(tmp_path / ("p%d.bin" % k)), prefix], 2, timeout=500)
    for k in range(2):
        assert open(tmp_path / ("p%d.bin" % k), "rb").read() == single, "rank %d returned different proof bytes" % k
        assert json.loads(outs[k].splitlines()[-1]) == {"materialised": False, "host_bytes": 0}, outs[k][-2000:]


def test_sharded_snark_proof_from_device_ingested_instances(work, tmp_path):
    prefix, r = _write_r1cs(work, "shard_c8", 8, "compiler", 3)
    nz = int(max(r["A"].size, r["B"].size, r["C"].size))
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nz)
    comm = oa.ComputationCommitment.encode(inst, gens)
    single = oa.SNARK.prove(inst, comm, oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"]), gens, LABEL, SEED).bytes
    seg = "otti-test-" + uuid.uuid4().hex
    outs = _run_ranks(lambda k: ["snark", seg, str(k), "2", str(tmp_path / ("s%d.bin" % k)), prefix], 2, timeout=900)
    for k in range(2):
        got = open(tmp_path / ("s%d.bin" % k), "rb").read()
        nc = int.from_bytes(got[:8], "little")
        assert got[8:8 + nc] == comm.bytes, "rank %d: another computation commitment" % k
        assert got[8 + nc:] == single, "rank %d returned different SNARK proof bytes" % k
        assert json.loads(outs[k].splitlines()[-1]) == {"materialised": False, "host_bytes": 0}, outs[k][-2000:]


# ------------------------------------------------------------------------------------------------ served SNARK requests
def _normal(stdout):
    """times, the one line that differs by design, and the output file's name as the request gave it (one.* / via.*)"""
    lines = [re.sub(r"[0-9.]+ ms", "N ms", "<start or served>" if l.startswith(("* process start to main()", "* served:")) else l) for l in stdout.splitlines()]
    return [re.sub(r"written to (one|via)\.", "written to X.", l) for l in lines]


def test_served_snark_requests_ingest_on_the_device(work):
    env = dict(os.environ, OTTI_MSM_WINDOW="10", OTTI_MSM_TABLE_GB="1")
    env.pop("SPZK_SERVER", None)
    assert subprocess.run([SPZK, "synth", "1024", os.path.join(work, "s"), "3", "2"], capture_output=True, timeout=120).returncode == 0
    bad = zc.write_case(work, "s_bad", dict(zc.defect_cases())["constraint_offset_beyond"])
    seed = ["--seed", "2a" * 32]
    files = ["s.zkif", "s.inp.zkif", "s.wit.zkif"]
    requests = [("verify", ["verify"] + files + seed + ["--proof-out"], ["%s.proof"]),
                ("encode", ["encode"] + files[:2] + ["--comm-out"], ["%s.comm"]),
                ("prove", ["prove"] + files + seed + ["--comm-in", "one.comm", "--proof-out"], ["%s.split"])]
    defect = ["verify"] + [os.path.basename(p) for p in bad]

    def one_shot(argv):
        return subprocess.run([SPZK] + argv, cwd=work, env=env, capture_output=True, text=True, timeout=120)
    ones = {name: one_shot(argv + [t % "one" for t in tail]) for name, argv, tail in requests}
    one_bad = one_shot(defect)
    assert all(o.returncode == 0 for o in ones.values()), [o.stderr for o in ones.values()]
    assert one_bad.returncode != 0
    srv = SpzkServer(socket_path=os.path.join(work, "sock"), jobs=1, idle_exit=300, env=dict(env, OTTI_INGEST_MIN_MB="0"), start_timeout=120)
    srv.start()
    try:
        vias = {name: srv.run(argv + [t % "via" for t in tail], cwd=work, timeout=120) for name, argv, tail in requests}
        via_bad = srv.run(defect, cwd=work, timeout=120)
    finally:
        status = srv.close(timeout=120)
    assert status == 0 and srv.abnormal_end is None
    for name, _, tail in requests:
        one, via = ones[name], vias[name]
        assert via.returncode == 0 and via.stderr == one.stderr and _normal(via.stdout) == _normal(one.stdout), name + "\n" + via.stdout + via.stderr
        f = tail[0]
        assert open(os.path.join(work, f % "via"), "rb").read() == open(os.path.join(work, f % "one"), "rb").read(), name
        served = [l for l in via.stdout.splitlines() if l.startswith("* served:")]
        assert len(served) == 1 and served[0].endswith(", ingest device"), (name, served)
    # the split proof, made from the stored commitment, is the combined request's
    assert open(os.path.join(work, "via.split"), "rb").read() == open(os.path.join(work, "via.proof"), "rb").read()
    assert (via_bad.returncode, via_bad.stderr, _normal(via_bad.stdout)) == (one_bad.returncode, one_bad.stderr, _normal(one_bad.stdout))
