"""otti_witness_assign / otti_witness_diff: a resident witness set from a whole new vector, of which the library finds the changed elements itself
(k_field.hip k_witness_diff_*), writes only those and brings kept rows up to date by the changes alone — patched as a scatter patches them, or the
touched rows summed again (OTTI_ASSIGN_RESUM_SHARE pins either path here, whatever the measured switch is).

The judge of every proof is the CPU oracle (orc.nizk_prove / orc.snark_prove) on an assignment kept in Python integers, byte for byte; z and
small_fraction are judged by a fresh upload of the same integers; counts and index lists by the pure-Python model of assign_cases.py.  That kept
rows are USED is read off the launch counters: a proof from them makes one fixed-base MSM launch fewer than one from a fresh witness.

The circuit is satisfied by EVERY assignment (row i: (k_i * v_i) * 1 = k_i * v_i).  Sizes: 2^5 (L = 4, R = 8), 2^10 (L = R = 32), 2^12 (L = R = 64):
the smallest with two rows and more, a range inside one row and a range across rows; 2^12 spans four of the comparison's chunks."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import otti_amd as oa
import orc
import assign_cases as ac
import witness_assign_worker as W
from witness_cases import Dev, Q, SEED, bytes32, case, msm_launches, values, z_of

pytestmark = pytest.mark.gpu
C32, M32, I64, U64 = oa.WIT_CANONICAL32, oa.WIT_MONTGOMERY32, oa.WIT_I64, oa.WIT_U64
INVALID_SCALAR = -5
HERE = os.path.dirname(os.path.abspath(__file__))
_vp = ctypes.c_void_p


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(autouse=True)
def _pinned_window(monkeypatch):
    monkeypatch.setenv("OTTI_MSM_WINDOW", "9")                 # a narrow table, whose width does not depend on what else ran in this process


def moved(rng, cur, k, first=0, count=None):
    """(a copy of cur in which exactly k uniformly placed elements of [first, first + count) have another value, their positions)"""
    count = len(cur) - first if count is None else count
    pos = sorted(first + int(j) for j in rng.choice(count, size=k, replace=False))
    new = list(cur)
    for i, v in zip(pos, values(rng, k)):
        new[i] = v if v != cur[i] else (v + 1) % Q
    return new, pos


def state(wit):
    return wit.rows_info(), wit.scatter_info(), wit.assign_info(), wit.info


def same_as_fresh(c, wit, cur):
    z, sf = z_of(wit)
    zf, sff = z_of(c.host_witness(cur))
    assert np.array_equal(z, zf), "z differs from a fresh upload's"
    assert sf == sff, (sf, sff)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("kept", [True, False], ids=["kept rows", "no rows"])
@pytest.mark.parametrize("ell", [5, 10, 12])
def test_assign_gives_a_fresh_uploads_witness_and_the_oracles_proof(rng, ell, kept):
    c = case(ell)
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    if kept:
        wit.keep_rows(c.inst, c.gens)
    calls = changed = 0
    for k in (1, c.R, c.V // 2, c.V):
        cur, pos = moved(rng, cur, k)
        assert wit.diff(c.inst, bytes32(cur), max_indices=0)[0] == k
        assert wit.assign(c.inst, bytes32(cur)) == k
        calls += 1; changed += k
        assert wit.assign_info()[:2] == (calls, changed)
        assert wit.scatter_info()[0] == 0
        same_as_fresh(c, wit, cur)
        c.check(wit, cur, b"assign %d" % k)
    n_wit = msm_launches(lambda: c.check(wit, cur, b"count"))
    n_fresh = msm_launches(lambda: c.check(c.host_witness(cur), cur, b"count"))
    assert n_fresh - n_wit == (1 if kept else 0), (n_fresh, n_wit)


@pytest.fixture(scope="module")
def snark():
    c = case(10)
    nz = c.V
    sg = oa.SNARKGens.new(c.V, c.V, 2, nz)
    comm = oa.ComputationCommitment.encode(c.inst, sg)
    og = orc.OSnarkGens(c.V, c.V, 2, nz)
    oc = orc.OSnarkComm.encode(c.oinst, og)
    assert comm.bytes == oc.bytes
    return sg, comm, og, oc


def test_assign_serves_a_snark_proof(rng, snark):
    c = case(10)
    sg, comm, og, oc = snark
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, sg)
    cur, pos = moved(rng, cur, 50)
    assert wit.assign(c.inst, bytes32(cur)) == 50
    got = oa.SNARK.prove(c.inst, comm, wit, None, sg, b"snark assign", SEED).bytes
    assert got == orc.snark_prove(c.oinst, oc, bytes32(cur), c.inputs32, og, b"snark assign", SEED)[0]


# ------------------------------------------------------------------------------------------------ 2. both kept-row paths
@pytest.mark.parametrize("share", ["2", "0"], ids=["patch", "re-sum"])
@pytest.mark.parametrize("ell", [5, 10, 12])
def test_both_kept_row_paths_move_their_own_counters(rng, monkeypatch, ell, share):
    monkeypatch.setenv("OTTI_ASSIGN_RESUM_SHARE", share)
    c = case(ell)
    R = c.R
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    for k in (1, R, c.V // 2, c.V):
        (_, _, _, resummed), (sc, rows_p, terms_p), (calls, changed, resums), _ = state(wit)
        cur, pos = moved(rng, cur, k)
        assert wit.assign(c.inst, bytes32(cur)) == k
        if share == "2":
            want = ((True, c.L, R, resummed), (sc, rows_p + len({i // R for i in pos}), terms_p + k), (calls + 1, changed + k, resums))
        else:
            want = ((True, c.L, R, resummed + pos[-1] // R - pos[0] // R + 1), (sc, rows_p, terms_p), (calls + 1, changed + k, resums + 1))
        assert state(wit)[:3] == want, k
        c.check(wit, cur, b"path %s, %d" % (share.encode(), k))
    n_wit = msm_launches(lambda: c.check(wit, cur, b"count"))
    assert msm_launches(lambda: c.check(c.host_witness(cur), cur, b"count")) - n_wit == 1


# ------------------------------------------------------------------------------------------------ 3. nothing changed
@pytest.mark.parametrize("ell", [5, 10, 12])
def test_an_unchanged_vector_writes_and_launches_nothing(rng, ell):
    c = case(ell)
    ints = [int(x) for x in rng.integers(-2 ** 63, 2 ** 63 - 1, size=c.V, endpoint=True)]
    ints[:4] = [-5, -2 ** 63, 2 ** 63 - 1, 0]
    cur = [x % Q for x in ints]
    wit = c.host_witness(cur)                                   # resident from canonical bytes: l - 5 and its like
    wit.keep_rows(c.inst, c.gens)
    z0 = z_of(wit)[0]
    d_mont = Dev(oa.fr_from_ints(cur))
    sources = [np.array(ints, dtype=np.int64), bytes32(cur), (d_mont.addr, c.V)]     # the same values in three other clothes
    for k, src in enumerate(sources):
        before = state(wit)
        oa.stats_enable(True)
        try:
            n = wit.assign(c.inst, src, fmt=M32 if isinstance(src, tuple) else None)
            s = oa.stats_read()
        finally:
            oa.stats_enable(False)
        assert n == 0
        launches = {name: v[0] for name, v in s.items() if v[0]}
        assert launches == {"other": 1}, launches                # the comparison (count and scan in one scope) and nothing after it: no apply, no patch, no MSM
        (rows, sc, (calls, changed, resums), info) = state(wit)
        assert (rows, sc, info) == (before[0], before[1], before[3])
        assert (calls, changed, resums) == (before[2][0] + 1, before[2][1], before[2][2])
    assert np.array_equal(z_of(wit)[0], z0)
    assert wit.assign(c.inst, np.array([], dtype=np.int64)) == 0                    # count = 0: not even a call
    assert wit.assign_info() == (len(sources), 0, 0)
    c.check(wit, cur, b"unchanged")


# ------------------------------------------------------------------------------------------------ 4. a sub-range
@pytest.mark.parametrize("share", ["2", "0"], ids=["patch", "re-sum"])
@pytest.mark.parametrize("ell", [5, 10, 12])
def test_a_sub_range_leaves_the_rest_alone(rng, monkeypatch, ell, share):
    monkeypatch.setenv("OTTI_ASSIGN_RESUM_SHARE", share)
    c = case(ell)
    R = c.R
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)

    def rows_moved(before, pos):
        """the kept-row counters after an assign that changed `pos`, by the pinned path"""
        (_, _, _, resummed), (sc, rows_p, terms_p), _, _ = before
        if share == "2":
            return (True, c.L, R, resummed), (sc, rows_p + len({i // R for i in pos}), terms_p + len(pos))
        return (True, c.L, R, resummed + pos[-1] // R - pos[0] // R + 1), (sc, rows_p, terms_p)

    first, count = R - 3, R + 5                                  # the range lies across rows 0 .. 2, the changes in row 1 alone:
    pos = [R, R + 2, 2 * R - 2, 2 * R - 1]                       # positions in the range (3 .. R + 2) would name rows 0 .. 1
    theirs = [(x + 7) % Q for x in cur]                          # the caller's notion of the whole vector differs everywhere ...
    new = list(cur)
    for i in pos:
        new[i] = (cur[i] + 1 + i) % Q
    theirs[first:first + count] = new[first:first + count]      # ... but only the range is handed over
    n, idx = wit.diff(c.inst, bytes32(theirs[first:first + count]), first=first)
    assert (n, idx.tolist()) == (4, pos)                         # indices are positions in the witness, not in the source
    before = state(wit)
    assert wit.assign(c.inst, bytes32(theirs[first:first + count]), first=first) == 4
    assert state(wit)[:2] == rows_moved(before, pos)
    same_as_fresh(c, wit, new)
    c.check(wit, new, b"sub-range, one row")
    cur = new                                                    # uniformly placed changes in the same range: rows 0 .. 2 as they fall
    new, pos = moved(rng, cur, 5, first, count)
    before = state(wit)
    assert wit.assign(c.inst, bytes32(new[first:first + count]), first=first) == 5
    assert state(wit)[:2] == rows_moved(before, pos)
    c.check(wit, new, b"sub-range, as they fall")
    # the last elements, one row: a range that ends with the vector
    cur = new
    new = list(cur); new[c.V - 1] = (cur[c.V - 1] + 1) % Q
    before = state(wit)
    assert wit.assign(c.inst, bytes32(new[c.V - 2:]), first=c.V - 2) == 1
    assert state(wit)[:2] == rows_moved(before, [c.V - 1])
    c.check(wit, new, b"the end")
    with pytest.raises(oa.R1CSError) as e:
        wit.assign(c.inst, bytes32(new[:2]), first=c.V - 1)
    assert e.value.code == -4


# ------------------------------------------------------------------------------------------------ 5. sources
def test_sources_and_formats(rng):
    c = case(10)
    R, V = c.R, c.V
    ints = [int(x) for x in rng.integers(-2 ** 40, 2 ** 40, size=V)]
    cur = [x % Q for x in ints]
    wit = oa.Witness.from_ints(c.inst, np.array(ints, dtype=np.int64), c.inputs)
    wit.keep_rows(c.inst, c.gens)
    KD = oa.kernels_dev
    stream = KD.stream_create()
    try:
        ints[5], ints[R], ints[V - 1] = -2 ** 63, 2 ** 63 - 1, -ints[V - 1] - 1     # host int64
        assert wit.assign(c.inst, np.array(ints, dtype=np.int64)) == 3
        cur = [x % Q for x in ints]
        c.check(wit, cur, b"host i64")
        r = orc.rand_fr(rng, 10)                                                  # a device source that a kernel queued on the caller's stream writes:
        buf = oa.DeviceArray(V)                                                   # the eq table of ten random variables, Montgomery words
        assert oa.lib.otti_dev_upload(buf.ptr, np.ascontiguousarray(oa.fr_from_ints(cur)).ctypes.data_as(_vp), 32 * V) == 0   # until it has run: no change
        KD.eq_evals(r, buf, stream)                                               # queued on the caller's stream ...
        n = wit.assign(c.inst, (buf, V), fmt=M32, stream=stream)                  # ... and read without a synchronisation in between
        new = [int(x) for x in orc.fr_to_ints(orc.eq_evals(r))]
        assert n == len(ac.model_diff(cur, new, C32)[0]) and n > V // 2
        cur = new
        same_as_fresh(c, wit, cur)
        c.check(wit, cur, b"device montgomery written on a caller's stream")
        new, pos = moved(rng, cur, 70)                                            # device canonical bytes
        d = Dev(bytes32(new))
        assert wit.assign(c.inst, (d.addr, V), fmt=C32) == 70
        cur = new
        c.check(wit, cur, b"device canonical")
        new, pos = moved(rng, cur, 33)                                            # device Montgomery words, strided by 64 bytes
        words = np.zeros((V, 64), dtype=np.uint8)
        words[:, :32] = oa.fr_from_ints(new)
        dm = Dev(words)
        assert wit.assign(c.inst, (dm.addr, V), fmt=M32, stride_bytes=64, stream=stream) == 33
        cur = new
        c.check(wit, cur, b"device montgomery, strided")
        small = [int(x) for x in rng.integers(0, 2 ** 64 - 1, size=R, endpoint=True, dtype=np.uint64)]   # host uint64 over one row
        assert wit.assign(c.inst, np.array(small, dtype=np.uint64), first=3 * R) == len([1 for a, b in zip(small, cur[3 * R:4 * R]) if a != b])
        cur[3 * R:4 * R] = small
        same_as_fresh(c, wit, cur)
        c.check(wit, cur, b"host u64")
        assert wit.scatter_info()[0] == 0
    finally:
        KD.stream_sync(stream)
        KD.stream_destroy(stream)


def test_torch_tensor_on_a_torch_stream_gives_the_oracles_proof():
    r, new, n_changed = W.assign_case()
    oinst = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    ogens = orc.OGens(r["num_cons"], r["num_vars"], r["num_inputs"])
    want = hashlib.sha256(orc.nizk_prove(oinst, bytes32([int(x) for x in new]), r["inputs"], ogens, W.LABEL, W.SEED)[0]).hexdigest()
    res = subprocess.run([sys.executable, os.path.join(HERE, "witness_assign_worker.py")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"the child ended with status {res.returncode}:\n{res.stdout}\n{res.stderr}"      # nothing further is started after a fault
    lines = res.stdout.split("\n")
    # setup_module has seen the device: a torch that does not see it is a failure here, not a skip
    assert not any(ln.startswith("skip ") for ln in lines), res.stdout + res.stderr
    got = dict(ln.split()[1:] for ln in lines if ln.startswith("digest "))
    assert got == {"int64_tensor": want, "changed": str(n_changed)}, res.stdout + res.stderr


# ------------------------------------------------------------------------------------------------ 6. refusal
@pytest.mark.parametrize("where", ["host", "device"])
def test_a_refused_scalar_leaves_everything_as_it_was(rng, where):
    c = case(10)
    V = c.V
    cur = values(rng, V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    cur, _ = moved(rng, cur, 9)
    assert wit.assign(c.inst, bytes32(cur)) == 9
    before = state(wit)
    z0 = z_of(wit)[0]
    l32 = np.frombuffer(Q.to_bytes(32, "little"), dtype=np.uint8)
    for fmt in (C32, M32):
        for k in (V // 2, V - 1):                                # a scalar = l in the middle and at the end, real changes before it
            new, _ = moved(rng, cur, 40)
            src = np.ascontiguousarray(bytes32(new) if fmt == C32 else oa.fr_from_ints(new)).copy()
            src[k] = l32
            keep = Dev(src) if where == "device" else None
            arg = (keep.addr, V) if where == "device" else src
            for call in (lambda: wit.assign(c.inst, arg, fmt=fmt), lambda: wit.diff(c.inst, arg, fmt=fmt)):
                with pytest.raises(oa.R1CSError) as e:
                    call()
                assert e.value.code == INVALID_SCALAR
                assert state(wit) == before
    assert np.array_equal(z_of(wit)[0], z0)
    c.check(wit, cur, b"after refusals")                         # the kept rows still belong to z
    assert msm_launches(lambda: c.check(wit, cur, b"count")) + 1 == msm_launches(lambda: c.check(c.host_witness(cur), cur, b"count"))


# ------------------------------------------------------------------------------------------------ 7. diff
@pytest.mark.parametrize("ell", [5, 10, 12])
def test_diff_counts_and_lists_without_touching_the_witness(rng, ell):
    c = case(ell)
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    z0 = z_of(wit)[0]
    before = state(wit)
    for k in (0, 1, 7, c.V // 2, c.V):
        new, pos = moved(rng, cur, k)
        want_idx, _ = ac.model_diff(cur, new, C32)
        assert want_idx == pos
        src = bytes32(new) if k % 2 else Dev(bytes32(new))
        arg = src if k % 2 else (src.addr, c.V)
        for cap in (0, 1, 64, c.V + 5):
            n, idx = wit.diff(c.inst, arg, fmt=C32, max_indices=cap)
            assert n == k and idx.dtype == np.uint64
            assert idx.tolist() == pos[:min(k, cap)], (k, cap)
        assert state(wit) == before
    assert np.array_equal(z_of(wit)[0], z0)
    new, pos = moved(rng, cur, 7)
    assert wit.diff(c.inst, bytes32(new))[0] == 7 and wit.assign(c.inst, bytes32(new)) == 7      # a following assign finds the same
    assert wit.diff(c.inst, bytes32(new))[0] == 0
    c.check(wit, new, b"after diff")


# ------------------------------------------------------------------------------------------------ 8. one consistent state
def test_assign_scatter_update_assign_on_one_witness(rng):
    c = case(10)
    R = c.R
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    cur, pos = moved(rng, cur, 20)
    assert wit.assign(c.inst, bytes32(cur)) == 20
    c.check(wit, cur, b"1 assign")
    idx, new = [1, R + 2, 9 * R], values(rng, 3)
    wit.scatter(c.inst, np.array(idx, dtype=np.int64), bytes32(new))
    for j, x in zip(idx, new):
        cur[j] = x
    c.check(wit, cur, b"2 scatter")
    new = values(rng, R + 3)
    wit.update(c.inst, R - 1, bytes32(new))                     # rows 0 .. 2
    cur[R - 1:2 * R + 2] = new
    c.check(wit, cur, b"3 update")
    cur, pos2 = moved(rng, cur, 2 * R)
    assert wit.assign(c.inst, bytes32(cur)) == 2 * R
    c.check(wit, cur, b"4 assign")
    assert wit.assign_info()[:2] == (2, 20 + 2 * R) and wit.scatter_info()[0] == 1
    same_as_fresh(c, wit, cur)
