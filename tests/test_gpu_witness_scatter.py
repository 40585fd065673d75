"""otti_witness_scatter: scattered variables of a resident witness replaced in one call, kept rows patched by (new - old) * P[column] instead of
summed again (k_msm.hip k_msm_scatter), and otti_witness_set_inputs.

The judge of every proof is the CPU oracle (orc.nizk_prove / orc.snark_prove) on an assignment kept in Python integers, byte for byte; the kernel
alone is judged by the oracle's commitment of a vector that holds the scalars at their indices and zero elsewhere.  That patched rows are USED
is read off the launch counters: a proof from them makes one fixed-base MSM launch fewer than one from a fresh witness.

The circuit is satisfied by EVERY assignment (row i: (k_i * v_i) * 1 = k_i * v_i).  Sizes: 2^5 (L = 4, R = 8), 2^10 (L = R = 32), 2^12 (L = R = 64);
the sub-chunk test runs the kernel over 2^18 generators (R = 512, two sub-chunks of kMsmScatterSub = 256 terms)."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import otti_amd as oa
import orc
import witness_scatter_worker as W
from witness_cases import Dev, Q, SEED, bytes32, case, msm_launches, values

pytestmark = pytest.mark.gpu
C32, M32, I64 = oa.WIT_CANONICAL32, oa.WIT_MONTGOMERY32, oa.WIT_I64
INVALID_INDEX, INVALID_SCALAR, INVALID_NUM_INPUTS = -6, -5, -3
SUB = 256                                                       # kMsmScatterSub
HERE = os.path.dirname(os.path.abspath(__file__))
_vp = ctypes.c_void_p


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(autouse=True)
def _pinned_window(monkeypatch):
    monkeypatch.setenv("OTTI_MSM_WINDOW", "9")                 # a narrow table, whose width does not depend on what else ran in this process


def patterns(L, R):
    """(name, indices, scalars or None for `mixed` values) over L rows of R"""
    V = L * R
    return [("one term", [R + 3], None), ("one per row", [i * R + (5 * i + 1) % R for i in range(L)], None),
            ("a full row", list(range(2 * R, 3 * R)), None), ("every index", list(range(V)), None),
            ("index 0 and the last", [0, V - 1], None), ("the pair R - 1, R", [R - 1, R], None),
            ("the scalars 0, 1, l - 1, 2^128", [1, R + 1, 2 * R - 1, V - 2], [0, 1, Q - 1, 2 ** 128])]


def dev_scatter(wit, inst, idx, src, fmt, stride=0, stream=None):
    """otti_witness_scatter with both lists in device memory; returns the status"""
    di, ds = Dev(np.array(idx, dtype=np.uint64)), Dev(src)
    return oa.lib.otti_witness_scatter(inst._h, wit._h, _vp(di.addr), _vp(ds.addr), len(idx), fmt, stride, 1, stream)


def sparse_commit(ogens, L, R, idx, s):
    Z = [0] * (L * R)
    for j, x in zip(idx, s):
        Z[j] = x
    return orc.commit_rows(ogens, orc.fr_from_ints(Z), L, R, orc.fr_from_ints([0] * L))


# ------------------------------------------------------------------------------------------------ 1. the kernel
def test_kernel_equals_the_oracles_commitment(rng):
    c = case(10)
    L, R = c.L, c.R
    for name, idx, s in patterns(L, R):
        s = values(rng, len(idx)) if s is None else s
        got, _ = oa.kernels.msm_scatter_rows(c.gens, L, idx, oa.fr_from_ints(s))
        assert np.array_equal(got, sparse_commit(c.ogens, L, R, idx, s)), name
    got, _ = oa.kernels.msm_scatter_rows(c.gens, L, [], oa.fr_from_ints([]))            # no terms: every row the identity
    assert not got.any()


# ------------------------------------------------------------------------------------------------ 2. sub-chunks
def test_kernel_sub_chunk_boundaries(rng):
    nv = 1 << 18
    gens, ogens = oa.NIZKGens.new(nv, nv, 1), orc.OGens(nv, nv, 1)
    R, L = ogens.R, 3
    assert R == 2 * SUB
    for name, counts in (("one sub-chunk, one more, two", (SUB, SUB + 1, R)), ("row 1 empty", (R, 0, R))):
        idx = [i * R + int(j) for i, n in enumerate(counts) for j in sorted(rng.choice(R, size=n, replace=False))]
        s = values(rng, len(idx), "large")
        got, _ = oa.kernels.msm_scatter_rows(gens, L, idx, oa.fr_from_ints(s))
        assert np.array_equal(got, sparse_commit(ogens, L, R, idx, s)), name
        if not counts[1]:
            assert not got[1].any()
    gens.release_device()


# ------------------------------------------------------------------------------------------------ 3 / 4. scatter, with and without kept rows
@pytest.mark.parametrize("kept", [True, False])
@pytest.mark.parametrize("ell", [5, 10, 12])
def test_scatter_gives_the_oracles_proof(rng, ell, kept):
    c = case(ell)
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    if kept:
        wit.keep_rows(c.inst, c.gens)
    calls = rows = terms = 0
    for name, idx, s in patterns(c.L, c.R):
        s = values(rng, len(idx)) if s is None else s
        wit.scatter(c.inst, np.array(idx, dtype=np.int64), bytes32(s))
        for j, x in zip(idx, s):
            cur[j] = x
        calls += 1
        if kept:
            rows += len({j // c.R for j in idx}); terms += len(idx)
        assert wit.scatter_info() == (calls, rows, terms), name
        assert wit.rows_info() == ((True, c.L, c.R, 0) if kept else (False, 0, 0, 0)), name
        c.check(wit, cur, name.encode())
    wit.scatter(c.inst, np.array([], dtype=np.int64), np.array([], dtype=np.int64))        # count = 0: nothing, no counter moved
    assert wit.scatter_info() == (calls, rows, terms)
    n_wit = msm_launches(lambda: c.check(wit, cur, b"count"))
    n_fresh = msm_launches(lambda: c.check(c.host_witness(cur), cur, b"count"))
    assert n_fresh - n_wit == (1 if kept else 0), (n_fresh, n_wit)


# ------------------------------------------------------------------------------------------------ 5. repeated patches
def test_repeated_patches_of_one_row(rng):
    c = case(10)
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    a, b = 3 * c.R + 4, 3 * c.R + 9
    idx = np.array([a, b], dtype=np.int64)
    for k in range(24):
        new = [cur[a] if k % 3 == 0 else values(rng, 1, "large")[0], (Q - 1) if k % 2 else 0]   # k % 3 == 0: a is written with what it holds (delta 0); b alternates 0, l - 1
        wit.scatter(c.inst, idx, bytes32(new))
        cur[a], cur[b] = new
    assert wit.scatter_info() == (24, 24, 48) and wit.rows_info()[3] == 0
    c.check(wit, cur, b"24 patches")
    wit.drop_rows()
    wit.keep_rows(c.inst, c.gens)
    c.check(wit, cur, b"kept again")


# ------------------------------------------------------------------------------------------------ 6. formats and sources
def test_formats_and_sources(rng):
    c = case(10)
    R, V = c.R, c.V
    cur = values(rng, V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    KD = oa.kernels_dev
    stream = KD.stream_create()
    try:
        idx, new = [2, R - 1, R, 5 * R + 7], [-5, -2 ** 63, 2 ** 63 - 1, 0]                  # host I64 with negatives and INT64_MIN
        wit.scatter(c.inst, np.array(idx, dtype=np.int64), np.array(new, dtype=np.int64))
        for j, x in zip(idx, new):
            cur[j] = x % Q
        c.check(wit, cur, b"host i64")
        idx = sorted(int(j) for j in rng.choice(V, size=70, replace=False))                   # device I64 on a caller's stream
        new = [int(x) for x in rng.integers(-2 ** 63, 2 ** 63 - 1, size=70, endpoint=True)]
        assert dev_scatter(wit, c.inst, idx, np.array(new, dtype=np.int64), I64, 0, stream) == 0
        for j, x in zip(idx, new):
            cur[j] = x % Q
        c.check(wit, cur, b"device i64")
        idx = sorted(int(j) for j in rng.choice(V, size=33, replace=False))                   # device Montgomery words on a caller's stream
        new = values(rng, 33)
        assert dev_scatter(wit, c.inst, idx, oa.fr_from_ints(new), M32, 0, stream) == 0
        for j, x in zip(idx, new):
            cur[j] = x
        c.check(wit, cur, b"device montgomery")
        idx, new = [V - 3, V - 1], values(rng, 2)                                           # host canonical bytes
        wit.scatter(c.inst, np.array(idx, dtype=np.uint64), bytes32(new))
        for j, x in zip(idx, new):
            cur[j] = x
        c.check(wit, cur, b"host canonical")
        idx = [7 * R + k for k in range(0, 10, 3)]                                           # a strided device source: every second integer
        pairs = [int(x) for x in rng.integers(-2 ** 40, 2 ** 40, size=2 * len(idx))]
        assert dev_scatter(wit, c.inst, idx, np.array(pairs, dtype=np.int64), I64, 16, None) == 0
        for j, x in zip(idx, pairs[::2]):
            cur[j] = x % Q
        c.check(wit, cur, b"strided device i64")
        assert wit.rows_info()[3] == 0
    finally:
        KD.stream_sync(stream)
        KD.stream_destroy(stream)


# ------------------------------------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("where", ["host", "device"])
def test_refusals_leave_everything_as_it_was(rng, where):
    c = case(10)
    V = c.V
    cur = values(rng, V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    wit.scatter(c.inst, np.array([3, 40], dtype=np.int64), bytes32([5, 6]))
    cur[3], cur[40] = 5, 6
    before = (wit.rows_info(), wit.scatter_info(), wit.info)
    l32 = np.frombuffer(Q.to_bytes(32, "little"), dtype=np.uint8)

    def call(idx, src, fmt):
        if where == "device":
            return dev_scatter(wit, c.inst, idx, src, fmt)
        ix = np.array(idx, dtype=np.uint64)
        return oa.lib.otti_witness_scatter(c.inst._h, wit._h, ix.ctypes.data_as(_vp), src.ctypes.data_as(_vp), len(idx), fmt, 0, 0, None)

    n = 300
    idx = sorted(int(j) for j in rng.choice(V, size=n, replace=False))
    for fmt in (C32, M32):
        for k in (0, n // 2, n - 1):                             # a scalar = l at the first, a middle and the last position
            src = np.ascontiguousarray(bytes32(values(rng, n)) if fmt == C32 else oa.fr_from_ints(values(rng, n))).copy()
            src[k] = l32
            assert call(idx, src, fmt) == INVALID_SCALAR, (fmt, k)
            assert (wit.rows_info(), wit.scatter_info(), wit.info) == before
    good = np.ascontiguousarray(bytes32(values(rng, 3)))
    both = good.copy(); both[1] = l32
    for bad in ([7, 7, 9], [9, 8, 10], [1, 2, V], [1, 2, 2 ** 63]):  # equal, descending, >= V
        assert call(bad, good, C32) == INVALID_INDEX, bad
        assert call(bad, both, C32) == INVALID_INDEX, bad        # both faults: the index list is named
        assert (wit.rows_info(), wit.scatter_info(), wit.info) == before
    c.check(wit, cur, b"after refusals")
    assert msm_launches(lambda: c.check(wit, cur, b"count")) + 1 == msm_launches(lambda: c.check(c.host_witness(cur), cur, b"count"))


# ------------------------------------------------------------------------------------------------ 8. interleaving
def test_scatter_between_range_updates(rng):
    c = case(10)
    R = c.R
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)

    def scatter(idx):
        new = values(rng, len(idx))
        wit.scatter(c.inst, np.array(idx, dtype=np.int64), bytes32(new))
        for j, x in zip(idx, new):
            cur[j] = x
    scatter([1, R + 2, 9 * R])
    new = values(rng, R + 3)
    wit.update(c.inst, R - 1, bytes32(new))                     # rows 0 .. 2
    cur[R - 1:2 * R + 2] = new
    scatter([0, R, 2 * R + 1, 31 * R + 31])
    assert wit.rows_info() == (True, c.L, c.R, 3)
    assert wit.scatter_info() == (2, 7, 7)
    c.check(wit, cur, b"interleaved")


# ------------------------------------------------------------------------------------------------ 9. small_fraction
@pytest.mark.parametrize("base", ["small", "large"])
def test_small_fraction_is_a_fresh_uploads(rng, base):
    c = case(10)
    cur = values(rng, c.V, base)
    wit = c.host_witness(cur)
    assert (wit.info[2] > 0.25) == (base == "small")
    wit.keep_rows(c.inst, c.gens)
    idx = sorted(int(j) for j in rng.choice(c.V, size=(7 * c.V) // 8, replace=False))
    new = values(rng, len(idx), "large" if base == "small" else "small")
    wit.scatter(c.inst, np.array(idx, dtype=np.int64), bytes32(new))
    for j, x in zip(idx, new):
        cur[j] = x
    assert (wit.info[2] > 0.25) == (base != "small")
    assert wit.info[2] == c.host_witness(cur).info[2]
    c.check(wit, cur, b"across the threshold")


# ------------------------------------------------------------------------------------------------ 10. SNARK
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


def test_scatter_serves_a_snark_proof(rng, snark):
    c = case(10)
    sg, comm, og, oc = snark
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, sg)
    idx = sorted(int(j) for j in rng.choice(c.V, size=50, replace=False))
    new = values(rng, 50)
    wit.scatter(c.inst, np.array(idx, dtype=np.int64), bytes32(new))
    for j, x in zip(idx, new):
        cur[j] = x
    assert wit.scatter_info() == (1, len({j // c.R for j in idx}), 50) and wit.rows_info()[3] == 0
    got = oa.SNARK.prove(c.inst, comm, wit, None, sg, b"snark scatter", SEED).bytes
    assert got == orc.snark_prove(c.oinst, oc, bytes32(cur), c.inputs32, og, b"snark scatter", SEED)[0]


# ------------------------------------------------------------------------------------------------ 11. set_inputs
def test_set_inputs(rng):
    c = case(10)
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    new_in = bytes32([Q - 1, 2 ** 130])
    before = (wit.rows_info(), wit.scatter_info(), wit.info)
    wit.set_inputs(c.inst, oa.InputsAssignment.new(new_in))
    assert (wit.rows_info(), wit.scatter_info(), wit.info) == before
    n_wit = msm_launches(lambda: c.check(wit, cur, b"new inputs", inputs32=new_in))
    fresh = oa.Witness(c.inst, oa.VarsAssignment.new(bytes32(cur)), oa.InputsAssignment.new(new_in))
    assert msm_launches(lambda: c.check(fresh, cur, b"new inputs", inputs32=new_in)) - n_wit == 1
    bad = new_in.copy(); bad[0] = np.frombuffer(Q.to_bytes(32, "little"), dtype=np.uint8)
    for arr, code in ((bytes32([1, 2, 3]), INVALID_NUM_INPUTS), (bad, INVALID_SCALAR)):
        with pytest.raises(oa.R1CSError) as e:
            wit.set_inputs(c.inst, arr)
        assert e.value.code == code
    c.check(wit, cur, b"after refused inputs", inputs32=new_in)


# ------------------------------------------------------------------------------------------------ 12. conveniences
def test_unsorted_numpy_indices_are_sorted_for_the_caller(rng):
    c = case(10)
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    idx = [int(j) for j in rng.permutation(c.V)[:40]]
    assert idx != sorted(idx)
    new = [int(x) for x in rng.integers(-2 ** 63, 2 ** 63 - 1, size=40, endpoint=True)]
    wit.scatter(c.inst, np.array(idx, dtype=np.int64), np.array(new, dtype=np.int64))
    for j, x in zip(idx, new):
        cur[j] = x % Q
    c.check(wit, cur, b"unsorted")
    with pytest.raises(ValueError):
        wit.scatter(c.inst, np.array([5, 9, 5], dtype=np.int64), np.array([1, 2, 3], dtype=np.int64))
    assert wit.scatter_info()[0] == 1


def test_torch_tensors_on_a_torch_stream_give_the_oracles_proof():
    r, idx, new = W.scatter_case()
    oinst = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    ogens = orc.OGens(r["num_cons"], r["num_vars"], r["num_inputs"])
    cur = [int(x) for x in W.start_values()]
    for j, x in zip(idx, new):
        cur[int(j)] = int(x)
    want = hashlib.sha256(orc.nizk_prove(oinst, bytes32(cur), r["inputs"], ogens, W.LABEL, W.SEED)[0]).hexdigest()
    res = subprocess.run([sys.executable, os.path.join(HERE, "witness_scatter_worker.py")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"the child ended with status {res.returncode}:\n{res.stdout}\n{res.stderr}"      # nothing further is started after a fault
    lines = res.stdout.split("\n")
    if any(ln.startswith("skip ") for ln in lines):
        pytest.skip(next(ln for ln in lines if ln.startswith("skip ")))
    got = dict(ln.split()[1:] for ln in lines if ln.startswith("digest "))
    assert set(got) == {"unsorted_int64"}, res.stdout + res.stderr
    assert got["unsorted_int64"] == want
