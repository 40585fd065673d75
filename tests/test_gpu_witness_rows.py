"""A resident witness that keeps the unblinded row sums of its commitment (otti_witness_keep_rows[_snark], otti_witness_drop_rows,
otti_witness_rows_info): proofs read them instead of summing the witness again, otti_witness_update sums only the rows it touches.

The judge of every proof is the CPU oracle (orc.nizk_prove / orc.snark_prove) for the same instance, assignment, inputs, label and seed, byte
for byte; the assignment the oracle gets is kept in Python integers, never read back from the code under test.  That kept rows are USED is read
off the library's launch counters (otti_stats_*): a proof from kept rows makes exactly one fixed-base MSM launch fewer.

The circuit is satisfied by EVERY assignment (row i: (k_i * v_i) * 1 = k_i * v_i), so any update leaves a witness both provers accept, while
Az and Cz still depend on every variable.  Sizes: 2^5 (L = 4, R = 8: odd ell), 2^10 (L = R = 32), 2^12 (L = R = 64)."""
import ctypes
import threading

import numpy as np
import pytest

import otti_amd as oa
import orc
from witness_cases import Case, Dev, Q, SEED, bytes32, case, msm_launches, values

pytestmark = pytest.mark.gpu
C32, M32, I64 = oa.WIT_CANONICAL32, oa.WIT_MONTGOMERY32, oa.WIT_I64
INVALID_SCALAR = -5
_vp = ctypes.c_void_p


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(autouse=True)
def _pinned_window(monkeypatch):
    monkeypatch.setenv("OTTI_MSM_WINDOW", "9")                 # a narrow table, whose width does not depend on what else ran in this process


def touched(first, count, R):
    return 0 if not count else (first + count - 1) // R - first // R + 1


# ------------------------------------------------------------------------------------------------ 1. reuse
@pytest.mark.parametrize("ell", [5, 10, 12])
def test_kept_rows_are_reused_and_save_the_commitment_launch(rng, ell):
    c = case(ell)
    cur = values(rng, c.V)
    wit, plain = c.host_witness(cur), c.host_witness(cur)
    assert wit.rows_info() == (False, 0, 0, 0)
    wit.keep_rows(c.inst, c.gens)
    assert wit.rows_info() == (True, c.L, c.R, 0)
    wit.keep_rows(c.inst, c.gens)                               # again: nothing
    assert wit.rows_info() == (True, c.L, c.R, 0)
    for k in range(3):
        c.check(wit, cur, b"reuse %d" % k, bytes([k + 1]) * 32)
    n_kept = msm_launches(lambda: c.check(wit, cur, b"count"))
    n_plain = msm_launches(lambda: c.check(plain, cur, b"count"))
    assert n_plain - n_kept == 1, (n_plain, n_kept)
    assert wit.rows_info() == (True, c.L, c.R, 0)
    other = case(10 if ell != 10 else 12)
    with pytest.raises(oa.SpartanError) as e:                   # generators of another size
        wit.keep_rows(c.inst, other.gens)
    assert e.value.code == -21


# ------------------------------------------------------------------------------------------------ 2. update geometry
def _ranges(c):
    V, L, R = c.V, c.L, c.R
    out = [("inside one row", [(R + 1, min(3, R - 2))]), ("across one row boundary", [(R - 1, 2)]), ("exactly one whole row", [(2 * R, R)])]
    if L >= 8:
        out.append(("a run of four rows", [(5 * R - 3, 2 * R + 6)]))
        out.append(("three whole rows", [(R, 3 * R)]))
    out += [("the last variable", [(V - 1, 1)]), ("the whole vector", [(0, V)]), ("count = 0", [(7, 0)]),
            ("two disjoint updates", [(1, 2), (V - R - 1, 3)])]
    return out


@pytest.mark.parametrize("ell", [5, 10, 12])
def test_update_resums_exactly_the_rows_it_touches(rng, ell):
    c = case(ell)
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    done = 0
    for name, ranges in _ranges(c):
        for first, count in ranges:
            new = values(rng, count)
            wit.update(c.inst, first, bytes32(new).reshape(-1, 32))
            cur[first:first + count] = new
            done += touched(first, count, c.R)
            assert wit.rows_info() == (True, c.L, c.R, done), name
        c.check(wit, cur, name.encode())
    assert touched(5 * c.R - 3, 2 * c.R + 6, c.R) == 4 and touched(c.R - 1, 2, c.R) == 2 and touched(2 * c.R, c.R, c.R) == 1
    wit.keep_rows(c.inst, c.gens)                               # the same points: nothing is summed, the count goes on
    assert wit.rows_info()[3] == done


# ------------------------------------------------------------------------------------------------ 3. formats and sources
@pytest.mark.parametrize("source", ["from_ints", "from_device_i64", "from_device_montgomery32"])
def test_other_witness_formats_and_update_sources(rng, source):
    c = case(10)
    V, R = c.V, c.R
    KD = oa.kernels_dev
    if source == "from_device_montgomery32":
        cur = values(rng, V)
        d = Dev(oa.fr_from_ints(cur))
        wit = oa.Witness.from_device(c.inst, d.addr, V, M32, c.inputs)
    else:
        ints = [int(x) for x in rng.integers(-2 ** 63, 2 ** 63 - 1, size=V, endpoint=True)]
        ints[:4] = [-1, -2 ** 63, 2 ** 63 - 1, 0]
        cur = [x % Q for x in ints]
        a = np.array(ints, dtype=np.int64)
        if source == "from_ints":
            wit = oa.Witness.from_ints(c.inst, a, c.inputs)
        else:
            d = Dev(a)
            wit = oa.Witness.from_device(c.inst, d.addr, V, I64, c.inputs)
    wit.keep_rows(c.inst, c.gens)
    c.check(wit, cur, b"as made")
    done = 0
    stream = KD.stream_create()
    try:
        # host integers (negative ones among them) across a row boundary; device integers and device Montgomery words on a caller's stream
        new = [-5, 7, -2 ** 63, 9]
        wit.update(c.inst, R - 2, np.array(new, dtype=np.int64))
        cur[R - 2:R + 2] = [x % Q for x in new]
        done += 2
        new = [int(x) for x in rng.integers(-2 ** 63, 2 ** 63 - 1, size=3 * R + 1, endpoint=True)]
        d1 = Dev(np.array(new, dtype=np.int64))
        wit.update(c.inst, 4 * R, (d1.addr, len(new)), fmt=I64, stream=stream)
        cur[4 * R:7 * R + 1] = [x % Q for x in new]
        done += 4
        new = values(rng, R)
        d2 = Dev(oa.fr_from_ints(new))
        wit.update(c.inst, V - R, (d2.addr, R), fmt=M32, stream=stream)
        cur[V - R:] = new
        done += 1
        new = values(rng, 5)
        wit.update(c.inst, 10 * R + 3, bytes32(new))            # canonical bytes from the host
        cur[10 * R + 3:10 * R + 8] = new
        done += 1
        assert wit.rows_info() == (True, c.L, c.R, done)
        c.check(wit, cur, b"updated")
    finally:
        KD.stream_sync(stream)
        KD.stream_destroy(stream)


# ------------------------------------------------------------------------------------------------ 4. failed update
@pytest.mark.parametrize("where", ["host", "device"])
def test_failed_update_leaves_rows_valid(rng, where):
    c = case(10)
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    wit.update(c.inst, 3, bytes32([5, 6]))
    cur[3:5] = [5, 6]
    before = wit.rows_info()
    assert before == (True, c.L, c.R, 1)
    for fmt, first, count, k in ((C32, c.R - 1, 2 * c.R, c.R), (M32, 0, c.V, c.V - 1), (C32, 7, 1, 0)):
        src = bytes32(values(rng, count)) if fmt == C32 else oa.fr_from_ints(values(rng, count))
        src = np.ascontiguousarray(src).copy()
        src[k] = np.frombuffer(Q.to_bytes(32, "little"), dtype=np.uint8)
        with pytest.raises(oa.R1CSError) as e:
            if where == "host":
                wit.update(c.inst, first, src, fmt=fmt)
            else:
                d = Dev(src)
                wit.update(c.inst, first, (d.addr, count), fmt=fmt)
        assert e.value.code == INVALID_SCALAR
        assert wit.rows_info() == before
    c.check(wit, cur, b"after refused updates")
    assert msm_launches(lambda: c.check(wit, cur, b"count")) + 1 == msm_launches(lambda: c.check(c.host_witness(cur), cur, b"count"))


# ------------------------------------------------------------------------------------------------ 5. both modes
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


def _snark_proof(c, snark, wit, label):
    sg, comm, _, _ = snark
    return oa.SNARK.prove(c.inst, comm, wit, None, sg, label, SEED).bytes


def test_rows_kept_with_nizk_generators_serve_a_snark_proof(rng, snark):
    c = case(10)
    _, _, og, oc = snark
    cur = values(rng, c.V)
    wit, plain = c.host_witness(cur), c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    want = orc.snark_prove(c.oinst, oc, bytes32(cur), c.inputs32, og, b"snark from nizk rows", SEED)[0]
    got = {}
    n_kept = msm_launches(lambda: got.__setitem__("kept", _snark_proof(c, snark, wit, b"snark from nizk rows")))
    n_plain = msm_launches(lambda: got.__setitem__("plain", _snark_proof(c, snark, plain, b"snark from nizk rows")))
    assert got["kept"] == want and got["plain"] == want
    assert n_plain - n_kept == 1, (n_plain, n_kept)
    new = values(rng, 3 * c.R)                                   # an update, then the SNARK prover again
    wit.update(c.inst, c.R // 2, bytes32(new))
    cur[c.R // 2:c.R // 2 + 3 * c.R] = new
    assert wit.rows_info()[3] == 4
    assert _snark_proof(c, snark, wit, b"updated") == orc.snark_prove(c.oinst, oc, bytes32(cur), c.inputs32, og, b"updated", SEED)[0]


def test_rows_kept_with_snark_generators_serve_a_nizk_proof(rng, snark):
    c = case(10)
    sg = snark[0]
    cur = values(rng, c.V)
    wit, plain = c.host_witness(cur), c.host_witness(cur)
    wit.keep_rows(c.inst, sg)
    assert wit.rows_info() == (True, c.L, c.R, 0)
    n_kept = msm_launches(lambda: c.check(wit, cur, b"nizk from snark rows"))
    n_plain = msm_launches(lambda: c.check(plain, cur, b"nizk from snark rows"))
    assert n_plain - n_kept == 1, (n_plain, n_kept)
    wit.keep_rows(c.inst, c.gens)                               # the same points under the other handle: nothing to do
    assert wit.rows_info() == (True, c.L, c.R, 0)


# ------------------------------------------------------------------------------------------------ 6. table rebuilt
def test_rows_outlive_the_window_table(rng, monkeypatch):
    c = Case(10)                                                # generators of its own: their table is released below
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    assert c.gens.table_info[0] == 9
    c.gens.release_device()
    assert c.gens.table_info == (0, 0)
    monkeypatch.setenv("OTTI_MSM_WINDOW", "8")                   # rebuilt with another window: the same points
    n_kept = msm_launches(lambda: c.check(wit, cur, b"rebuilt"))
    assert c.gens.table_info[0] == 8
    assert wit.rows_info() == (True, c.L, c.R, 0)
    assert msm_launches(lambda: c.check(c.host_witness(cur), cur, b"rebuilt")) - n_kept == 1
    c.gens.release_device()                                     # an update rebuilds the table it needs
    wit.update(c.inst, 0, bytes32([9]))
    cur[0] = 9
    assert wit.rows_info()[3] == 1
    c.check(wit, cur, b"updated after a release")


# ------------------------------------------------------------------------------------------------ 7. drop
def test_drop_rows(rng):
    c = case(10)
    cur = values(rng, c.V)
    wit, plain = c.host_witness(cur), c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    wit.drop_rows()
    assert wit.rows_info() == (False, 0, 0, 0)
    n_dropped = msm_launches(lambda: c.check(wit, cur, b"dropped"))
    assert n_dropped == msm_launches(lambda: c.check(plain, cur, b"dropped"))
    wit.update(c.inst, 5, bytes32([1, 2, 3]))
    cur[5:8] = [1, 2, 3]
    assert wit.rows_info() == (False, 0, 0, 0)
    c.check(wit, cur, b"dropped and updated")
    wit.drop_rows()                                             # none kept: fine
    wit.keep_rows(c.inst, c.gens)                               # and kept again, for the assignment as it is now
    assert wit.rows_info() == (True, c.L, c.R, 0)
    c.check(wit, cur, b"kept again")


# ------------------------------------------------------------------------------------------------ 8. two threads
def test_two_threads_prove_from_one_witness_with_kept_rows(rng):
    c = case(10)
    cur = values(rng, c.V)
    wit = c.host_witness(cur)
    wit.keep_rows(c.inst, c.gens)
    labels = [b"thread zero", b"thread one"]
    want = [c.want(cur, lb) for lb in labels]
    got, errs = [None, None], []

    def run(k):
        try:
            got[k] = oa.NIZK.prove(c.inst, wit, None, c.gens, labels[k], SEED).bytes
        except Exception as e:                                  # noqa: BLE001 — reported by the assertion below
            errs.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert got == want


# ------------------------------------------------------------------------------------------------ 9. values at the edges
@pytest.mark.parametrize("base", ["small", "large"])
def test_edge_values_in_resummed_rows(rng, base):
    """l - 1, 0, 2^128 - 1 and 2^128 (the boundary of small_fraction, which picks the bulk kernel's variant): written over one row (the
    latency-bound launch) and over a run of three (the bulk launch; `small` starts above the sparse threshold, `large` below it)"""
    c = case(12)
    cur = values(rng, c.V, base)
    wit = c.host_witness(cur)
    sf = wit.info[2]
    assert (sf > 0.25) == (base == "small"), sf
    wit.keep_rows(c.inst, c.gens)
    R, done = c.R, 0
    for k, fill in enumerate(([Q - 1] * R, [0] * R, [2 ** 128 - 1, 2 ** 128] * (R // 2))):
        wit.update(c.inst, (2 + k) * R, bytes32(fill))          # one row
        cur[(2 + k) * R:(3 + k) * R] = fill
        wit.update(c.inst, (10 + 4 * k) * R, bytes32(fill * 3))  # three rows
        cur[(10 + 4 * k) * R:(13 + 4 * k) * R] = fill * 3
        done += 4
    assert wit.rows_info() == (True, c.L, c.R, done)
    c.check(wit, cur, b"edges")
    big = [Q - 1] * c.V if base == "small" else [0] * c.V       # the whole vector across the threshold
    wit.update(c.inst, 0, bytes32(big))
    assert (wit.info[2] > 0.25) == (base != "small")
    c.check(wit, big, b"edges, whole vector")
