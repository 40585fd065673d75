"""Kept products through the witness: otti_witness_keep_products / _drop_products / _products_info, the four mutators that bring them up to date,
and their two consumers (the provers' copy instead of multiply_vec, check_sat's answer without a pass).

The judge of the kept vectors is otti_k_multiply_vec of the witness's own z, bit for bit, and the satisfiability pass on that z for count and bitmap;
the judge of every proof is the CPU oracle, byte for byte, beside a fresh upload of the same values.  Two instances: the synthetic 2^10 one (one entry
per row and matrix: the lane layout) and the compiler-like 2^12 one (the quad layout, coefficient codes, the heavy constant column and a long row)."""
import ctypes
import threading
import uuid

import numpy as np
import pytest

import otti_amd as oa
import orc
from witness_cases import Dev, Q, SEED, bytes32, z_of

pytestmark = pytest.mark.gpu
K, KD = oa.kernels, oa.kernels_dev
C32, M32, I64 = oa.WIT_CANONICAL32, oa.WIT_MONTGOMERY32, oa.WIT_I64
BAD_ARG, INVALID_INDEX, INVALID_SCALAR, INVALID_NUM_VARS = -21, -6, -5, -4
_vp = ctypes.c_void_p
L32 = np.frombuffer(Q.to_bytes(32, "little"), dtype=np.uint8)


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


class Inst:
    def __init__(self, kind, lg, ni=10, seed=1):
        self.r = r = (oa.synth_r1cs if kind == "uniform" else oa.synth_r1cs_compiler_like)(1 << lg, ni, seed)
        self.args = (r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
        self.inst, self.gens = oa.Instance.new(*self.args), oa.NIZKGens.new(*self.args[:3])
        self.oinst, self.ogens = orc.OInstance(*self.args), orc.OGens(*self.args[:3])
        self.N, self.V, self.ni = self.inst.dims
        self.vars = [int.from_bytes(r["vars"][i].tobytes(), "little") for i in range(r["vars"].shape[0])]
        self.vars += [0] * (self.V - len(self.vars))
        self.inputs32 = np.ascontiguousarray(r["inputs"])

    def touches(self, cols):
        """whether a column of z in `cols` holds an entry of A, B or C (num_vars is a power of two here: a caller's column is its index in z)"""
        assert self.r["num_vars"] == self.V
        return any(bool(np.isin(self.r[k]["col"].astype(np.int64), np.array(list(cols), dtype=np.int64)).any()) for k in "ABC")

    def witness(self, cur, inputs32=None):
        return oa.Witness(self.inst, oa.VarsAssignment.new(bytes32(cur)), oa.InputsAssignment.new(self.inputs32 if inputs32 is None else inputs32))

    def oracle(self, cur, label, inputs32=None):
        return orc.nizk_prove(self.oinst, bytes32(cur), self.inputs32 if inputs32 is None else inputs32, self.ogens, label, SEED)[0]

    def prove(self, wit, label):
        return oa.NIZK.prove(self.inst, wit, None, self.gens, label, SEED).bytes


_insts = {}


def inst_of(name):
    if name not in _insts:
        _insts[name] = Inst("uniform", 10) if name == "uniform10" else Inst("compiler", 12)
    return _insts[name]


def test_the_two_instances_take_the_two_layouts():
    u, c = inst_of("uniform10"), inst_of("compiler12")
    iu, ic, icc = u.inst.device_info(), c.inst.device_info(), c.inst.device_info(by_col=True)
    assert not iu["quad"] and iu["n_heavy"] == 0
    assert ic["quad"] and ic["use_small"] and ic["n_heavy"] >= 1 and icc["n_heavy"] >= 1, (ic, icc)


def kept(wit):
    """(Az, Bz, Cz downloaded from the witness's device pointers, the info dict)"""
    info = wit.products_info()
    out = []
    for key in ("d_Az", "d_Bz", "d_Cz"):
        a = np.zeros((info["n_rows"], 32), dtype=np.uint8)
        assert oa.lib.otti_dev_download(a.ctypes.data_as(_vp), _vp(info[key]), a.nbytes) == 0
        out.append(a)
    return out, info


def state(I, wit):
    """everything a refusal must leave alone: the three vectors, the bitmap (as check_sat lists it), the count and the counters, z and small_fraction"""
    abc, info = kept(wit)
    rep = wit.check_sat(I.inst, max_rows=I.N, values=False)
    z, sf = z_of(wit)
    return (b"".join(a.tobytes() for a in abc), rep.n_unsat, rep.rows.tolist(), tuple(sorted(info.items())), z.tobytes(), sf)


def assert_current(I, wit, what):
    """the kept vectors are otti_k_multiply_vec of the witness's z bit for bit; count and bitmap are the satisfiability pass's on that z"""
    z, _ = z_of(wit)
    want = K.multiply_vec(I.inst, z)[:3]
    got, info = kept(wit)
    assert info["kept"] and info["n_rows"] == I.N
    for k in range(3):
        bad = np.nonzero((got[k] != want[k]).any(axis=1))[0]
        assert not bad.size, "%s: kept %sz differs from multiply_vec in %d rows, first %s" % (what, "ABC"[k], bad.size, bad[:6].tolist())
    words = (I.N + 63) // 64
    bits = oa.DeviceArray(words, 8)
    n = KD.check_sat(I.inst, oa.DeviceArray.from_host(z), bits)
    want_bits = bits.to_host().reshape(-1).view(np.uint64)
    want_rows = [64 * w + b for w in range(words) for b in range(64) if (int(want_bits[w]) >> b) & 1]
    assert info["n_unsat"] == n == len(want_rows), (what, info["n_unsat"], n)
    rep = wit.check_sat(I.inst, max_rows=I.N, values=False)
    assert rep.n_unsat == n and rep.rows.tolist() == want_rows, (what, rep.n_unsat, rep.rows.tolist()[:8], want_rows[:8])
    return info


def small_values(rng, n):
    return [int(x) for x in rng.integers(1, 1 << 40, size=n)]


# ------------------------------------------------------------------------------------------------ 1. keep, then every mutator from host and device
@pytest.mark.parametrize("share", ["1", "0", None])
@pytest.mark.parametrize("name", ["uniform10", "compiler12"])
def test_products_follow_every_mutator(rng, monkeypatch, name, share):
    if share is None:
        monkeypatch.delenv("OTTI_PRODUCTS_FULL_SHARE", raising=False)
    else:
        monkeypatch.setenv("OTTI_PRODUCTS_FULL_SHARE", share)      # 1: always the patch; 0: always the full pass; None: the measured rule
    I = inst_of(name)
    cur = list(I.vars)
    plain = I.witness(cur)
    before = plain.check_sat(I.inst).n_unsat
    assert before == 0
    wit = I.witness(cur)
    assert wit.products_info() == dict(kept=False, n_rows=0, d_Az=None, d_Bz=None, d_Cz=None, n_unsat=0, patches=0, rows_recomputed=0, full_passes=0)
    wit.keep_products(I.inst)
    info = assert_current(I, wit, "keep")
    assert (info["n_unsat"], info["patches"], info["rows_recomputed"], info["full_passes"]) == (before, 0, 0, 1)
    wit.keep_products(I.inst)                                      # again for the same instance: nothing done
    assert wit.products_info() == info
    V = I.V
    steps = 0

    def moved(what, cols):
        nonlocal steps, info
        new = assert_current(I, wit, what)
        steps += 1
        touch = I.touches(cols)                                    # (a column without entries touches no row: then only the forced full pass counts)
        assert new["patches"] + new["full_passes"] == info["patches"] + info["full_passes"] + (1 if touch or share == "0" else 0), (what, info, new)
        if share == "1":
            assert new["full_passes"] == 1 and (new["rows_recomputed"] > info["rows_recomputed"]) == touch, (what, new)
        if share == "0":
            assert new["patches"] == 0 and new["rows_recomputed"] == 0, (what, new)
        info = new

    # update: a host range of canonical bytes, then a device range of int64
    new = small_values(rng, 70)
    wit.update(I.inst, 5, bytes32(new)); cur[5:75] = new
    moved("update, host", range(5, 75))
    new = small_values(rng, 9)
    d = Dev(np.array(new, dtype=np.int64))
    wit.update(I.inst, V - 9, (d.addr, 9), fmt=I64); cur[V - 9:] = new
    moved("update, device", range(V - 9, V))
    # scatter: host indices and values, then both in device memory
    idx = sorted(int(j) for j in rng.choice(V, size=40, replace=False)); new = small_values(rng, 40)
    wit.scatter(I.inst, np.array(idx, dtype=np.int64), bytes32(new))
    for j, x in zip(idx, new):
        cur[j] = x
    moved("scatter, host", idx)
    idx = [0, 63, 64, V - 1]; new = small_values(rng, 4)
    di, ds = Dev(np.array(idx, dtype=np.uint64)), Dev(np.array(new, dtype=np.int64))
    assert oa.lib.otti_witness_scatter(I.inst._h, wit._h, _vp(di.addr), _vp(ds.addr), 4, I64, 0, 1, None) == 0
    for j, x in zip(idx, new):
        cur[j] = x
    moved("scatter, device", idx)
    # assign: a whole vector of which a few elements moved, from the host and from the device; then one of which none moved
    for where in ("host", "device"):
        nxt = list(cur)
        idx = [int(j) for j in rng.choice(V, size=17, replace=False)]
        for j in idx:
            nxt[j] = (cur[j] + 1) % Q
        if where == "host":
            assert wit.assign(I.inst, bytes32(nxt)) == 17
        else:
            d = Dev(bytes32(nxt))
            assert wit.assign(I.inst, (d.addr, V), fmt=C32) == 17
        cur = nxt
        moved("assign, " + where, idx)
    assert wit.assign(I.inst, bytes32(cur)) == 0                  # nothing changed: no counter moves
    assert wit.products_info() == info
    # set_inputs: inputs are columns of z too
    new_in = bytes32(small_values(rng, I.ni))
    wit.set_inputs(I.inst, new_in)
    moved("set_inputs", range(V + 1, V + 1 + I.ni))
    # the state at the end serves a proof equal to a fresh upload's and to the oracle's
    want = I.oracle(cur, b"after the mutators", new_in)
    assert I.prove(wit, b"after the mutators") == want
    assert I.prove(I.witness(cur, new_in), b"after the mutators") == want
    assert wit.products_info() == info                            # proofs and checks only read


# ------------------------------------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("name", ["uniform10", "compiler12"])
def test_refusals_leave_everything_as_it_was(rng, name):
    I = inst_of(name)
    cur = list(I.vars)
    wit = I.witness(cur)
    wit.keep_products(I.inst)
    wit.scatter(I.inst, np.array([3, 40], dtype=np.int64), bytes32([5, 6]))      # a state with failing rows and moved counters
    cur[3], cur[40] = 5, 6
    before = state(I, wit)
    assert before[1] > 0
    V = I.V
    # a scalar >= l: update, scatter, assign
    src = bytes32(small_values(rng, 8)).copy(); src[5] = L32
    assert oa.lib.otti_witness_update(I.inst._h, wit._h, 10, src.ctypes.data_as(_vp), 8, C32, 0, 0, None) == INVALID_SCALAR
    assert state(I, wit) == before
    ix = np.arange(20, 28, dtype=np.uint64)
    assert oa.lib.otti_witness_scatter(I.inst._h, wit._h, ix.ctypes.data_as(_vp), src.ctypes.data_as(_vp), 8, C32, 0, 0, None) == INVALID_SCALAR
    assert state(I, wit) == before
    whole = bytes32(cur).copy(); whole[V // 2] = L32
    assert oa.lib.otti_witness_assign(I.inst._h, wit._h, 0, whole.ctypes.data_as(_vp), V, C32, 0, 0, None, None) == INVALID_SCALAR
    assert state(I, wit) == before
    # a bad device index list
    good = np.array(small_values(rng, 3), dtype=np.int64)
    for bad in ([7, 7, 9], [9, 8, 10], [1, 2, V]):
        di, ds = Dev(np.array(bad, dtype=np.uint64)), Dev(good)
        assert oa.lib.otti_witness_scatter(I.inst._h, wit._h, _vp(di.addr), _vp(ds.addr), 3, I64, 0, 1, None) == INVALID_INDEX, bad
        assert state(I, wit) == before
    # a witness of other dimensions, and an instance of other dimensions
    other = inst_of("compiler12" if name == "uniform10" else "uniform10")
    small = other.witness(other.vars)
    assert oa.lib.otti_witness_keep_products(I.inst._h, small._h) == INVALID_NUM_VARS
    assert small.products_info()["kept"] is False
    assert oa.lib.otti_witness_keep_products(other.inst._h, wit._h) == INVALID_NUM_VARS
    ok = bytes32(small_values(rng, 8))
    assert oa.lib.otti_witness_update(other.inst._h, wit._h, 10, ok.ctypes.data_as(_vp), 8, C32, 0, 0, None) == INVALID_NUM_VARS
    assert state(I, wit) == before
    # another instance of the same dimensions: every mutator refuses, and a check or proof with it computes as without kept products
    twin = Inst("uniform" if name == "uniform10" else "compiler", 10 if name == "uniform10" else 12, seed=2)
    assert twin.inst.dims == I.inst.dims
    assert oa.lib.otti_witness_update(twin.inst._h, wit._h, 10, ok.ctypes.data_as(_vp), 8, C32, 0, 0, None) == BAD_ARG
    assert oa.lib.otti_witness_scatter(twin.inst._h, wit._h, ix.ctypes.data_as(_vp), ok.ctypes.data_as(_vp), 8, C32, 0, 0, None) == BAD_ARG
    assert oa.lib.otti_witness_assign(twin.inst._h, wit._h, 0, bytes32(cur).ctypes.data_as(_vp), V, C32, 0, 0, None, None) == BAD_ARG
    assert oa.lib.otti_witness_set_inputs(twin.inst._h, wit._h, I.inputs32.ctypes.data_as(_vp), I.ni) == BAD_ARG
    assert state(I, wit) == before
    rep_twin, rep_plain = wit.check_sat(twin.inst, max_rows=64), twin.witness(cur, I.inputs32).check_sat(twin.inst, max_rows=64)
    assert (rep_twin.n_unsat, rep_twin.rows.tolist()) == (rep_plain.n_unsat, rep_plain.rows.tolist()) and np.array_equal(rep_twin.values, rep_plain.values)
    assert twin.prove(wit, b"twin") == orc.nizk_prove(twin.oinst, bytes32(cur), I.inputs32, twin.ogens, b"twin", SEED)[0]
    assert state(I, wit) == before
    assert I.prove(wit, b"after refusals") == I.oracle(cur, b"after refusals")


# ------------------------------------------------------------------------------------------------ 3. proof bytes
@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("name", ["uniform10", "compiler12"])
def test_nizk_proofs_are_the_oracles(rng, name, rows):
    I = inst_of(name)
    cur = list(I.vars)
    wit = I.witness(cur)
    wit.keep_products(I.inst)
    if rows:
        wit.keep_rows(I.inst, I.gens)
    assert I.prove(wit, b"kept") == I.oracle(cur, b"kept")
    idx = sorted(int(j) for j in rng.choice(I.V, size=64, replace=False)); new = small_values(rng, 64)
    wit.scatter(I.inst, np.array(idx, dtype=np.int64), np.array(new, dtype=np.int64))
    for j, x in zip(idx, new):
        cur[j] = x
    want = I.oracle(cur, b"after a scatter")
    assert I.prove(wit, b"after a scatter") == want and I.prove(I.witness(cur), b"after a scatter") == want
    new_in = bytes32(small_values(rng, I.ni))
    wit.set_inputs(I.inst, new_in)
    want = I.oracle(cur, b"after set_inputs", new_in)
    assert I.prove(wit, b"after set_inputs") == want and I.prove(I.witness(cur, new_in), b"after set_inputs") == want
    # a world of one proves unsharded: the same bytes
    oa.shard_init("otti-test-" + uuid.uuid4().hex, 0, 1)
    try:
        assert oa.NIZK.prove_sharded(I.inst, wit, I.gens, b"after set_inputs", SEED).bytes == want
    finally:
        oa.shard_finalize()
    assert_current(I, wit, "after the proofs")


@pytest.mark.parametrize("rows", [False, True])
def test_snark_proofs_are_the_oracles(rng, rows):
    I = inst_of("uniform10")
    nz = max(len(I.r[k]) for k in "ABC")
    sg, og = oa.SNARKGens.new(*I.args[:3], nz), orc.OSnarkGens(*I.args[:3], nz)
    comm, oc = oa.ComputationCommitment.encode(I.inst, sg), orc.OSnarkComm.encode(I.oinst, og)
    assert comm.bytes == oc.bytes
    cur = list(I.vars)
    wit = I.witness(cur)
    wit.keep_products(I.inst)
    if rows:
        wit.keep_rows(I.inst, sg)
    idx = sorted(int(j) for j in rng.choice(I.V, size=30, replace=False)); new = small_values(rng, 30)
    wit.scatter(I.inst, np.array(idx, dtype=np.int64), np.array(new, dtype=np.int64))
    for j, x in zip(idx, new):
        cur[j] = x
    want = orc.snark_prove(I.oinst, oc, bytes32(cur), I.inputs32, og, b"snark, scatter", SEED)[0]
    assert oa.SNARK.prove(I.inst, comm, wit, None, sg, b"snark, scatter", SEED).bytes == want
    assert oa.SNARK.prove(I.inst, comm, I.witness(cur), None, sg, b"snark, scatter", SEED).bytes == want
    new_in = bytes32(small_values(rng, I.ni))
    wit.set_inputs(I.inst, new_in)
    want = orc.snark_prove(I.oinst, oc, bytes32(cur), new_in, og, b"snark, inputs", SEED)[0]
    assert oa.SNARK.prove(I.inst, comm, wit, None, sg, b"snark, inputs", SEED).bytes == want
    assert oa.SNARK.prove(I.inst, comm, I.witness(cur, new_in), None, sg, b"snark, inputs", SEED).bytes == want


# ------------------------------------------------------------------------------------------------ 4. the passes are really skipped
def _launches(fn):
    oa.stats_enable(True)
    try:
        fn()
        s = oa.stats_read()
    finally:
        oa.stats_enable(False)
    return {k: v[0] for k, v in s.items()}


@pytest.mark.parametrize("name", ["uniform10", "compiler12"])
def test_the_passes_are_skipped(name):
    I = inst_of(name)
    cur = list(I.vars)
    plain, wit = I.witness(cur), I.witness(cur)
    wit.keep_products(I.inst)
    z, _ = z_of(plain)
    one_multiply_vec = _launches(lambda: K.multiply_vec(I.inst, z))["spmv"]
    assert one_multiply_vec >= 1
    n_plain = _launches(lambda: I.prove(plain, b"count"))
    n_kept = _launches(lambda: I.prove(wit, b"count"))
    print(name, "spmv launches: one multiply_vec", one_multiply_vec, "proof from a plain witness", n_plain["spmv"], "from a keeping one", n_kept["spmv"])
    assert n_plain["spmv"] - n_kept["spmv"] == one_multiply_vec
    c_plain = _launches(lambda: plain.check_sat(I.inst))
    c_kept = _launches(lambda: wit.check_sat(I.inst))
    assert c_plain["sat_check"] >= 1 and c_kept["sat_check"] == 0 and c_kept["spmv"] == 0
    assert wit.check_sat(I.inst).kernel_ms == 0                   # satisfied: nothing launched


# ------------------------------------------------------------------------------------------------ 5. an unsatisfied assignment, and its repair
@pytest.mark.parametrize("name", ["uniform10", "compiler12"])
def test_check_sat_reports_as_a_plain_witness_does(rng, name):
    I = inst_of(name)
    cur = list(I.vars)
    broken = sorted(int(j) for j in rng.choice(I.V, size=9, replace=False))
    good = [cur[j] for j in broken]
    for j in broken:
        cur[j] = cur[j] + 7
    plain, wit = I.witness(cur), I.witness(cur)
    wit.keep_products(I.inst)
    for max_rows in (4, 64, I.N):
        a, b = plain.check_sat(I.inst, max_rows=max_rows), wit.check_sat(I.inst, max_rows=max_rows)
        assert a.n_unsat == b.n_unsat > 0 and a.rows.tolist() == b.rows.tolist() and np.array_equal(a.values, b.values), (name, max_rows)
    assert wit.check_sat(I.inst).kernel_ms > 0                     # the report kernel ran for the failing rows
    assert wit.products_info()["n_unsat"] == plain.check_sat(I.inst).n_unsat
    wit.scatter(I.inst, np.array(broken, dtype=np.int64), bytes32(good))
    assert wit.products_info()["n_unsat"] == 0 and bool(wit.check_sat(I.inst))
    assert_current(I, wit, "repaired")


# ------------------------------------------------------------------------------------------------ 6. threads
def test_two_threads_prove_from_one_keeping_witness():
    I = inst_of("compiler12")
    wit = I.witness(I.vars)
    wit.keep_products(I.inst)
    wit.keep_rows(I.inst, I.gens)
    want = I.prove(wit, b"threads")
    assert want == I.oracle(I.vars, b"threads")
    out, errs = {}, []

    def work(k):
        try:
            out[k] = [I.prove(wit, b"threads") for _ in range(3)] + [wit.check_sat(I.inst).n_unsat]
        except Exception as e:                                     # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert all(out[k] == [want] * 3 + [0] for k in range(2))


# ------------------------------------------------------------------------------------------------ 7. drop
def test_after_drop_the_witness_is_a_plain_one(rng):
    I = inst_of("compiler12")
    cur = list(I.vars)
    wit = I.witness(cur)
    wit.drop_products()                                            # none kept: fine
    wit.keep_products(I.inst)
    wit.drop_products()
    assert wit.products_info() == dict(kept=False, n_rows=0, d_Az=None, d_Bz=None, d_Cz=None, n_unsat=0, patches=0, rows_recomputed=0, full_passes=0)
    idx = [1, 2, 100]; new = small_values(rng, 3)
    wit.scatter(I.inst, np.array(idx, dtype=np.int64), np.array(new, dtype=np.int64))
    for j, x in zip(idx, new):
        cur[j] = x
    assert wit.products_info()["patches"] == 0
    plain = I.witness(cur)
    a, b = plain.check_sat(I.inst), wit.check_sat(I.inst)
    assert a.n_unsat == b.n_unsat and a.rows.tolist() == b.rows.tolist() and np.array_equal(a.values, b.values) and b.kernel_ms > 0
    n_plain, n_wit = _launches(lambda: I.prove(plain, b"dropped")), _launches(lambda: I.prove(wit, b"dropped"))
    assert n_plain == n_wit
    assert _launches(lambda: wit.check_sat(I.inst))["sat_check"] >= 1
    assert I.prove(wit, b"dropped") == I.oracle(cur, b"dropped")
    wit.keep_products(I.inst)                                      # and kept again: one full pass, current
    info = assert_current(I, wit, "kept again")
    assert (info["patches"], info["full_passes"]) == (0, 1)
