"""A resident witness filled from host bytes, from device memory, from host integers, and updated in place (otti_witness_upload,
otti_witness_from_device, otti_witness_upload_ints, otti_witness_update, otti_witness_info).

The reference for z is Python integers: z[:V + 1 + ni] is `oa.fr_from_ints` (pure Python, x * R mod l) of the values padded with zeros, then 1,
then the inputs; the rest of z is zero; small_fraction is sum(x % l < 2^128 over the padded values) / V, compared with == (both sides are one
correctly rounded division of integers below 2^53).  Every source is judged against that, the host upload included: it shares the ingest kernel
with the other sources, so it is no independent reference.  The comparison with a host upload of the same values stays as a second check (the
promise of the C ABI is "bit for bit what otti_witness_upload builds").  Whole proofs are compared with the CPU oracle's.  Bit-exact throughout:
the arithmetic is in GF(l)."""
import ctypes

import numpy as np
import pytest

import otti_amd as oa
import orc
from witness_cases import Dev, bytes32, z_of
from witness_tensor_worker import int_r1cs

pytestmark = pytest.mark.gpu
L = orc.L_ORDER
R = (1 << 256) % L
C32, M32, I64, U64 = oa.WIT_CANONICAL32, oa.WIT_MONTGOMERY32, oa.WIT_I64, oa.WIT_U64
FORMATS = {"canonical32": C32, "montgomery32": M32, "i64": I64, "u64": U64}
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63
INVALID_SCALAR, INVALID_NUM_VARS = -5, -4
V = 256
SENTINEL = 0x5e5e5e5e
_vp = ctypes.c_void_p


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(autouse=True)
def _pinned_window(monkeypatch):
    monkeypatch.setenv("OTTI_MSM_WINDOW", "9")                 # the window table's width does not depend on what else ran in this process


# ------------------------------------------------------------------------------------------------ helpers
def from_dev(inst, a, n, fmt, inputs, offset=0, **kw):
    d = Dev(a)                                                 # alive until the call has returned: the ingest has finished by then
    return oa.Witness.from_device(inst, d.addr + offset, n, fmt, inputs, **kw)


def update_dev(wit, inst, first, a, count, fmt, offset=0, **kw):
    d = Dev(a)
    wit.update(inst, first, (d.addr + offset, count), fmt=fmt, **kw)


def bare_instance(nv, ni=2):
    """an instance of nv variables with two one-entry constraints: enough to hold a witness (z does not depend on the matrices)"""
    e = np.zeros(2, dtype=oa.ENTRY_DTYPE)
    e["row"] = [0, 1]; e["col"] = [0, nv]; e["val"] = bytes32([1, 1])
    return oa.Instance.new(2, nv, ni, e, e, e), oa.InputsAssignment.new(bytes32([11, L - 3][:ni]))


def host_witness(inst, inputs, ints):
    return oa.Witness(inst, oa.VarsAssignment.new(bytes32(ints)), inputs)


def source(fmt, ints):
    """the values as the bytes of format fmt"""
    if fmt == C32:
        return bytes32(ints)
    if fmt == M32:
        return oa.fr_from_ints([int(x) % L for x in ints])
    return np.array([int(x) for x in ints], dtype=np.int64 if fmt == I64 else np.uint64)


def ints_of(a):
    """the integers of (n, 32) canonical little-endian bytes"""
    return [int.from_bytes(bytes(row), "little") for row in a]


def values_for(fmt, n, rng):
    """n values format fmt can carry: 32-byte ones mix widths around 2^128 (the small_fraction rule) and the ends of the range"""
    if fmt in (C32, M32):
        out = [int.from_bytes(rng.bytes(40), "little") % L >> int(s) for s in rng.choice([0, 100, 124, 125, 200], size=n)]
        out[:6] = [0, 1, 2 ** 128 - 1, 2 ** 128, L - 1, 2 ** 64][:n]
    elif fmt == I64:
        out = [int(x) for x in rng.integers(I64_MIN, I64_MAX, size=n, endpoint=True)]
        out[:5] = [0, 1, -1, I64_MAX, I64_MIN][:n]
    else:
        out = [int(x) for x in rng.integers(0, 2 ** 64 - 1, size=n, dtype=np.uint64, endpoint=True)]
        out[:4] = [0, 1, 2 ** 63, 2 ** 64 - 1][:n]
    return out


INPUTS = [11, L - 3]                                           # bare_instance's


def assert_z(wit, ints, what, nv=V, inputs=INPUTS):
    """z and small_fraction of wit against Python integers: the variables `ints`, padded with zeros to nv"""
    z, sf = z_of(wit)
    padded = [int(x) % L for x in ints] + [0] * (nv - len(ints))
    head = padded + [1] + [int(x) % L for x in inputs]
    assert z.shape == (2 * nv, 32), what
    assert np.array_equal(z[:len(head)], oa.fr_from_ints(head)), what
    assert not z[len(head):].any(), what
    want = sum(x < 2 ** 128 for x in padded) / nv
    print(f"{what}: small_fraction {sf} (Python integers {want})")
    assert sf == want, what


def assert_same(wit, ref, what, ints=None, **kw):
    """the Python integers first (ints=None: the caller anchors z itself), then a host upload of the same values as a second check"""
    if ints is not None:
        assert_z(wit, ints, what, **kw)
    (z, sf), (zr, sfr) = z_of(wit), z_of(ref)
    print(f"{what}: small_fraction {sf} (host upload {sfr})")
    assert z.shape == zr.shape and np.array_equal(z, zr), what
    assert sf == sfr, what


@pytest.fixture(scope="module")
def small():
    return bare_instance(V)


# ------------------------------------------------------------------------------------------------ the host upload, a source like the others
NVARS = (0, 1, 63, 64, 65, 255, V - 1, V)


def test_host_upload_is_the_python_integers(small, rng):
    inst, inputs = small
    for nvars in NVARS:
        ints = values_for(C32, nvars, rng)
        assert_z(host_witness(inst, inputs, ints), ints, f"host upload nvars={nvars}")


def test_host_upload_refuses_scalars_not_below_l(small, rng):
    inst, inputs = small
    ip = np.ascontiguousarray(inputs.assignment)
    for nvars, k in ((V, 0), (V, V - 1), (65, 64)):
        ints = values_for(C32, nvars, rng)
        for raw, ok in ((L, False), (L + 1, False), (2 ** 256 - 1, False), (L - 1, True)):
            src = bytes32(ints)
            src[k] = np.frombuffer(raw.to_bytes(32, "little"), dtype=np.uint8)
            out = _vp(SENTINEL)
            rc = oa.lib.otti_witness_upload(inst._h, src.ctypes.data_as(_vp), nvars, ip.ctypes.data_as(_vp), ip.shape[0], ctypes.byref(out))
            if not ok:
                assert rc == INVALID_SCALAR and out.value == SENTINEL, (nvars, k, hex(raw), rc)
                continue
            assert rc == 0 and out.value != SENTINEL, (nvars, k, rc)
            wit = oa.Witness._adopt(out)
            assert np.array_equal(z_of(wit)[0][k], np.frombuffer((raw * R % L).to_bytes(32, "little"), dtype=np.uint8))
            assert_z(wit, ints[:k] + [raw] + ints[k + 1:], f"host upload of l - 1 at {k} of {nvars}")


# ------------------------------------------------------------------------------------------------ same z as the Python integers and as a host upload
@pytest.mark.parametrize("name", list(FORMATS))
def test_same_z_as_host_upload(small, rng, name):
    inst, inputs = small
    fmt = FORMATS[name]
    for nvars in NVARS:
        ints = values_for(fmt, nvars, rng)
        src = source(fmt, ints)
        ref = host_witness(inst, inputs, ints)
        assert_z(ref, ints, f"{name} nvars={nvars} host upload")
        d = Dev(src)
        assert_same(oa.Witness.from_device(inst, d.addr, nvars, fmt, inputs), ref, f"{name} nvars={nvars} from_device", ints)
        if fmt in (I64, U64):
            assert_same(oa.Witness.from_ints(inst, src, inputs), ref, f"{name} nvars={nvars} from_ints", ints)


def test_grid_stride_loop_at_2p20(rng):
    n = 1 << 20                                                # above kMaxBlocks * kBlock = 524,288 elements: every lane takes a second element
    inst, inputs = bare_instance(n)
    x = rng.integers(0, I64_MAX, size=n, dtype=np.int64, endpoint=True)
    neg = np.unique(np.concatenate([rng.integers(0, n, size=500), [0, 524287, 524288, 524289, n - 1]]))
    x[neg] = -x[neg] - 1
    canon = np.zeros((n, 32), dtype=np.uint8)
    canon[:, :8] = np.where(x < 0, 0, x).astype("<i8").view(np.uint8).reshape(n, 8)
    canon[neg] = bytes32([int(v) for v in x[neg]])
    ref = oa.Witness(inst, oa.VarsAssignment.new(canon), inputs)
    zr = z_of(ref)[0]                                          # the host upload against Python integers on a sample: the edges of the first pass, every negated index, 4096 more
    sample = np.unique(np.concatenate([neg, rng.integers(0, n, size=4096)]))
    assert np.array_equal(zr[sample], oa.fr_from_ints([int(v) for v in x[sample]]))
    assert np.array_equal(zr[n:n + 3], oa.fr_from_ints([1] + INPUTS)) and not zr[n + 3:].any()
    assert_same(from_dev(inst, x, n, I64, inputs), ref, "2^20 packed i64 from_device")
    assert_same(oa.Witness.from_ints(inst, x, inputs), ref, "2^20 from_ints")
    assert z_of(ref)[1] == (n - len(neg)) / n


# ------------------------------------------------------------------------------------------------ integer edges
def test_integer_edges(small):
    inst, inputs = small
    for fmt, ints in ((I64, [0, 1, -1, I64_MAX, I64_MIN]), (U64, [0, 1, 2 ** 63, 2 ** 64 - 1])):
        want = oa.fr_from_ints([x % L for x in ints])
        for wit in (from_dev(inst, source(fmt, ints), len(ints), fmt, inputs), oa.Witness.from_ints(inst, source(fmt, ints), inputs)):
            z, sf = z_of(wit)
            assert np.array_equal(z[:len(ints)], want)
            assert not z[len(ints):V].any()
            n_small = sum(1 for x in ints if x % L < 2 ** 128)
            assert sf == (n_small + V - len(ints)) / V
    # negative numbers are l - |x|: none is below 2^128, so only the padding counts as small
    for nvars in (1, 100, V):
        ints = [-(k + 1) for k in range(nvars)]
        ints[0] = I64_MIN
        for wit in (from_dev(inst, source(I64, ints), nvars, I64, inputs), oa.Witness.from_ints(inst, source(I64, ints), inputs)):
            z, sf = z_of(wit)
            assert sf == (V - nvars) / V
            assert np.array_equal(z[:nvars], oa.fr_from_ints([x % L for x in ints]))


# ------------------------------------------------------------------------------------------------ strides
def test_strides(small, rng):
    inst, inputs = small
    n = 200
    table = rng.integers(I64_MIN, I64_MAX, size=(n, 3), dtype=np.int64, endpoint=True)       # row-major: column 1 is 24 bytes apart
    d = Dev(table)
    col = [int(x) for x in table[:, 1]]
    ref = host_witness(inst, inputs, col)
    assert_same(oa.Witness.from_device(inst, d.addr + 8, n, I64, inputs, stride_bytes=24), ref, "column 1 of (n, 3) int64", col)
    ints = values_for(C32, n, rng)
    wide = np.full((n, 64), 0xff, dtype=np.uint8)
    wide[:, :32] = bytes32(ints)
    ref = host_witness(inst, inputs, ints)
    assert_same(from_dev(inst, wide, n, C32, inputs, stride_bytes=64), ref, "canonical32 stride 64", ints)
    wide40 = np.full((n, 40), 0xff, dtype=np.uint8)              # a stride that rules the 16-byte loads out
    wide40[:, :32] = bytes32(ints)
    assert_same(from_dev(inst, wide40, n, C32, inputs, stride_bytes=40), ref, "canonical32 stride 40", ints)
    mont = np.zeros((n, 96), dtype=np.uint8)
    mont[:, :32] = source(M32, ints)
    assert_same(from_dev(inst, mont, n, M32, inputs, stride_bytes=96), ref, "montgomery32 stride 96", ints)
    for fmt in (C32, M32, I64, U64):                             # stride 0 is the packed size
        vals = values_for(fmt, n, rng)
        d = Dev(source(fmt, vals))
        packed = 8 if fmt in (I64, U64) else 32
        assert_same(oa.Witness.from_device(inst, d.addr, n, fmt, inputs, stride_bytes=packed), oa.Witness.from_device(inst, d.addr, n, fmt, inputs, stride_bytes=0), f"stride 0, format {fmt}", vals)
        assert_same(oa.Witness.from_device(inst, d.addr, n, fmt, inputs), host_witness(inst, inputs, vals), f"packed, format {fmt}", vals)


# ------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize("name", ["canonical32", "montgomery32"])
def test_scalars_not_below_l_are_refused(small, rng, name):
    inst, inputs = small
    fmt = FORMATS[name]
    ip = np.ascontiguousarray(inputs.assignment)
    for nvars, k in ((V, 0), (V, V - 1), (65, 64)):
        base = source(fmt, values_for(fmt, nvars, rng))
        for raw, ok in ((L, False), (L + 1, False), (2 ** 256 - 1, False), (L - 1, True)):
            src = base.copy()
            src[k] = np.frombuffer(raw.to_bytes(32, "little"), dtype=np.uint8)
            out, d = _vp(SENTINEL), Dev(src)
            rc = oa.lib.otti_witness_from_device(inst._h, d.addr, nvars, fmt, 0, ip.ctypes.data_as(_vp), ip.shape[0], None, ctypes.byref(out))
            if not ok:
                assert rc == INVALID_SCALAR and out.value == SENTINEL, (nvars, k, hex(raw), rc)
                continue
            assert rc == 0 and out.value != SENTINEL, (nvars, k, rc)
            wit = oa.Witness._adopt(out)
            want = raw * R % L if fmt == C32 else raw              # l - 1 as a value, or as the stored word itself
            assert np.array_equal(z_of(wit)[0][k], np.frombuffer(want.to_bytes(32, "little"), dtype=np.uint8))


# ------------------------------------------------------------------------------------------------ ordering on a caller's stream
def test_ingest_is_ordered_after_the_callers_stream(rng):
    KD = oa.kernels_dev
    inst, inputs = bare_instance(1 << 10)
    r = orc.rand_fr(rng, 10)
    want, _ = oa.kernels.eq_evals(r)
    stream = KD.stream_create()
    try:
        buf = oa.DeviceArray(1 << 10)
        assert oa.lib.otti_dev_upload(buf.ptr, np.zeros((1 << 10, 32), dtype=np.uint8).ctypes.data_as(_vp), 32 << 10) == 0
        KD.eq_evals(r, buf, stream)                              # queued on the caller's stream ...
        wit = oa.Witness.from_device(inst, buf, 1 << 10, M32, inputs, stream=stream)         # ... and read without a synchronisation in between
        z, _ = z_of(wit)
        assert np.array_equal(z[:1 << 10], want)
        assert np.array_equal(want, orc.eq_evals(r))
    finally:
        KD.stream_sync(stream)
        KD.stream_destroy(stream)


# ------------------------------------------------------------------------------------------------ update
RANGES = [(0, 1), (63, 2), (65, 130), (V - 1, 1), (0, V)]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", ["i64", "canonical32"])
def test_update_equals_a_fresh_upload(small, rng, name, where):
    inst, inputs = small
    fmt = FORMATS[name]
    cur = values_for(C32, V, rng)
    wit = host_witness(inst, inputs, cur)
    for first, count in RANGES:
        new = values_for(fmt, count, rng)
        if (first, count) == (65, 130) and fmt == I64:
            new = [-1 - k for k in range(count)]                 # a range that moves small_fraction a long way
        src = source(fmt, new)
        if where == "host":
            wit.update(inst, first, src)
        else:
            update_dev(wit, inst, first, src, count, fmt)
        cur[first:first + count] = [x % L for x in new]
        assert_same(wit, host_witness(inst, inputs, cur), f"{name} from {where} [{first}, {first + count})", cur)


def test_update_from_a_strided_device_source(small, rng):
    inst, inputs = small
    cur = values_for(C32, V, rng)
    wit = host_witness(inst, inputs, cur)
    table = rng.integers(I64_MIN, I64_MAX, size=(40, 3), dtype=np.int64, endpoint=True)
    update_dev(wit, inst, 100, table, 40, I64, offset=16, stride_bytes=24)
    cur[100:140] = [int(x) % L for x in table[:, 2]]
    assert_same(wit, host_witness(inst, inputs, cur), "column 2 of (40, 3) int64 into [100, 140)", cur)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", ["canonical32", "montgomery32"])
def test_failed_update_leaves_the_witness_unchanged(small, rng, name, where):
    inst, inputs = small
    fmt = FORMATS[name]
    wit = host_witness(inst, inputs, values_for(C32, V, rng))
    before, sf_before = z_of(wit)
    for first, count, k in ((0, V, 200), (60, 10, 0), (V - 5, 5, 4)):
        src = source(fmt, values_for(fmt, count, rng))
        src[k] = np.frombuffer(L.to_bytes(32, "little"), dtype=np.uint8)
        with pytest.raises(oa.R1CSError) as e:
            if where == "host":
                wit.update(inst, first, src, fmt=fmt)
            else:
                update_dev(wit, inst, first, src, count, fmt)
        assert e.value.code == INVALID_SCALAR
        after, sf_after = z_of(wit)
        assert np.array_equal(before, after) and sf_after == sf_before
    for first, count in ((V, 1), (V - 1, 2), (1, V)):
        with pytest.raises(oa.R1CSError) as e:
            wit.update(inst, first, np.zeros(count, dtype=np.int64))
        assert e.value.code == INVALID_NUM_VARS
    assert np.array_equal(before, z_of(wit)[0])


# ------------------------------------------------------------------------------------------------ whole proofs
LABEL, SEED = b"witness_device", b"\x2a" * 32
N = 1 << 10


def _int_case(kind, rng):
    if kind == "small_non_negative":
        ints = [int(x) for x in rng.integers(1, 1 << 20, size=N)]
    else:
        ints = [int(x) or 1 for x in rng.integers(I64_MIN, I64_MAX, size=N, endpoint=True)]
        ints[:4] = [-1, I64_MIN, I64_MAX, 1]
    r = int_r1cs(ints, [7, 8, 9])
    return r, np.array(ints, dtype=np.int64)


def _both(r):
    args = (r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    return oa.Instance.new(*args), oa.NIZKGens.new(*args[:3]), orc.OInstance(*args), orc.OGens(*args[:3])


@pytest.mark.parametrize("kind", ["small_non_negative", "mixed_signs"])
def test_proofs_from_integer_witnesses_are_the_oracles(rng, kind):
    r, x = _int_case(kind, rng)
    inst, gens, oinst, ogens = _both(r)
    assert oinst.is_sat(r["vars"], r["inputs"])
    want, _ = orc.nizk_prove(oinst, r["vars"], r["inputs"], ogens, LABEL, SEED)      # the host bytes are the values mod l
    inputs = oa.InputsAssignment.new(r["inputs"])
    proofs = {"host bytes": oa.NIZK.prove(inst, oa.VarsAssignment.new(r["vars"]), inputs, gens, LABEL, SEED)}
    proofs["from_device"] = oa.NIZK.prove(inst, from_dev(inst, x, N, I64, inputs), None, gens, LABEL, SEED)
    proofs["from_ints"] = oa.NIZK.prove(inst, oa.Witness.from_ints(inst, x, inputs), None, gens, LABEL, SEED)
    off = x.copy()
    off[100:300] += 1; off[N - 1] = 5
    upd = oa.Witness.from_ints(inst, off, inputs)
    assert upd.check_sat(inst).n_unsat > 0
    upd.update(inst, 100, x[100:300])
    update_dev(upd, inst, N - 1, x[N - 1:], 1, I64)
    proofs["updated"] = oa.NIZK.prove(inst, upd, None, gens, LABEL, SEED)
    for name, p in proofs.items():
        assert p.bytes == want, f"{kind}: the proof from `{name}` differs from the oracle's"
    proofs["from_device"].verify(inst, inputs, gens, LABEL)
    assert orc.nizk_verify(oinst, r["inputs"], ogens, proofs["updated"].bytes, LABEL) == 0


def test_compiler_like_witness_takes_the_sparse_commitment():
    n, ni = 1 << 16, 10                                         # 2^16 scalars: the size from which the commitment is a bulk launch, and so can be the sparse one
    r = oa.synth_r1cs_compiler_like(n, ni, 5)
    inst, gens, oinst, ogens = _both(r)
    inputs = oa.InputsAssignment.new(r["inputs"])
    wit = from_dev(inst, r["vars"], n, C32, inputs)
    ref = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), inputs)
    assert_same(wit, ref, "compiler-like 2^16", ints_of(r["vars"]), nv=n, inputs=ints_of(r["inputs"]))
    assert wit.info[2] > 0.25
    want, _ = orc.nizk_prove(oinst, r["vars"], r["inputs"], ogens, LABEL, SEED)
    assert oa.NIZK.prove(inst, wit, None, gens, LABEL, SEED).bytes == want
    assert oa.NIZK.prove(inst, oa.VarsAssignment.new(r["vars"]), inputs, gens, LABEL, SEED).bytes == want


def test_snark_proof_from_a_device_witness():
    r = oa.synth_r1cs(2, 0, 7)                                  # the smallest instance test_gpu_snark.py proves
    nz = max(r["A"].size, r["B"].size, r["C"].size)
    args = (r["num_cons"], r["num_vars"], r["num_inputs"])
    inst = oa.Instance.new(*args, r["A"], r["B"], r["C"])
    gens = oa.SNARKGens.new(*args, nz)
    comm = oa.ComputationCommitment.encode(inst, gens)
    v, i = oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"])
    want = oa.SNARK.prove(inst, comm, v, i, gens, b"snark_example", SEED).bytes
    wit = from_dev(inst, r["vars"], r["vars"].shape[0], C32, i)
    got = oa.SNARK.prove(inst, comm, wit, None, gens, b"snark_example", SEED)
    assert got.bytes == want
    got.verify(oa.ComputationCommitment.from_bytes(comm.bytes), i, gens, b"snark_example")


# ------------------------------------------------------------------------------------------------ satisfiability check
def test_check_sat_follows_updates(rng):
    r, x = _int_case("mixed_signs", rng)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    inputs = oa.InputsAssignment.new(r["inputs"])
    wit = from_dev(inst, x, N, I64, inputs)
    assert wit.check_sat(inst).n_unsat == 0
    k = 321
    z = [int(v) % L for v in x] + [1, 7, 8, 9]
    z[k] = (z[k] + 1) % L
    want = [row for row, (a, b, c, coef) in enumerate(r["rows"]) if z[a] * z[b] % L != coef * z[c] % L]
    assert k in want                                            # row k reads variable k in A
    wit.update(inst, k, np.array([int(x[k]) + 1], dtype=np.int64))
    rep = wit.check_sat(inst, max_rows=64)
    assert rep.n_unsat == len(want) and rep.rows.tolist() == want[:64]
    update_dev(wit, inst, k, x[k:k + 1], 1, I64)
    assert wit.check_sat(inst).n_unsat == 0
