"""What the assign entry points (otti_witness_assign, otti_witness_diff, otti_witness_assign_info, otti_k_witness_diff) promise without a GPU:
exported, declared and bound symbols with the header's signatures, a header that states the contract, argument errors answered before any device is
touched (the witness pointers below are never dereferenced), an empty range answered OTTI_OK, OTTI_ERR_NO_DEVICE for valid arguments without a
device — and the pure-Python model of the comparison (assign_cases.model_diff), which the GPU tests judge the kernels by, against the oracle's field."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import otti_amd as oa
import orc
import assign_cases as ac
from assign_cases import C32, I64, M32, Q, U64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
SIGNATURES = {
    "otti_witness_assign": "otti_instance *inst, otti_witness *wit, size_t first, const void *src, size_t count, int32_t format, size_t stride_bytes, "
                           "int32_t src_on_device, void *stream, uint64_t *n_changed",
    "otti_witness_diff": "otti_instance *inst, const otti_witness *wit, size_t first, const void *src, size_t count, int32_t format, size_t stride_bytes, "
                         "int32_t src_on_device, void *stream, uint64_t *n_changed, uint64_t *idx, size_t idx_cap",
    "otti_witness_assign_info": "const otti_witness *wit, uint64_t *calls, uint64_t *changed, uint64_t *resums",
    "otti_k_witness_diff": "const uint8_t *h_old, size_t n, const void *h_src, int32_t format, size_t stride_bytes, uint8_t *h_new, uint64_t *h_idx, "
                           "uint8_t *h_delta, uint64_t *n_changed, uint32_t *chunk, float *kernel_ms",
}
OK, BAD_ARG, NO_DEVICE, NUM_VARS = 0, -21, -20, -4
SENTINEL = 0x5e5e5e5e
V, NI = 8, 2
_vp = ctypes.c_void_p


def _inst():
    r = oa.synth_r1cs(V, NI, 1)
    return oa.Instance.new(V, V, NI, r["A"], r["B"], r["C"])


def _p(a):
    return a.ctypes.data_as(_vp)


def test_symbols_exported_declared_and_bound():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = " ".join(open(HEADER).read().split())
    for name, params in SIGNATURES.items():
        assert re.search(r"\bT %s\b" % name, syms), name
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert " ".join(m.group(1).split()) == " ".join(params.split()), name
        f = getattr(oa.lib, name)
        assert len(f.argtypes) == params.count(",") + 1, name
    for name in ("assign", "diff", "assign_info"):
        assert hasattr(oa.Witness, name), name
    assert hasattr(oa.kernels, "witness_diff")


def test_header_states_the_contract():
    text = " ".join(open(HEADER).read().split())
    i = text.index("---- assign: variables [first, first + count)")
    block = text[i:text.index("int32_t otti_witness_assign(", i)]
    for phrase in ("bit for bit", "byte-identical", "must not overlap", "Never while a proof or check", "Sharded provers call it on every rank",
                   "HBM is short", "OTTI_ASSIGN_RESUM_SHARE", "profiles/witness_assign.md", "count == 0", "changes nothing", "OTTI_ERR_INVALID_SCALAR"):
        assert phrase in block, phrase


def test_argument_errors_come_before_any_device():
    inst = _inst()
    fake = _vp(4096)                                           # never dereferenced: every case below is refused on its arguments alone
    assign, diff, info = oa.lib.otti_witness_assign, oa.lib.otti_witness_diff, oa.lib.otti_witness_assign_info
    src = np.array([5, 6], dtype=np.int64)
    n = ctypes.c_uint64(SENTINEL)
    nb = ctypes.byref(n)
    idx = np.full(4, SENTINEL, dtype=np.uint64)

    def both(inst_h, wit, first, s, count, fmt, stride, on_dev):
        """the two calls on the same arguments: they refuse alike"""
        a = assign(inst_h, wit, first, s, count, fmt, stride, on_dev, None, nb)
        d = diff(inst_h, wit, first, s, count, fmt, stride, on_dev, None, nb, _p(idx), 4)
        assert a == d, (a, d)
        return a

    assert both(None, fake, 0, _p(src), 2, I64, 0, 0) == BAD_ARG                # null handles
    assert both(inst._h, None, 0, _p(src), 2, I64, 0, 0) == BAD_ARG
    assert both(inst._h, fake, 0, None, 2, I64, 0, 0) == BAD_ARG                # null source with a count
    assert both(inst._h, fake, 0, None, 2, C32, 0, 1) == BAD_ARG
    for fmt in (-1, 4, 99):                                                       # unknown formats
        assert both(inst._h, fake, 0, _p(src), 2, fmt, 0, 0) == BAD_ARG
    for fmt, stride in ((I64, 4), (U64, 7), (I64, 12), (C32, 8), (C32, 24), (M32, 31), (C32, 36), (M32, 33)):
        assert both(inst._h, fake, 0, fake, 1, fmt, stride, 0) == BAD_ARG, (fmt, stride)
        assert both(inst._h, fake, 0, fake, 1, fmt, stride, 1) == BAD_ARG, (fmt, stride)
    for fmt in (C32, M32, I64, U64):                                              # a device source off the 8-byte grid
        assert both(inst._h, fake, 0, _vp(4100), 1, fmt, 0, 1) == BAD_ARG
    # diff's own: a null count, room for indices without a list
    assert diff(inst._h, fake, 0, _p(src), 2, I64, 0, 0, None, None, _p(idx), 4) == BAD_ARG
    assert diff(inst._h, fake, 0, _p(src), 2, I64, 0, 0, None, nb, None, 4) == BAD_ARG
    # a bad argument is named before a bad range
    assert both(inst._h, fake, V, _p(src), 2, 4, 0, 0) == BAD_ARG
    # ranges beyond the padded num_vars
    assert both(inst._h, fake, V, _p(src), 1, I64, 0, 0) == NUM_VARS
    assert both(inst._h, fake, 1, fake, V, C32, 0, 1) == NUM_VARS
    assert both(inst._h, fake, 2 ** 64 - 1, _p(src), 2, I64, 0, 0) == NUM_VARS    # first + count wraps round
    assert both(inst._h, fake, V + 1, None, 0, I64, 0, 0) == NUM_VARS
    assert n.value == SENTINEL and (idx == SENTINEL).all()

    a, b, c = ctypes.c_uint64(SENTINEL), ctypes.c_uint64(SENTINEL), ctypes.c_uint64(SENTINEL)
    assert info(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == BAD_ARG
    assert info(None, None, None, None) == BAD_ARG
    assert (a.value, b.value, c.value) == (SENTINEL,) * 3

    k = oa.lib.otti_k_witness_diff
    old, new, delta = np.zeros((2, 32), dtype=np.uint8), np.zeros((2, 32), dtype=np.uint8), np.zeros((2, 32), dtype=np.uint8)
    kidx = np.zeros(2, dtype=np.uint64)
    assert k(_p(old), 2, _p(src), 4, 0, _p(new), _p(kidx), _p(delta), nb, None, None) == BAD_ARG       # unknown format
    assert k(_p(old), 2, _p(src), I64, 12, _p(new), _p(kidx), _p(delta), nb, None, None) == BAD_ARG    # bad stride
    assert k(_p(old), 2, _p(src), C32, 24, _p(new), _p(kidx), _p(delta), nb, None, None) == BAD_ARG
    assert k(None, 2, _p(src), I64, 0, _p(new), _p(kidx), _p(delta), nb, None, None) == BAD_ARG
    assert k(_p(old), 2, None, I64, 0, _p(new), _p(kidx), _p(delta), nb, None, None) == BAD_ARG
    assert k(_p(old), 2, _p(src), I64, 0, _p(new), _p(kidx), _p(delta), None, None, None) == BAD_ARG
    assert n.value == SENTINEL


def test_an_empty_range_is_ok_and_touches_nothing():
    inst = _inst()
    fake = _vp(4096)
    n = ctypes.c_uint64(SENTINEL)
    assert oa.lib.otti_witness_assign(inst._h, fake, 3, None, 0, I64, 0, 0, None, ctypes.byref(n)) == OK
    assert n.value == 0
    assert oa.lib.otti_witness_assign(inst._h, fake, V, None, 0, C32, 0, 1, None, None) == OK           # n_changed may be NULL
    n.value = SENTINEL
    idx = np.full(2, SENTINEL, dtype=np.uint64)
    assert oa.lib.otti_witness_diff(inst._h, fake, 0, None, 0, U64, 0, 0, None, ctypes.byref(n), _p(idx), 2) == OK
    assert n.value == 0 and (idx == SENTINEL).all()
    assert oa.lib.otti_witness_diff(inst._h, fake, 0, None, 0, U64, 0, 0, None, ctypes.byref(n), None, 0) == OK
    chunk = ctypes.c_uint32(0)
    assert oa.lib.otti_k_witness_diff(None, 0, None, I64, 0, None, None, None, ctypes.byref(n), ctypes.byref(chunk), None) == OK
    assert n.value == 0 and chunk.value >= 64 and chunk.value % 64 == 0


@pytest.mark.skipif(oa.device_count() > 0, reason="only meaningful without a GPU")
def test_valid_arguments_without_a_device_are_no_device():
    inst = _inst()
    fake = _vp(4096)
    src = np.array([5, -6], dtype=np.int64)
    n = ctypes.c_uint64(SENTINEL)
    idx = np.full(2, SENTINEL, dtype=np.uint64)
    assert oa.lib.otti_witness_assign(inst._h, fake, 2, _p(src), 2, I64, 0, 0, None, ctypes.byref(n)) == NO_DEVICE
    assert oa.lib.otti_witness_assign(inst._h, fake, 0, fake, V, C32, 64, 1, None, None) == NO_DEVICE
    assert oa.lib.otti_witness_diff(inst._h, fake, 2, _p(src), 2, I64, 0, 0, None, ctypes.byref(n), _p(idx), 2) == NO_DEVICE
    assert oa.lib.otti_witness_diff(inst._h, fake, 0, fake, V, M32, 0, 1, None, ctypes.byref(n), None, 0) == NO_DEVICE
    assert (idx == SENTINEL).all()
    a = ctypes.c_uint64(SENTINEL)
    assert oa.lib.otti_witness_assign_info(fake, ctypes.byref(a), None, None) == NO_DEVICE
    assert a.value == SENTINEL
    old = np.zeros((2, 32), dtype=np.uint8)
    with pytest.raises(oa.NoDeviceError):
        oa.kernels.witness_diff(old, src, I64)
    w = oa.Witness._adopt(fake)
    try:
        with pytest.raises(oa.NoDeviceError):
            w.assign(inst, src)
        with pytest.raises(oa.NoDeviceError):
            w.diff(inst, src, first=1)
        with pytest.raises(oa.NoDeviceError):
            w.assign_info()
    finally:
        w._h = None                                            # not a handle: nothing to free


def test_python_names_the_types_it_takes():
    w = oa.Witness._adopt(None)                                # no handle: the values are looked at before the library is called
    inst = _inst()
    for bad in ([1, 2, 3], "abc", 7, np.zeros(3, dtype=np.float64)):
        with pytest.raises(ValueError):
            w.assign(inst, bad)
        with pytest.raises(ValueError):
            w.diff(inst, bad)
    with pytest.raises(ValueError):
        w.assign(inst, (4096, 2))                              # a device address without fmt
    with pytest.raises(ValueError):
        oa.kernels.witness_diff(np.zeros((3, 32), dtype=np.uint8), np.zeros(2, dtype=np.int64), I64)   # a source shorter than the vector


# ------------------------------------------------------------------------------------------------ the model
def test_model_values_agree_with_the_oracles_field():
    """value_of / mont_words against orc.fr_from_ints / fr_to_ints (the oracle's Montgomery form), on the values the GPU tests reuse"""
    vals = [0, 1, 5, Q - 5, Q - 1, 2 ** 128 - 1, 2 ** 128, 2 ** 63, 2 ** 64 - 1, (Q - 2 ** 63) % Q]
    words = np.ascontiguousarray(orc.fr_from_ints(vals)).reshape(-1, 32)
    assert (ac.mont_words(vals) == words).all()
    assert [int(x) for x in orc.fr_to_ints(words)] == vals
    raw = [int.from_bytes(bytes(w), "little") for w in words]
    assert [ac.value_of(x, M32) for x in raw] == vals           # the raw word stands for the value
    assert ac.encode(vals, M32) == raw
    assert [ac.value_of(v, C32) for v in vals] == vals
    assert ac.value_of(-5, I64) == Q - 5 and ac.value_of(-2 ** 63, I64) == Q - 2 ** 63 and ac.value_of(2 ** 64 - 1, U64) == 2 ** 64 - 1
    for fmt in (C32, M32):
        for x in (Q, Q + 1, 2 ** 256 - 1):
            with pytest.raises(ac.Refused):
                ac.value_of(x, fmt)
        assert ac.value_of(Q - 1, fmt) == (Q - 1 if fmt == C32 else (Q - 1) * pow(ac.R_MONT, -1, Q) % Q)


def test_model_diff_compares_values_not_clothes():
    old = [Q - 5, 7, 0, 2 ** 128 - 1, Q - 1, Q - 2 ** 63]
    assert ac.model_diff(old, [-5, 7, 0, 1, -1, -2 ** 63], I64) == ([3], [(1 - (2 ** 128 - 1)) % Q])
    assert ac.model_diff(old, old, C32) == ([], [])
    assert ac.model_diff(old, ac.encode(old, M32), M32) == ([], [])
    assert ac.model_diff([0, 0], [0, 0], U64) == ([], [])
    # the ends of the field, both ways
    assert ac.model_diff([0, Q - 1], [Q - 1, 0], C32) == ([0, 1], [Q - 1, 1])
    assert ac.model_diff([2 ** 128 - 1, 2 ** 128], [2 ** 128, 2 ** 128 - 1], C32) == ([0, 1], [1, Q - 1])
    idx, delta = ac.model_diff([3] * 5, [3, 4, 3, 2, 3], U64)
    assert idx == [1, 3] and delta == [1, Q - 1]
    # deltas are what the patch adds: old + delta = new in the oracle's field
    rng = np.random.default_rng(7)
    a, b = [int(x) for x in orc.fr_to_ints(orc.rand_fr(rng, 16))], [int(x) for x in orc.fr_to_ints(orc.rand_fr(rng, 16))]
    b[::3] = a[::3]
    idx, delta = ac.model_diff(a, b, C32)
    assert idx == [i for i in range(16) if i % 3]
    assert [(a[i] + d) % Q for i, d in zip(idx, delta)] == [b[i] for i in idx]
    with pytest.raises(ac.Refused):
        ac.model_diff([1, 2], [1, Q], C32)


def test_patterns_and_raw_bytes():
    chunk = 1024
    for n in (1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 17):
        for name in ac.PATTERNS:
            pos = ac.pattern(name, n, chunk)
            assert pos == sorted(set(pos)) and all(0 <= i < n for i in pos), (name, n)
        assert len(ac.pattern("one per chunk", n, chunk)) == (n + chunk - 1) // chunk
    assert ac.pattern("wave edges", 130, chunk) == [63, 64, 127, 128]
    b = ac.raw_bytes([-1, 2], I64, 24)
    assert b.size == 32 and bytes(b[:8]) == b"\xff" * 8 and b[8] == 0xa5 and bytes(b[24:]) == (2).to_bytes(8, "little")
    assert bytes(ac.raw_bytes([Q - 1], C32)) == (Q - 1).to_bytes(32, "little")
    assert ac.raw_bytes([], C32).size == 0
