"""The two passes of otti_witness_assign at kernel level (otti_k_witness_diff: k_witness_diff_count, _scan and _apply of k_field.hip) against the
pure-Python model of assign_cases.py, for exact equality of the new vector, the ascending list of changed indices, their deltas and the count.

Sizes sit on the boundaries of the kernels' geometry — a wave (64), the workgroup's chunk as the entry reports it, several chunks with a ragged
tail; patterns on the boundaries of the rank computation (the last lane of a wave and the first of the next, one element per chunk, every other
lane).  The resident vector of each format is made once per module and only read."""
import ctypes

import numpy as np
import pytest

import otti_amd as oa
import assign_cases as ac
from assign_cases import C32, I64, M32, Q, U64
from witness_cases import values

pytestmark = pytest.mark.gpu
INVALID_SCALAR = -5
_vp = ctypes.c_void_p


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def _chunk():
    n, chunk = ctypes.c_uint64(), ctypes.c_uint32()
    assert oa.lib.otti_k_witness_diff(None, 0, None, I64, 0, None, None, None, ctypes.byref(n), ctypes.byref(chunk), None) == 0
    return chunk.value


CHUNK = _chunk()
SIZES = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17)
NMAX = max(SIZES)


@pytest.fixture(scope="module")
def resident():
    """per format: NMAX source elements (as integers in that format), the values they stand for, and those values' Montgomery words"""
    rng = np.random.default_rng(20261019)
    out = {}
    for fmt in (C32, M32, I64, U64):
        if fmt == I64:
            elems = [int(x) for x in rng.integers(-2 ** 63, 2 ** 63 - 1, size=NMAX, endpoint=True)]
            elems[:4] = [-1, -2 ** 63, 2 ** 63 - 1, 0]
        elif fmt == U64:
            elems = [int(x) for x in rng.integers(0, 2 ** 64 - 1, size=NMAX, endpoint=True, dtype=np.uint64)]
            elems[:3] = [0, 2 ** 64 - 1, 1]
        else:
            elems = ac.encode(values(rng, NMAX), fmt)
        vals = [ac.value_of(x, fmt) for x in elems]
        out[fmt] = (elems, vals, ac.mont_words(vals))
    return out


def _other(x, i, fmt):
    """a source element whose value differs from x's"""
    if fmt == I64:
        return x + 1 + i % 5 if x < 2 ** 62 else x - 1 - i % 5
    if fmt == U64:
        return x + 1 + i % 5 if x < 2 ** 63 else x - 1 - i % 5
    return (x + 1 + i) % Q                                      # for MONTGOMERY32 another raw word below l: another value


def _run(old_words, elems, fmt, stride):
    return oa.kernels.witness_diff(old_words, ac.raw_bytes(elems, fmt, stride), fmt, stride)


def _check(old_vals, old_words, elems, fmt, stride, what):
    want_idx, want_delta = ac.model_diff(old_vals, elems, fmt)
    new, idx, delta, chunk = _run(old_words, elems, fmt, stride)
    assert chunk == CHUNK
    assert len(idx) == len(want_idx), (what, len(idx), len(want_idx))
    assert idx.tolist() == want_idx, what
    assert (delta == ac.mont_words(want_delta).reshape(-1, 32)).all(), what
    assert (new == ac.mont_words(ac.apply_model(old_vals, elems, fmt))).all(), what


@pytest.mark.parametrize("strided", [False, True], ids=["packed", "strided"])
@pytest.mark.parametrize("fmt", [C32, M32, I64, U64], ids=["canonical32", "montgomery32", "i64", "u64"])
def test_sizes_and_patterns(resident, fmt, strided):
    elems, vals, words = resident[fmt]
    stride = 0 if not strided else (24 if fmt in (I64, U64) else 48)
    for n in SIZES:
        for name in ac.PATTERNS:
            pos = ac.pattern(name, n, CHUNK)
            new = list(elems[:n])
            for i in pos:
                new[i] = _other(new[i], i, fmt)
            want_idx, _ = ac.model_diff(vals[:n], new, fmt)
            assert want_idx == pos                              # the pattern is what the model sees
            _check(vals[:n], words[:n], new, fmt, stride, (n, name))


def test_equal_values_in_other_clothes_are_unchanged():
    """each with a really changed neighbour, so that "nothing found" is not the answer"""
    old = [Q - 5, 3, Q - 5]
    words = ac.mont_words(old)
    _check(old, words, [-5, 4, -5], I64, 0, "I64 -5 over l - 5")
    _check(old, words, [Q - 5, 4, Q - 5], C32, 0, "CANONICAL32 over the same value")
    raw = ac.encode(old, M32)
    _check(old, words, [raw[0], ac.encode([4], M32)[0], raw[2]], M32, 0, "MONTGOMERY32 over the identical word")
    _check([0, 3, 0], ac.mont_words([0, 3, 0]), [0, 4, 0], U64, 0, "U64 0 over the padding's zero")
    for fmt, elems in ((I64, [-5, 3, -5]), (C32, old), (M32, raw), (U64, None)):
        o = old if elems is not None else [0, 3, 0]
        e = elems if elems is not None else [0, 3, 0]
        new, idx, delta, _ = _run(ac.mont_words(o), e, fmt, 0)
        assert len(idx) == 0 and len(delta) == 0 and (new == ac.mont_words(o)).all(), fmt


def test_the_ends_of_the_field():
    old = [0, Q - 1, 2 ** 128 - 1, 2 ** 128, 0, Q - 2 ** 63, 2 ** 63]
    words = ac.mont_words(old)
    _check(old, words, [Q - 1, 0, 2 ** 128, 2 ** 128 - 1, Q - 2 ** 63, 0, Q - 2 ** 63], C32, 0, "canonical ends")
    _check(old, words, ac.encode([Q - 1, 0, 2 ** 128, 2 ** 128 - 1, Q - 2 ** 63, 0, Q - 2 ** 63], M32), M32, 48, "montgomery ends")
    old = [0, Q - 1, 0, Q - 2 ** 63, 2 ** 63, 2 ** 63 - 1, 1]
    words = ac.mont_words(old)
    # -1 over 0 and 0 over l - 1; INT64_MIN over 0, over itself (unchanged) and over +2^63; INT64_MAX over itself; 0 over 1
    elems = [-1, 0, -2 ** 63, -2 ** 63, -2 ** 63, 2 ** 63 - 1, 0]
    want_idx, _ = ac.model_diff(old, elems, I64)
    assert want_idx == [0, 1, 2, 4, 6]
    _check(old, words, elems, I64, 0, "int64 ends")
    _check([2 ** 63, 2 ** 64 - 1, 0], ac.mont_words([2 ** 63, 2 ** 64 - 1, 0]), [2 ** 63, 0, 2 ** 64 - 1], U64, 24, "uint64 ends")


@pytest.mark.parametrize("fmt,word", [(C32, Q), (M32, Q), (M32, 2 ** 256 - 1), (C32, 2 ** 255)],
                         ids=["canonical l", "montgomery raw l", "montgomery raw 2^256-1", "canonical 2^255"])
@pytest.mark.parametrize("at", ["second wave", "second chunk"])
def test_a_refused_scalar_leaves_the_outputs_untouched(resident, fmt, word, at):
    elems, vals, words = resident[fmt]
    n = CHUNK + 5
    k = 70 if at == "second wave" else CHUNK + 2
    new = list(elems[:n])
    for i in (0, 1, 2, 3, k - 1):                               # real changes before the refused one
        new[i] = _other(new[i], i, fmt)
    new[k] = word
    with pytest.raises(ac.Refused):
        ac.model_diff(vals[:n], new, fmt)
    src = ac.raw_bytes(new, fmt)
    old = np.ascontiguousarray(words[:n])
    h_new, h_delta = np.full((n, 32), 0x5e, dtype=np.uint8), np.full((n, 32), 0x5e, dtype=np.uint8)
    h_idx, cnt = np.full(n, 0x5e5e5e5e, dtype=np.uint64), ctypes.c_uint64(0x5e5e5e5e)
    p = lambda a: a.ctypes.data_as(_vp)                         # noqa: E731
    rc = oa.lib.otti_k_witness_diff(p(old), n, p(src), fmt, 0, p(h_new), p(h_idx), p(h_delta), ctypes.byref(cnt), None, None)
    assert rc == INVALID_SCALAR
    assert (h_new == 0x5e).all() and (h_delta == 0x5e).all() and (h_idx == 0x5e5e5e5e).all() and cnt.value == 0x5e5e5e5e
    with pytest.raises(oa.R1CSError) as e:
        oa.kernels.witness_diff(old, src, fmt)
    assert e.value.code == INVALID_SCALAR
