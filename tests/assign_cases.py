"""Shared by the tests of otti_witness_assign / otti_witness_diff (test_witness_assign_host.py, test_gpu_witness_diff_kernel.py,
test_gpu_witness_assign.py): the pure-Python model of the comparison, the raw bytes of a source in each format, and the change patterns.  A plain
module like witness_cases.py; nothing here is collected and nothing here calls the library."""
import numpy as np

import orc

Q = orc.L_ORDER
R_MONT = (1 << 256) % Q
R_INV = pow(R_MONT, -1, Q)
C32, M32, I64, U64 = 0, 1, 2, 3
FORMATS = {"canonical32": C32, "montgomery32": M32, "i64": I64, "u64": U64}


class Refused(Exception):
    """a 32-byte word that is not below l"""


def value_of(x, fmt):
    """the field element a source element stands for.  Integers: the number mod l (int64 may be negative); CANONICAL32: the number itself, which
    has to be below l; MONTGOMERY32: the raw word w, which has to be below l, standing for w / 2^256."""
    x = int(x)
    if fmt == I64:
        assert -2 ** 63 <= x < 2 ** 63
        return x % Q
    if fmt == U64:
        assert 0 <= x < 2 ** 64
        return x
    assert 0 <= x < 2 ** 256
    if x >= Q:
        raise Refused(x)
    return x if fmt == C32 else x * R_INV % Q


def model_diff(old_ints, new_values, fmt):
    """(idx, delta mod l): the ascending positions whose VALUE differs and new - old there.  old_ints: the resident values as integers below l;
    new_values: the source elements as integers in `fmt` (value_of)."""
    assert len(old_ints) == len(new_values)
    idx, delta = [], []
    for i, (o, x) in enumerate(zip(old_ints, new_values)):
        v = value_of(x, fmt)
        if v != o % Q:
            idx.append(i)
            delta.append((v - o) % Q)
    return idx, delta


def apply_model(old_ints, new_values, fmt):
    """the values afterwards"""
    return [value_of(x, fmt) for x in new_values] if len(new_values) else list(old_ints)


def encode(vals, fmt):
    """source elements in `fmt` that stand for the field elements vals (integers: the values themselves, which must fit)"""
    if fmt == I64:
        return [int(v) for v in vals]
    if fmt == U64:
        return [int(v) for v in vals]
    if fmt == C32:
        return [int(v) % Q for v in vals]
    return [int(v) % Q * R_MONT % Q for v in vals]


def raw_bytes(elems, fmt, stride=0):
    """the bytes of a source: element i at i * stride (0: packed), the gaps filled with 0xa5"""
    eb = 8 if fmt in (I64, U64) else 32
    stride = stride or eb
    n = len(elems)
    out = np.full(max((n - 1) * stride + eb, 0) if n else 0, 0xa5, dtype=np.uint8)
    for i, x in enumerate(elems):
        x = int(x)
        b = (x % (1 << 64)).to_bytes(8, "little") if eb == 8 else x.to_bytes(32, "little")
        out[i * stride:i * stride + eb] = np.frombuffer(b, dtype=np.uint8)
    return out


def mont_words(ints):
    """(n, 32) uint8 Montgomery words of field elements, computed here (not by the library)"""
    return np.array([np.frombuffer((int(x) % Q * R_MONT % Q).to_bytes(32, "little"), dtype=np.uint8) for x in ints], dtype=np.uint8).reshape(-1, 32)


PATTERNS = ("none", "all", "first", "last", "wave edges", "one per chunk", "every other")


def pattern(name, n, chunk):
    """the positions a pattern changes among n elements"""
    if name == "none":
        return []
    if name == "all":
        return list(range(n))
    if name == "first":
        return [0]
    if name == "last":
        return [n - 1]
    if name == "wave edges":                                   # the last lane of every wave and the first of the next
        return [i for i in range(n) if i % 64 in (63, 0) and i > 0]
    if name == "one per chunk":
        return [min(c * chunk + (7 * c + 3) % chunk, n - 1) for c in range((n + chunk - 1) // chunk)]
    if name == "every other":
        return list(range(0, n, 2))
    raise KeyError(name)
