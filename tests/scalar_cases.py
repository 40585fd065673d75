"""Operands and the plain big-integer reference for the device's arithmetic over GF(l), l the order of ristretto255: the eight-word Montgomery form
(field.h Fr) and the nine limbs of 29 bits (fr9.h Fr9, Montgomery radix 2^261; fold9 of kernels_common.h).  Needs no GPU and nothing of the product.
The counterpart of curve_cases.py.

What is restated here and why:
    * arithmetic mod l on Python integers, the value of a limb vector (sum v_i 2^(29 i)), the normalised limbs of an integer: THE reference;
    * the borrow-proof limbs of K l (fr9_kl_limb), recomputed from l, and limb-wise a + b, a - b + K l: exact by definition;
    * the C bodies of fr9_mul and fr9_fold_top, limb for limb: their results are one representative among several, so the limbs a device result must
      equal come from the transcription, and the transcription itself is held against the integers (test_scalar_cases_host.py: the value mod l, the
      value bound, every column of the product below 2^64).
Every operation has a PRECONDITION (what fr9.h states for it) that every committed case satisfies; a case is never dropped to make that hold."""
import functools
import itertools
import math
import random

L = 2 ** 252 + 27742317777372353535851937790883648493
R = 2 ** 256 % L                                                 # the memory format: a stored word is x R mod l
RINV = pow(R, -1, L)
M29 = 2 ** 29 - 1
KS = (2, 4, 8, 16, 128)


def limbs_of(v):
    """the normalised limbs of an integer below 2^264: limbs 0..7 of 29 bits, limb 8 the rest"""
    assert 0 <= v < 2 ** 264
    return tuple((v >> (29 * i)) & M29 for i in range(8)) + (v >> 232,)


def value(v):
    return sum(int(x) << (29 * i) for i, x in enumerate(v))


def normalised(v):
    return all(0 <= x <= M29 for x in v[:8]) and 0 <= v[8] < 2 ** 32


L9 = limbs_of(L)                                                 # FR9_L0 .. FR9_L8
LINV = (-pow(L, -1, 2 ** 29)) % 2 ** 29                          # FR9_LINV


def kl_limbs(K):
    """fr9_kl_limb(K, 0 .. 8): K l with every limb but the top one raised by what the limb above gives up"""
    t = limbs_of(K * L)
    return (t[0] + 2 ** 29,) + tuple(x + M29 for x in t[1:8]) + (t[8] - 1,)


# the "loose" operand classes of fr9_mul (fr9.h): a column holds nine a_i b_j, quotient digits times limbs of l and a carry-in
S = 2 * L9[0] + L9[1] + L9[2] + L9[3] + L9[4] + L9[8]
ROOM = 2 ** 64 - M29 * S - 2 ** 36
B_A = ROOM // (9 * M29)                                          # beside an operand with all nine limbs below 2^29
B_B = math.isqrt(ROOM // 9)                                      # both operands
assert (B_A, B_B) == (3597011027, 1389651246)
assert sum(x != 0 for x in L9) == 6 and L9[5] == L9[6] == L9[7] == 0


# ------------------------------------------------------------------------------------------------ the operations on integers
def unpack_s(x, s):
    """fr9_unpack_s<S>: the limbs of x << S"""
    return limbs_of(x << s)


def add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def sub_kl(K, a, b):
    return tuple(x + o - y for x, y, o in zip(a, b, kl_limbs(K)))


def norm(a):
    return limbs_of(value(a))


def shl5(a):
    return limbs_of(value(a) << 5)


def mul_columns(a, b):
    """the C body of fr9_mul on integers: (result limbs, the largest value the accumulator takes)"""
    m, r, acc, top = [0] * 9, [0] * 9, 0, 0
    for k in range(17):
        for i in range(9):
            if 0 <= k - i < 9:
                acc += a[i] * b[k - i]
        for i in range(min(k, 9)):
            if 1 <= k - i < 9:
                acc += m[i] * L9[k - i]
        if k < 9:
            m[k] = (acc * LINV) & M29
            acc += m[k] * L9[0]
        else:
            r[k - 9] = acc & M29
        top = max(top, acc)
        acc >>= 29
    r[8] = acc
    return tuple(r), top


def mul(a, b):
    return mul_columns(a, b)[0]


def fold_top(a):
    """the C body of fr9_fold_top: low 252 bits + l - q delta (q = the bits from 252 up, delta = l - 2^252), then one carry sweep"""
    q = a[8] >> 20
    d, acc = [], 0
    for j in range(5):
        acc += q * L9[j]; d.append(acc & M29); acc >>= 29
    d += [acc, 0, 0]
    o = kl_limbs(1)
    r = [a[i] + o[i] - d[i] for i in range(8)] + [(a[8] & 0xfffff) + o[8]]
    assert all(0 <= x < 2 ** 32 for x in r)
    return norm(r)


def fold9(x0, x2, r):
    """fold9 (kernels_common.h) on three stored words: the limbs it hands on"""
    a = unpack_s(x0, 0)
    return norm(add(a, mul(unpack_s(r, 5), sub_kl(2, unpack_s(x2, 0), a))))


# ------------------------------------------------------------------------------------------------ words
def _dedupe(vals):
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v); out.append(v)
    return tuple(out)


NAMED = {"0": 0, "1": 1, "2": 2, "l-1": L - 1, "l-2": L - 2, "(l+1)/2": (L + 1) // 2, "(l-1)/2": (L - 1) // 2, "2^252": 2 ** 252, "2^252-1": 2 ** 252 - 1,
         "l-2^232": L - 2 ** 232, "R mod l": R}
CANON = _dedupe(list(NAMED.values()) + [v for k in range(1, 9) for v in (2 ** (29 * k), 2 ** (29 * k) - 1)]
                + [v for k in range(1, 8) for v in (2 ** (32 * k), 2 ** (32 * k) - 1)])
NONCANON = (L, L + 1, 2 * L - 1, 2 ** 253 - 1, 2 ** 255, 2 ** 256 - 1)      # for the unpackers and from_canonical only
WORDS = CANON + NONCANON
assert all(v < L for v in CANON) and all(L <= v < 2 ** 256 for v in NONCANON) and len(CANON) == 41
CANON_PAIRS = tuple(itertools.product(CANON, CANON))             # 1681 lanes: seven workgroups, a ragged last wave
EDGE_CHALLENGES = (0, 1, L - 1, 2 ** 252 - 1)


def words(v):
    return int(v).to_bytes(32, "little")


# ------------------------------------------------------------------------------------------------ limb vectors
TOPS = (0x1fffffff, 0x20000000, 0x200fffff, 0x3fffffff, 0x40000000, 0x7fffffff, 0x80000000, 0xfff00000, 0xffefffff, 0xffffffff)   # limb9_check.cpp


def _hot(i, x):
    return tuple(x if k == i else 0 for k in range(9))


def _normalised_pool():
    rng = random.Random("scalar_cases normalised")
    out = [unpack_s(w, s) for s in (0, 5) for w in WORDS]
    out.append((M29,) * 9)
    out += [_hot(i, x) for x in (1, M29) for i in range(9)]
    for t in TOPS:
        out += [(M29,) * 8 + (t,), (0,) * 8 + (t,), tuple(rng.getrandbits(29) for _ in range(8)) + (t,)]
    out += [limbs_of(K * L - 2 ** 232 - 1) for K in KS]          # the largest subtrahend of fr9_sub_kl<K>
    out += [limbs_of(v) for v in (2 * L, 2 * L + 1, 3 * L - 1)]   # the ends of pack_lt2l and pack_lt3l (l, l + 1, 2l - 1 are unpacked words)
    out = _dedupe(out)
    assert all(normalised(v) for v in out)
    return out


def _loose_pool(bound, key):
    """all limbs at the bound, one limb at the bound (and one below it) in each position, seeded draws in which every second one pins half its limbs"""
    rng = random.Random("scalar_cases loose " + key)
    out = [(bound,) * 9, (bound - 1,) * 9]
    out += [_hot(i, x) for x in (bound, bound - 1) for i in range(9)]
    for n in range(12):
        v = [rng.randint(0, bound) for _ in range(9)]
        if n & 1:
            v = [bound if rng.getrandbits(1) else x for x in v]
        out.append(tuple(v))
    return _dedupe(out)


NORMALISED = _normalised_pool()
LOOSE_A = _loose_pool(B_A, "A")
LOOSE_B = _loose_pool(B_B, "B")
VECTORS = _dedupe(NORMALISED + LOOSE_A + LOOSE_B)
N29 = tuple(v for v in NORMALISED if v[8] <= M29)                # "all nine limbs below 2^29": the partner of a class-A operand
CLASS_A = LOOSE_A + tuple(v for v in NORMALISED if M29 < v[8] <= B_A)
CLASS_B = LOOSE_B + tuple(v for v in NORMALISED if M29 < v[8] <= B_B)


def _extremes():
    rng = random.Random("scalar_cases extremes")
    out = [(M29,) * 9, (0,) * 9, _hot(0, 1)]
    out += [unpack_s(w, s) for s in (0, 5) for w in (L - 1, 2 ** 252 - 1, 2 ** 256 - 1, R)]
    out += [_hot(i, M29) for i in range(9)]
    out += [tuple(rng.getrandbits(29) for _ in range(9)) for _ in range(4)]
    out = _dedupe(out)
    assert all(max(v) <= M29 for v in out)
    return out


N_EXTREME = _extremes()                                         # normalised, all limbs below 2^29


# ------------------------------------------------------------------------------------------------ preconditions, as fr9.h states them
def mul_class(a, b):
    """which operand class of fr9.h a pair is in: "NA" (a below 2^29, b <= B_A), "AN", "BB", or None"""
    if max(a) <= M29 and max(b) <= B_A:
        return "NA"
    if max(b) <= M29 and max(a) <= B_A:
        return "AN"
    if max(a) <= B_B and max(b) <= B_B:
        return "BB"
    return None


def _u32(v):
    return all(0 <= x < 2 ** 32 for x in v)


def _carries_fit(a):
    c = 0
    for i in range(8):
        c = (a[i] + c) >> 29
    return a[8] + c < 2 ** 32


def _sub_ok(K):
    o = kl_limbs(K)
    return lambda a, b: _u32(a) and normalised(b) and value(b) < K * L - 2 ** 232 and all(x + y < 2 ** 32 for x, y in zip(a, o))


PRECONDITION = {
    "unpack": lambda x: 0 <= x < 2 ** 256, "unpack5": lambda x: 0 <= x < 2 ** 256, "unpack10": lambda x: 0 <= x < 2 ** 253,
    "mul": lambda a, b: _u32(a) and _u32(b) and mul_class(a, b) is not None,
    "mul_self": lambda a: _u32(a) and mul_class(a, a) is not None,
    "add": lambda a, b: _u32(a) and _u32(b) and _u32(add(a, b)),
    "norm": lambda a: _u32(a) and _carries_fit(a),
    "fold_top": normalised, "canon": normalised,
    "shl5": lambda a: normalised(a) and value(a) < 2 ** 256,
    "pack_lt2l": lambda a: normalised(a) and value(a) < 2 * L,
    "pack_lt3l": lambda a: normalised(a) and value(a) < 3 * L,
    "mul9": lambda a, b: 0 <= a < L and 0 <= b < L,
    "fold9": lambda x0, x2, r: 0 <= x0 < L and 0 <= x2 < L and 0 <= r < L,
}
PRECONDITION.update({"sub_kl%d" % K: _sub_ok(K) for K in KS})
WORDS_IN = {"unpack": 1, "unpack5": 1, "unpack10": 1, "mul9": 2, "fold9": 3}   # operands that are words; every other operand is a limb vector
OPS = ("unpack", "unpack5", "unpack10", "mul", "mul_self", "add", "norm") + tuple("sub_kl%d" % K for K in KS) + (
    "fold_top", "shl5", "pack_lt2l", "pack_lt3l", "canon", "mul9", "fold9")


# ------------------------------------------------------------------------------------------------ the cases of every operation
def _mul_cases():
    out = [(a, b) for a in N_EXTREME for b in CLASS_A]                      # normalised x A ...
    out += [(b, a) for a in N_EXTREME for b in CLASS_A]                     # ... and A x normalised: the block reads its operands in another order
    out += list(itertools.product(CLASS_B, CLASS_B))                        # B x B
    for x, y in ((M29, M29), (M29, B_A), (B_A, M29), (B_B, B_B)):           # each of the 81 partial products alone
        out += [(_hot(i, x), _hot(j, y)) for i in range(9) for j in range(9)]
    out += [(unpack_s(a, 5), unpack_s(b, 0)) for a in WORDS for b in WORDS]  # pool pairs, in the operand forms the kernels feed
    return _dedupe(out)


def _sub_cases(K):
    o, top = kl_limbs(K), limbs_of(K * L - 2 ** 232 - 1)
    fits = lambda a: all(x + y < 2 ** 32 for x, y in zip(a, o))
    bs = [b for b in NORMALISED if value(b) < K * L - 2 ** 232]
    assert top in bs
    a_all = [a for a in VECTORS if fits(a)]
    a_ext = [a for a in N_EXTREME + (top, (B_B,) * 9, (2 ** 32 - 1 - max(o),) * 9) if fits(a)]
    b_ext = [b for b in (top, (0,) * 9, unpack_s(L - 1, 0), unpack_s(2 * L - 2 ** 232 - 1, 0)) if b in bs or b == (0,) * 9]
    out = [(a, b) for a in a_ext for b in bs] + [(a, b) for a in a_all for b in b_ext]
    if K == 128:                                                            # the shifted operands of the four-table cubic
        out += [(unpack_s(a, 5), unpack_s(b, 5)) for a, b in CANON_PAIRS]
    return _dedupe(out)


def _fold9_cases():
    ext = (0, 1, L - 1, 2 ** 252 - 1, L - 2 ** 232)
    rng = random.Random("scalar_cases fold9")
    out = list(itertools.product(ext, repeat=3))
    while len(out) < 1543:
        t = [rng.choice(CANON) for _ in range(3)]
        if len(out) & 1:
            t = [rng.choice(ext) if rng.getrandbits(1) else x for x in t]
        out.append(tuple(t))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases(op):
    """the operand tuples an operation runs on (integers for word operands, limb tuples for the others)"""
    if op in ("unpack", "unpack5"):
        return tuple((w,) for w in WORDS)
    if op == "unpack10":
        return tuple((w,) for w in WORDS if w < 2 ** 253)
    if op == "mul":
        return _mul_cases()
    if op == "mul_self":
        return tuple((a,) for a in _dedupe(N29 + CLASS_B))
    if op == "add":
        ext = N_EXTREME + ((B_B,) * 9, (B_A,) * 9, (2 ** 31,) * 9)
        return _dedupe((a, b) for a in ext for b in VECTORS if _u32(add(a, b)))
    if op == "norm":
        sums = [add(a, b) for a, b in cases("add")]
        return tuple((a,) for a in _dedupe(VECTORS + ((2 ** 32 - 8,) * 9,) + tuple(s for s in sums if _carries_fit(s))))
    if op.startswith("sub_kl"):
        return _sub_cases(int(op[6:]))
    if op in ("fold_top", "canon"):
        return tuple((a,) for a in NORMALISED)
    if op == "shl5":
        return tuple((a,) for a in NORMALISED if value(a) < 2 ** 256)
    if op == "pack_lt2l":
        return tuple((a,) for a in NORMALISED if value(a) < 2 * L)
    if op == "pack_lt3l":
        return tuple((a,) for a in NORMALISED if value(a) < 3 * L)
    if op == "mul9":
        return CANON_PAIRS
    if op == "fold9":
        return _fold9_cases()
    raise KeyError(op)


def expected(op, t):
    """(the word, the limbs) an operation returns for operands t; None for the output it does not produce"""
    if op in ("unpack", "unpack5", "unpack10"):
        return None, unpack_s(t[0], {"unpack": 0, "unpack5": 5, "unpack10": 10}[op])
    if op == "mul":
        return None, mul(t[0], t[1])
    if op == "mul_self":
        return None, mul(t[0], t[0])
    if op == "add":
        return None, add(t[0], t[1])
    if op == "norm":
        return None, norm(t[0])
    if op.startswith("sub_kl"):
        return None, sub_kl(int(op[6:]), t[0], t[1])
    if op == "fold_top":
        return None, fold_top(t[0])
    if op == "shl5":
        return None, shl5(t[0])
    if op in ("pack_lt2l", "pack_lt3l", "canon"):
        return value(t[0]) % L, None
    if op == "mul9":
        return t[0] * t[1] * RINV % L, mul(unpack_s(t[0], 5), unpack_s(t[1], 0))
    if op == "fold9":
        x0, x2, r = t
        return (x0 + r * (x2 - x0) * RINV) % L, fold9(x0, x2, r)
    raise KeyError(op)


@functools.lru_cache(maxsize=None)
def expected_all(op):
    return tuple(expected(op, t) for t in cases(op))


# ------------------------------------------------------------------------------------------------ the case file of tests/limb9_check.cpp
def _hex_word(v):
    return " ".join("%x" % ((v >> (32 * i)) & 0xffffffff) for i in range(8))


def _hex_limbs(v):
    return " ".join("%x" % x for x in v)


def write_case_file(path):
    """one case per line: the operation, its operands, the expected word (if it has one), the expected limbs (if it has them); a word is eight
    32-bit hex words from the low end, a limb vector nine.  Returns the number of lines."""
    n = 0
    with open(path, "w") as f:
        for op in OPS:
            nw = WORDS_IN.get(op, 0)
            for t, (w, l) in zip(cases(op), expected_all(op)):
                cols = [op] + [_hex_word(x) if k < nw else _hex_limbs(x) for k, x in enumerate(t)]
                if w is not None:
                    cols.append(_hex_word(w))
                if l is not None:
                    cols.append(_hex_limbs(l))
                f.write(" ".join(cols) + "\n"); n += 1
    return n
