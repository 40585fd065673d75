"""GF(l) on the device against plain big integers (scalar_cases.py; shown right on the host by test_scalar_cases_host.py): the nine-limb form of
fr9.h with its generated asm product (fr9_mul_gfx950.inc), through otti_k_fr9_op, which calls the very inline functions the sum-check, eq-table and
sparse kernels call; the eight-word Montgomery form of field.h (fr_mul's generated asm, fr_add, fr_sub, the conditional subtraction) through
otti_k_fr_op and the two conversions; and the eq tables at edge challenges.  The operands are the ones that stored words and uniform challenges
never bring: limbs at the ends of the ranges fr9.h states (normalised, the two loose classes of the product, the largest subtrahend of each
a - b + K l, a top limb up to 2^32 - 1), one partial product alone, non-canonical words.  Every comparison is exact."""
import random

import numpy as np
import pytest

import otti_amd as oa
import orc
import scalar_cases as sc

pytestmark = pytest.mark.gpu
K, L = oa.kernels, sc.L


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def warr(vals):
    """integers below 2^256 -> (n, 32) uint8"""
    return np.frombuffer(b"".join(sc.words(v) for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def ints(a):
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32)
    return [int.from_bytes(r.tobytes(), "little") for r in a]


def run(op):
    """one launch over all cases of an operation: (cases, device words as integers, device limbs as tuples, expected (word, limbs) per case)"""
    cases = sc.cases(op)
    nw = sc.WORDS_IN.get(op, 0)
    operands = [warr(t[k] for t in cases) if k < nw else np.array([t[k] for t in cases], dtype=np.uint32) for k in range(len(cases[0]))]
    assert list(K.FR9_OPS) == list(sc.OPS)
    w, l = K.fr9_op(op, *operands)
    assert w.shape == (len(cases), 32) and l.shape == (len(cases), 9)
    return cases, ints(w), [tuple(r) for r in l.tolist()], sc.expected_all(op)


def check_expected(op, cases, words, limbs, want):
    for t, w, l, (ww, wl) in zip(cases, words, limbs, want):
        assert w == (0 if ww is None else ww), (op, t, hex(w), ww)         # an output the operation does not produce is zero
        assert l == ((0,) * 9 if wl is None else wl), (op, t, l, wl)


# ------------------------------------------------------------------------------------------------ nine limbs, operation by operation
@pytest.mark.parametrize("op,shift", [("unpack", 0), ("unpack5", 5), ("unpack10", 10)])
def test_unpack_gives_the_limbs_of_the_shifted_word(op, shift):
    cases, words, limbs, want = run(op)
    check_expected(op, cases, words, limbs, want)
    for (x,), l in zip(cases, limbs):
        assert sc.value(l) == x << shift and sc.normalised(l)


@pytest.mark.parametrize("op", ["mul", "mul_self"])
def test_product_equals_the_integers_and_the_c_body_limb_for_limb(op):
    """normalised x A, A x normalised, B x B, each partial product alone, pool pairs (6626 lanes); the same registers as both operands (155)"""
    cases, words, limbs, want = run(op)
    for t, r in zip(cases, limbs):
        a, b = (t[0], t[-1])
        va, vb, vr = sc.value(a), sc.value(b), sc.value(r)
        assert all(x <= sc.M29 for x in r[:8]), (op, a, b, r)
        assert vr * 2 ** 261 % L == va * vb % L, (op, a, b, r)
        assert vr < va * vb // 2 ** 261 + L + 1, (op, a, b, r)
    check_expected(op, cases, words, limbs, want)


def test_add_is_limb_wise():
    cases, words, limbs, want = run("add")
    check_expected("add", cases, words, limbs, want)
    for (a, b), r in zip(cases, limbs):
        assert r == tuple(x + y for x, y in zip(a, b))


def test_norm_keeps_the_value_and_brings_the_low_limbs_below_2_29():
    cases, words, limbs, want = run("norm")
    for (a,), r in zip(cases, limbs):
        assert sc.value(r) == sc.value(a) and all(x <= sc.M29 for x in r[:8]), (a, r)
    check_expected("norm", cases, words, limbs, want)


@pytest.mark.parametrize("k", sc.KS)
def test_difference_plus_k_l_never_borrows(k):
    op = "sub_kl%d" % k
    cases, words, limbs, want = run(op)
    for (a, b), r in zip(cases, limbs):
        assert sc.value(r) == sc.value(a) - sc.value(b) + k * L, (k, a, b, r)
        assert all(x == y + o - z for x, y, z, o in zip(r, a, b, sc.kl_limbs(k))), (k, a, b, r)   # 0 <= each limb, no wrap: the integers' own
    check_expected(op, cases, words, limbs, want)


def test_fold_top_brings_any_normalised_value_into_0_2l():
    cases, words, limbs, want = run("fold_top")
    for (a,), r in zip(cases, limbs):
        assert sc.normalised(r) and r[8] <= sc.M29 and sc.value(r) % L == sc.value(a) % L and 0 < sc.value(r) < 2 * L, (a, r)
    check_expected("fold_top", cases, words, limbs, want)


def test_shl5_gives_the_limbs_of_32_x():
    cases, words, limbs, want = run("shl5")
    for (a,), r in zip(cases, limbs):
        assert sc.value(r) == 32 * sc.value(a) and sc.normalised(r), (a, r)
    check_expected("shl5", cases, words, limbs, want)


@pytest.mark.parametrize("op", ["pack_lt2l", "pack_lt3l", "canon"])
def test_pack_gives_the_canonical_word(op):
    cases, words, limbs, want = run(op)
    for (a,), w in zip(cases, words):
        assert w == sc.value(a) % L, (op, a, hex(w))
    check_expected(op, cases, words, limbs, want)


def test_mul9_is_the_product_in_the_memory_format():
    """fr9_pack_lt2l(fr9_mul(fr9_unpack5(a), fr9_unpack(b))) on all pairs of the canonical pool: the form of eq_mul9, mul9 and the sparse products"""
    cases, words, limbs, want = run("mul9")
    for (a, b), w, l in zip(cases, words, limbs):
        assert w == a * b * sc.RINV % L, (hex(a), hex(b), hex(w))
        assert sc.normalised(l) and sc.value(l) < 2 * L and sc.value(l) % L == w
    check_expected("mul9", cases, words, limbs, want)


def test_fold9_is_x0_plus_r_times_x2_minus_x0():
    cases, words, limbs, want = run("fold9")
    for (x0, x2, r), w, l in zip(cases, words, limbs):
        assert w == (x0 + r * (x2 - x0) * sc.RINV) % L, (hex(x0), hex(x2), hex(r), hex(w))
        assert sc.normalised(l) and sc.value(l) < 3 * L and sc.value(l) % L == w
    check_expected("fold9", cases, words, limbs, want)


def test_entry_refuses_what_it_cannot_run():
    a, l = warr([1]), np.ones((1, 9), dtype=np.uint32)
    w, lm = K.fr9_op("unpack", warr([]))                                    # n = 0 returns at once
    assert w.shape == (0, 32) and lm.shape == (0, 9)
    for bad in (lambda: K.fr9_op("mul", l), lambda: K.fr9_op("unpack", a, a), lambda: K.fr9_op("mul", a, a), lambda: K.fr9_op("fold9", a, a, l)):
        with pytest.raises(ValueError):
            bad()
    out, limbs = np.zeros((1, 32), dtype=np.uint8), np.zeros((1, 9), dtype=np.uint32)
    p = lambda x: x.ctypes.data
    assert oa.api.lib.otti_k_fr9_op(len(K.FR9_OPS), p(a), p(a), p(a), 1, p(out), p(limbs), None) == oa.api.lib.otti_k_fr9_op(-1, p(a), p(a), p(a), 1, p(out), p(limbs), None) != 0
    assert oa.api.lib.otti_k_fr9_op(0, p(a), None, p(a), 1, p(out), p(limbs), None) != 0
    assert oa.api.lib.otti_k_fr9_op(0, p(a), p(a), p(a), 1, None, p(limbs), None) != 0
    assert not out.any() and not limbs.any()
    assert oa.api.lib.otti_k_fr9_op(0, None, None, None, 0, None, None, None) == 0


# ------------------------------------------------------------------------------------------------ eight words
def test_eight_word_ops_on_all_pairs_of_the_canonical_pool():
    """fr_mul, fr_add, fr_sub, the pool read twice: as stored words (every canonical word is a Montgomery-form element: a b / R, a + b, a - b
    mod l on the words themselves) and as values (x y, x + y, x - y mod l through the Montgomery form)"""
    xs, ys = [p[0] for p in sc.CANON_PAIRS], [p[1] for p in sc.CANON_PAIRS]
    a, b, am, bm = warr(xs), warr(ys), orc.fr_from_ints(xs), orc.fr_from_ints(ys)
    for op, f in (("mul", lambda x, y: x * y), ("add", lambda x, y: x + y), ("sub", lambda x, y: x - y)):
        got = ints(K.fr_op(op, a, b)[0])
        for x, y, g in zip(xs, ys, got):
            assert g == f(x, y) * (sc.RINV if op == "mul" else 1) % L, (op, hex(x), hex(y), hex(g))
        assert orc.fr_to_ints(K.fr_op(op, am, bm)[0]) == [f(x, y) % L for x, y in zip(xs, ys)], op


def test_conversions_on_the_whole_word_pool():
    got = ints(K.from_canonical(warr(sc.WORDS)))                            # non-canonical words included: the word mod l, in Montgomery form
    assert got == [w * sc.R % L for w in sc.WORDS]
    mont = [w * sc.R % L for w in sc.CANON]
    assert ints(K.to_canonical(warr(mont))) == list(sc.CANON)
    assert ints(K.to_canonical(warr(sc.CANON))) == [w * sc.RINV % L for w in sc.CANON]   # the pool's own words as stored elements


# ------------------------------------------------------------------------------------------------ eq tables at edge challenges
def _eq_ref(r):
    """eq(r, .) over integers: index bit (ell - 1 - k) selects r_k or 1 - r_k"""
    out = [1]
    for x in r:
        out = [v * f % L for v in out for f in ((1 - x) % L, x)]
    return out


@pytest.mark.parametrize("ell", [1, 6, 7, 12, 13, 14])
def test_eq_tables_at_edge_challenges(ell):
    """every challenge from {0, 1, l - 1, 2^252 - 1}, as a value and as a stored word; all-0 and all-1 included; both sides of the 12-variable split"""
    rng = random.Random("eq edge %d" % ell)
    E = sc.EDGE_CHALLENGES
    draws = [[0] * ell, [1] * ell, [rng.choice((0, 1)) for _ in range(ell)]] + [[rng.choice(E) for _ in range(ell)] for _ in range(3 if ell < 13 else 2)]
    one = sc.R
    for n, vals in enumerate(draws):
        for stored in (False, True):
            r = warr(vals) if stored else orc.fr_from_ints(vals)            # a stored word w is the element w / R
            want = orc.eq_evals(r)
            got, _ = K.eq_evals(r)
            assert np.array_equal(got, want), (ell, vals, stored)
            if ell <= 7:                                                    # the oracle itself against the integers, where that is quick
                elems = [v * sc.RINV % L for v in vals] if stored else vals
                assert ints(want) == [v * sc.R % L for v in _eq_ref(elems)]
            m = min(ell, 13)                                                # a pyramid has at most 13 levels: of 14 challenges, the last 13
            pyr = K.eq_pyramid(r[ell - m:])
            for k in range(m + 1):                                          # level k: eq over the LAST k variables
                lvl = want if k == ell else orc.eq_evals(r[ell - k:])
                assert np.array_equal(pyr[(1 << k) - 1: (2 << k) - 1], lvl), (ell, vals, stored, k)
            if n < 3 and not stored:                                        # challenges in {0, 1}: an indicator
                hot = int("".join(str(v) for v in vals), 2)
                g = ints(got)
                assert g[hot] == one and not any(g[:hot]) and not any(g[hot + 1:]), (ell, vals)
