"""GF(2^255-19) on the device against plain big integers (curve_cases.py; shown right on the host by test_curve_cases_host.py): the three forms of a
field element (field.h Fp, fp9.h F9 with its generated asm product, fp10.h F10), the point formulas built on them (p9_madd, p10_madd, p10_add, the
quad-lane forms), RFC 9496 encode (k_encode_points) and decode (k_decode_niels) — through otti_k_fp_op / otti_k_pt_op, which call the very inline
functions the MSM kernels call.  The operands are the ones an MSM over hashed generators and uniform scalars never meets: limbs at their bounds,
non-canonical words, zero coordinates, P + P, P + (-P), the identity, the 4-torsion.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import otti_amd as oa
import orc
import curve_cases as cc

pytestmark = pytest.mark.gpu
K, P = oa.kernels, cc.P
REDUCED_OUT = ("mul", "sqr", "carry", "repack", "mul_sub_add", "mul_3a_2b", "mul_f_e", "mul_carried_f_g", "pow22523")   # fp9.h / fp10.h: "output of mul/sqr/carry/unpack"


def arr(vals, width=1):
    """integers below 2^256, `width` per row -> (n, 32 * width) uint8"""
    vals = list(vals)
    return np.frombuffer(b"".join(cc.words(v) for v in vals), dtype=np.uint8).reshape(-1, 32 * width).copy()


def rows(tuples):
    tuples = list(tuples)
    return arr([v for t in tuples for v in t], len(tuples[0]))


def ints(a):
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32)
    return [int.from_bytes(r.tobytes(), "little") for r in a]


def tuples_of(a, width):
    v = ints(a)
    return [tuple(v[i:i + width]) for i in range(0, len(v), width)]


def check_limbs(form, limbs, want, reduced=True):
    """raw limbs of one field element per row: they stand for the expected value, and satisfy the header's "reduced" bound"""
    F = cc.FORMS[form]
    for l, w in zip(limbs.tolist(), want):
        assert F.value(l) % P == w % P, (form, l, w)
        assert not reduced or F.reduced(l), (form, l)


# ------------------------------------------------------------------------------------------------ field operations, every form
@pytest.mark.parametrize("form,op", [(f, o) for f in K.FP_FORMS for o in cc.FORM_OPS[f]])
def test_field_op_equals_the_integers_mod_p(form, op):
    """one launch per operation: the pool (50 lanes), all its pairs (2500 lanes, ten workgroups) or the sampled quadruples (1031 lanes)"""
    cases = cc.op_cases(op)
    got, limbs = K.fp_op(form, op, *(arr(t[k] for t in cases) for k in range(4)))
    want = [cc.fp_ref(op, t) for t in cases]
    got = ints(got)
    for t, g, w in zip(cases, got, want):
        assert g % P == w, (form, op, [hex(v) for v in t], hex(g), hex(w))
    if form == "fp8":
        assert ints(limbs.astype("<u4").view(np.uint8)) == got       # the saturated form's "limbs" are its words
        if op in ("carry", "repack"):
            assert got == want                                       # fp_canon, fp_to_bytes: THE representative below p
    else:
        check_limbs(form, limbs, want, reduced=op in REDUCED_OUT)


def test_unsupported_operations_are_refused():
    a = arr([1])
    for op in ("sqr", "pow22523", "mul_f_e"):
        with pytest.raises(oa.SpartanError):
            K.fp_op("f9", op, a)


# ------------------------------------------------------------------------------------------------ the formulas on arbitrary field elements
def check_points(form, got, limbs, want):
    for g, w in zip(tuples_of(got, 4), want):
        assert tuple(v % P for v in g) == tuple(w), ([hex(v) for v in g], [hex(v) for v in w])
    for k in range(4):
        check_limbs(form, limbs[:, k, :], [w[k] for w in want])


@pytest.mark.parametrize("neg", [False, True])
@pytest.mark.parametrize("op,form", [("p9_madd", "f9"), ("p10_madd", "f10"), ("q10_madd", "f10")])
def test_mixed_addition_formula_on_pool_tuples(op, form, neg):
    """(X, Y, Z, T) and (y+x, y-x, 2dxy) are ANY pool values: the formulas are polynomial maps, every output coordinate must equal the map's mod p"""
    t = cc.MADD_TUPLES
    got, limbs = K.pt_op(op, rows(x[:4] for x in t), rows(x[4:] for x in t), neg=neg)
    check_points(form, got, limbs, [cc.madd_ref(x[:4], x[4:], neg) for x in t])


@pytest.mark.parametrize("op", ["p10_add", "q10_add"])
def test_full_addition_formula_on_pool_tuples(op):
    t = cc.ADD_TUPLES
    got, limbs = K.pt_op(op, rows(x[:4] for x in t), rows(x[4:] for x in t))
    check_points("f10", got, limbs, [cc.add_ref(x[:4], x[4:]) for x in t])


# ------------------------------------------------------------------------------------------------ the group
@functools.lru_cache(maxsize=None)
def gens():
    """the oracle's generator stream for R = 16 (18 points), decoded by the reference"""
    out = []
    for row in orc.OGens(256, 256, 1).points():
        pt, why = cc.rist_decode(row.tobytes())
        assert why is None
        out.append(pt)
    return tuple(out)


SCALES = tuple(v for v in cc.POOL if v % P)                       # projective scalings: every pool value that is not zero mod p, the non-canonical ones too


@functools.lru_cache(maxsize=None)
def group_cases():
    """(A, B, scale of A, scale of B, lift): O + O, O + P, P + O, P + P, P + (-P), P + Q, and every one of E[4] on either side"""
    G = gens()
    pairs = []
    for i in range(0, len(G), 3):
        p, q = G[i], G[(i + 1) % len(G)]
        pairs += [(cc.O, cc.O), (cc.O, p), (p, cc.O), (p, p), (p, cc.aff_neg(p)), (p, q), (cc.aff_neg(q), p)]
        for t in cc.TORSION4:
            pairs += [(p, t), (t, p), (t, cc.TORSION4[2]), (cc.aff_add(p, t), cc.aff_neg(p))]
    out = []
    for k, (a, b) in enumerate(pairs):
        out.append((a, b, 1, 1, False))                            # Z = 1
        out.append((a, b, SCALES[(5 * k + 1) % len(SCALES)], SCALES[(7 * k + 3) % len(SCALES)], bool(k & 1)))
    return tuple(out)


def check_projective(got, want_affine):
    for g, w in zip(tuples_of(got, 4), want_affine):
        X, Y, Z, T = (v % P for v in g)
        assert Z != 0 and (T * Z - X * Y) % P == 0, g
        assert (X * cc.inv(Z) % P, Y * cc.inv(Z) % P) == w, (g, w)


@pytest.mark.parametrize("neg", [False, True])
@pytest.mark.parametrize("op", ["p9_madd", "p10_madd", "q10_madd"])
def test_mixed_addition_on_points(op, neg):
    c = group_cases()
    Pa = rows(cc.extended(a, sa, lift) for a, b, sa, sb, lift in c)
    Q = rows(cc.niels(b) if b != cc.O else cc.NIELS_IDENTITY for a, b, sa, sb, lift in c)
    got, _ = K.pt_op(op, Pa, Q, neg=neg)
    check_projective(got, [cc.aff_add(a, cc.aff_neg(b) if neg else b) for a, b, *_ in c])
    enc = K.pt_op("encode", got)                                   # whatever representation the formula left, the encoding is the sum's
    assert [e.tobytes() for e in enc] == [cc.rist_encode(cc.extended(cc.aff_add(a, cc.aff_neg(b) if neg else b))) for a, b, *_ in c]


@pytest.mark.parametrize("op", ["p10_add", "q10_add"])
def test_full_addition_on_points(op):
    c = group_cases()
    Pa, Q = rows(cc.extended(a, sa, lift) for a, b, sa, sb, lift in c), rows(cc.extended(b, sb, not lift) for a, b, sa, sb, lift in c)
    got, _ = K.pt_op(op, Pa, Q)
    check_projective(got, [cc.aff_add(a, b) for a, b, *_ in c])
    assert [e.tobytes() for e in K.pt_op("encode", got)] == [cc.rist_encode(cc.extended(cc.aff_add(a, b))) for a, b, *_ in c]


@pytest.mark.parametrize("k", [1, 2, 64, 300])
def test_chain_of_mixed_additions_is_k_times_the_point(k):
    """k successive p9_madd of one entry: reduced in, reduced out, all the way; from the identity (the first step is O + P, the second P + P), from
    another point in a non-trivial scaling, and with the entry negated"""
    G = gens()
    for neg in (False, True):
        starts = [(cc.O, 1)] * len(G) + [(G[(i + 5) % len(G)], SCALES[(3 * i + 2) % len(SCALES)]) for i in range(len(G))] + [(G[i], 2 ** 255 + 18) for i in range(len(G))]
        entries = list(G) * 3
        got, limbs = K.pt_op("chain", rows(cc.extended(a, s, True) for a, s in starts), rows(cc.niels(q) for q in entries), neg=neg, k=k)
        want = [cc.aff_add(a, cc.aff_mul(k, cc.aff_neg(q) if neg else q)) for (a, s), q in zip(starts, entries)]
        check_projective(got, want)
        assert all(cc.F9.reduced(l) for l in limbs.reshape(-1, 9).tolist())


# ------------------------------------------------------------------------------------------------ encode
def test_encode_equals_the_reference_in_every_scaling_and_coset():
    G = gens()
    pts, want = [], []
    for i, p in enumerate(G):
        e = cc.rist_encode(cc.extended(p))
        for j, t in enumerate(cc.TORSION4):                        # encode(P + T) == encode(P): the rotate branch and both sign flips
            s = cc.aff_add(p, t)
            for scale, lift in ((1, False), (SCALES[(4 * i + j) % len(SCALES)], True), (P - 1, False)):
                pts.append(cc.extended(s, scale, lift)); want.append(e)
    for scale in SCALES:                                           # the identity, and its coset, in any projective scaling: 32 zero bytes
        for t in cc.TORSION4:
            pts.append(cc.extended(t, scale, bool(scale & 2))); want.append(bytes(32))
    assert len(pts) % 64 and len(pts) > 64
    got = K.pt_op("encode", rows(pts))
    assert [g.tobytes() for g in got] == want
    assert want == [cc.rist_encode(p) for p in pts]


def test_encode_with_addend_is_the_encoding_of_the_sum():
    c = group_cases()
    Pa, Q = rows(cc.extended(a, sa, lift) for a, b, sa, sb, lift in c), rows(cc.extended(b, sb, not lift) for a, b, sa, sb, lift in c)
    got = K.pt_op("encode", Pa, Q)
    assert [g.tobytes() for g in got] == [cc.rist_encode(cc.extended(cc.aff_add(a, b))) for a, b, *_ in c]
    zero = [i for i, (a, b, *_) in enumerate(c) if cc.aff_mul(4, cc.aff_add(a, b)) == cc.O]
    assert len(zero) >= 8 and all(got[i].tobytes() == bytes(32) for i in zero)     # P + (-P), O + O, T + T': the identity's coset


# ------------------------------------------------------------------------------------------------ decode
def check_niels(got_row, want3):
    assert tuple(v % P for v in tuples_of(got_row, 3)[0]) == tuple(v % P for v in want3)


def test_decode_equals_the_reference_and_refuses_by_every_rule():
    G = gens()
    valid = [cc.rist_encode(cc.extended(p)) for p in G] + [cc.rist_encode(cc.extended(cc.aff_neg(p))) for p in G] + [bytes(32)]
    valid += [cc.rist_encode(cc.extended(cc.aff_mul(k, G[k % len(G)]), SCALES[k % len(SCALES)])) for k in range(2, 42)]
    refused = cc.refused_encodings()
    enc = list(valid)
    where = {}
    for j, (why, b) in enumerate(refused.items()):                 # spread over both workgroups of the launch
        where[why] = 3 + 17 * j; enc.insert(where[why], b)
    assert len(enc) > 64 and len(enc) % 64
    out, bad = K.pt_op("decode", np.frombuffer(b"".join(enc), dtype=np.uint8).reshape(-1, 32))
    assert bad == len(refused) == 5
    for i, b in enumerate(enc):
        pt, why = cc.rist_decode(b)
        check_niels(out[i], cc.NIELS_IDENTITY if why else (cc.niels(pt) if pt != cc.O else cc.NIELS_IDENTITY))
        assert (why is not None) == (i in where.values())
    assert cc.rist_decode(valid[0])[0] == G[0]
    for why, b in refused.items():                                 # each rule on its own raises the count by one
        one = valid[:5] + [b] + valid[5:9]
        out, bad = K.pt_op("decode", np.frombuffer(b"".join(one), dtype=np.uint8).reshape(-1, 32))
        assert bad == 1, why
        check_niels(out[5], cc.NIELS_IDENTITY)
        check_niels(out[6], cc.niels(cc.rist_decode(one[6])[0]))
    out, bad = K.pt_op("decode", np.frombuffer(b"".join(valid), dtype=np.uint8).reshape(-1, 32))
    assert bad == 0
