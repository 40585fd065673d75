"""The operands and the reference of the device's GF(2^255-19) tests (curve_cases.py), shown right without a GPU: the big-integer group arithmetic
and RFC 9496 encode / decode against the golden primitives and the oracle's generator stream, the restated limb forms against the integers they
stand for, and every case against the precondition its header (fp9.h, fp10.h) states for each product it reaches.

Which bound "within a factor 2" is measured against.  f9_mul wants 9 * max f * max g < 2^63.9, f10_mul f < 2^28.1 and g < 2^27.7.  A formula does
not offer every product operands that large: fp9.h's own limb line gives E < 3 * 2^29 and a carried F < 2^29, so E * F can never load the
multiplier beyond 2^62.8.  So each product is held against the product of the bounds the header's reasoning gives ITS two operands (BoundForm:
every unpacked, carried or multiplied value "reduced" as the header defines it, sums and a - b + 2p on top of that), that bound itself is checked
against the multiplier's precondition, and per formula the tightest product must come within a factor 2 of the multiplier's stated bound."""
import json
import os

import numpy as np
import pytest

import orc
import curve_cases as cc

P = cc.P
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "primitives.json")))


def _dec(hexstr):
    pt, why = cc.rist_decode(bytes.fromhex(hexstr))
    assert why is None, why
    return pt


def _enc(pt, scale=1):
    return cc.rist_encode(cc.extended(pt, scale)).hex()


def test_constants_and_pool():
    assert cc.SQRT_M1 * cc.SQRT_M1 % P == P - 1 and not cc.is_neg(cc.SQRT_M1)
    assert cc.INVSQRT_A_MINUS_D ** 2 * (-1 - cc.D) % P == 1
    assert cc.L == orc.L_ORDER
    for name in ("0", "1", "2", "19", "p-1", "p", "p+1", "2^255-1", "2^255", "2^255+18", "2p", "2^256-1", "(p-1)/2", "d", "2d", "sqrt(-1)"):
        assert cc.NAMED[name] in cc.POOL
    for k in range(1, 9):
        assert 2 ** (29 * k) in cc.POOL and 2 ** (29 * k) - 1 in cc.POOL
    for s in (26, 51, 77, 102, 128, 153, 179, 204, 230):
        assert 2 ** s in cc.POOL and 2 ** s - 1 in cc.POOL
    assert len(cc.BINARY) == len(cc.POOL) ** 2 and len(set(cc.POOL)) == len(cc.POOL)
    for tuples, width in ((cc.QUADS, 4), (cc.MADD_TUPLES, 7), (cc.ADD_TUPLES, 8)):
        for e in (2 ** 256 - 1, 2 ** 255 - 1, P - 1):
            assert (e,) * width in tuples
        assert len(tuples) % 64 and len(tuples) % 256 and len(tuples) > 256   # a ragged last wave, more than one workgroup
    assert len(cc.BINARY) % 64 and len(cc.POOL) % 64
    assert all(cc.on_curve(t) for t in cc.TORSION4)
    assert all(cc.aff_mul(4, t) == cc.O for t in cc.TORSION4) and len(set(cc.TORSION4)) == 4


def test_group_reference_equals_the_golden_primitives():
    for g in GOLDEN["point_add"]:
        a, b = _dec(g["a"]), _dec(g["b"])
        assert cc.on_curve(a) and cc.on_curve(b)
        assert _enc(cc.aff_add(a, b)) == g["out"]
        # the same sum through the formulas (as polynomial maps), mixed and full, and in another projective scaling
        assert cc.rist_encode(cc.add_ref(cc.extended(a, 5), cc.extended(b, P - 3))).hex() == g["out"]
        assert cc.rist_encode(cc.madd_ref(cc.extended(a, 7), cc.niels(b))).hex() == g["out"]
        assert cc.rist_encode(cc.madd_ref(cc.madd_ref(cc.extended(a), cc.niels(b)), cc.niels(b), neg=True)).hex() == g["a"]
    for g in GOLDEN["scalarmul"]:
        k = int.from_bytes(bytes.fromhex(g["scalar"]), "little")
        assert _enc(cc.aff_mul(k, _dec(g["point"]))) == g["out"]


def test_from_uniform_bytes_outputs_decode_and_encode_back():
    """the golden one-way map's outputs: valid encodings, decode then encode is the identity, in any projective scaling and for every coset member"""
    for g in GOLDEN["from_uniform_bytes"]:
        pt = _dec(g["out"])
        assert cc.on_curve(pt)
        for scale in (1, 2, P - 1, cc.SQRT_M1):
            assert _enc(pt, scale) == g["out"]
        for t in cc.TORSION4:
            assert _enc(cc.aff_add(pt, t)) == g["out"]


def test_decode_then_encode_is_the_identity_on_the_oracles_generators():
    og = orc.OGens(256, 256, 1)
    pts = og.points()
    assert pts.shape[0] == og.R + 2 == 18
    for row in pts:
        pt = _dec(row.tobytes().hex())
        assert cc.on_curve(pt) and _enc(pt) == row.tobytes().hex() and _enc(cc.aff_neg(pt)) != row.tobytes().hex()
    assert cc.rist_encode((0, 1, 1, 0)) == bytes(32) and cc.rist_decode(bytes(32)) == (cc.O, None)
    assert cc.rist_encode((0, 5, 5, 0)) == bytes(32)


def test_one_refused_encoding_per_rule():
    r = cc.refused_encodings()
    assert tuple(sorted(r)) == tuple(sorted(cc.DECODE_RULES)) and len(set(r.values())) == 5
    for why, b in r.items():
        assert cc.rist_decode(b) == (None, why)


@pytest.mark.parametrize("form", ["f9", "f10"])
def test_restated_limbs_stand_for_the_value(form):
    """unpack / add / sub / carry / product on limbs against plain integers mod p, on every pair of the pool; unpack and product outputs are reduced"""
    F = cc.FORMS[form]
    for v in cc.POOL:
        l = F.unpack(v)
        assert F.value(l) % P == v % P and F.reduced(l)
        assert F.value(F.carry(F.sub([0] * F.n, l))) % P == -v % P
    for a, b in cc.BINARY:
        x, y = F.unpack(a), F.unpack(b)
        assert F.value(F.add(x, y)) % P == (a + b) % P and F.value(F.sub(x, y)) % P == (a - b) % P
        m = F.mul(x, y)
        assert F.value(m) % P == a * b % P and F.reduced(m)
        assert F.reduced(F.carry(F.add(F.sub(x, y), F.add(x, y))))


def _run_cases(form, which):
    """(the record over all cases, the record over the header's limb bounds) of one operation or formula"""
    F = cc.FORMS[form]
    rec, bound = cc.Products(F), cc.Products(cc.BoundForm(F))
    B = bound.form
    if which in cc.FP_OPS:
        for t in cc.op_cases(which):
            r = cc.limbs_fp_op(rec, which, t)
            assert F.value(r) % P == cc.fp_ref(which, t), (which, t)
            if which in ("mul", "sqr", "carry", "repack", "mul_sub_add", "mul_3a_2b", "mul_f_e", "mul_carried_f_g"):
                assert F.reduced(r)
        cc.limbs_fp_op(bound, which, (0, 0, 0, 0))
    elif which in ("madd", "madd_neg", "chain"):
        neg = which == "madd_neg"
        for t in cc.MADD_TUPLES:
            p4, n3 = [F.unpack(v) for v in t[:4]], cc.limbs_niels(rec, t[4:], neg)
            want = tuple(t[:4])
            for _ in range(3 if which == "chain" else 1):          # reduced out is reduced in: the contract holds through a chain
                p4 = cc.limbs_madd(rec, p4, n3); want = cc.madd_ref(want, t[4:], neg)
                assert all(F.reduced(x) for x in p4)
                assert tuple(F.value(x) % P for x in p4) == want
        cc.limbs_madd(bound, [B.unpack(0)] * 4, cc.limbs_niels(bound, (0, 0, 0), neg))
    else:
        assert which == "padd" and form == "f10"
        for t in cc.ADD_TUPLES:
            r = cc.limbs_add10(rec, [F.unpack(v) for v in t[:4]], [F.unpack(v) for v in t[4:]])
            assert all(F.reduced(x) for x in r) and tuple(F.value(x) % P for x in r) == cc.add_ref(t[:4], t[4:])
        cc.limbs_add10(bound, [B.unpack(0)] * 4, [B.unpack(0)] * 4)
    return rec, bound


def product_report(form, which):
    """per product: (cases, largest max f * max g reached, the header-reasoned bound of max f * max g, load of the multiplier's own bound reached)"""
    rec, bound = _run_cases(form, which)
    return rec, bound, {k: (rec.count[k], rec.maxfg[k], bound.maxfg[k], rec.load[k]) for k in rec.maxfg}


FORMULAS = [("f9", "madd"), ("f9", "madd_neg"), ("f9", "chain"), ("f10", "madd"), ("f10", "madd_neg"), ("f10", "padd")]
# the formulas, and the compounds the headers name as their own extreme: fp9.h's 2^30 x 3 * 2^29, fp10.h's f < 2^28 times e < 2^27.6
AT_THE_MULTIPLIERS_BOUND = FORMULAS + [("f9", "mul_3a_2b"), ("f9", "mul_sub_add"), ("f10", "mul_f_e")]
COMPOUND = [(f, o) for f in ("f9", "f10") for o in cc.FORM_OPS[f] if o.startswith("mul") or o == "sqr"]


@pytest.mark.parametrize("form,which", FORMULAS + COMPOUND)
def test_every_case_is_within_contract_and_some_case_is_at_the_bound(form, which):
    rec, bound, rep = product_report(form, which)
    assert not bound.bad, bound.bad                               # the header's reasoning: operands at their bounds satisfy the multiplier
    assert not rec.bad, rec.bad[:5]                               # every case satisfies it, computed from its own limbs
    assert set(rep) == set(bound.maxfg)
    for name, (count, got, limit, load) in rep.items():
        assert count >= len(cc.POOL) and got <= limit, (name, got, limit)
        assert 2 * got >= limit, (name, got / limit)              # some case brings the operands within a factor 2 of what the header allows them
    if (form, which) in AT_THE_MULTIPLIERS_BOUND:                 # ... and the tightest product within a factor 2 of the multiplier's own bound
        assert max(v[3] for v in rep.values()) >= 0.5, rep


def test_arrays_for_the_device_are_what_the_cases_say():
    a = np.frombuffer(b"".join(cc.words(v) for v in cc.POOL), dtype=np.uint8).reshape(-1, 32)
    assert [int.from_bytes(r.tobytes(), "little") for r in a] == list(cc.POOL)


if __name__ == "__main__":                                     # the table behind the assertions above: python tests/test_curve_cases_host.py
    import math
    for _form, _which in FORMULAS + COMPOUND:
        for _name, (_n, _got, _limit, _load) in product_report(_form, _which)[2].items():
            print(f"{_form:4s} {_which:16s} {_name:20s} cases {_n:5d}  max f x max g 2^{math.log2(_got):.2f} of 2^{math.log2(_limit):.2f}  multiplier's bound x {_load:.3f}")
