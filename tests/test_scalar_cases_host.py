"""The operands and the reference of the device's GF(l) tests (scalar_cases.py), shown right without a GPU: the constants against the oracle and
fr9.h, the restated product and top fold against the integers they stand for, every case against the precondition fr9.h states for its operation
(no case dropped), the reference's own columns below 2^64 — and the plain-C bodies of fr9.h (tests/limb9_check.cpp, host build) against the same
case file, limb for limb.  The device bodies run the same cases in tests/test_gpu_scalar_arith.py."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import orc
import scalar_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = sc.L


def test_constants_equal_the_headers_and_the_oracles():
    assert L == orc.L_ORDER and sc.R == orc._R
    text = open(os.path.join(ROOT, "otti_amd", "csrc", "fr9.h")).read()
    defs = {k: int(v, 16) for k, v in re.findall(r"#define FR9_(\w+) (0x[0-9a-f]+)u", text)}
    assert [defs["L%d" % i] for i in (0, 1, 2, 3, 4, 8)] == [sc.L9[i] for i in (0, 1, 2, 3, 4, 8)]
    assert defs["LINV"] == sc.LINV and defs["M"] == sc.M29 and sc.LINV * L % 2 ** 29 == 2 ** 29 - 1
    assert "%d" % sc.B_A in text and "%d" % sc.B_B in text            # the header's "loose" sentence states the derived bounds
    for K in sc.KS + (1,):
        o = sc.kl_limbs(K)
        assert sc.value(o) == K * L and all(sc.M29 <= x < 2 ** 30 + 1 for x in o[:8]) and o[8] >= 0


def test_loose_bounds_are_the_largest_that_the_inequality_admits():
    fits = lambda x, y: 9 * x * y + sc.M29 * sc.S + 2 ** 36 < 2 ** 64
    assert fits(sc.M29, sc.B_A) and not fits(sc.M29, sc.B_A + 1)
    assert fits(sc.B_B, sc.B_B) and not fits(sc.B_B + 1, sc.B_B + 1)
    assert sc.B_A < 2 ** 31.9                                         # what fr9.h used to offer beside a normalised operand does not fit ...
    _, top = sc.mul_columns((sc.M29,) * 9, (int(2 ** 31.9),) * 9)
    assert top >= 2 ** 64                                             # ... and a column of the product passes 2^64 there


def test_pools_hold_what_they_promise():
    for name in ("0", "1", "2", "l-1", "l-2", "(l+1)/2", "(l-1)/2", "2^252", "2^252-1", "l-2^232", "R mod l"):
        assert sc.NAMED[name] in sc.CANON
    for k in range(1, 9):
        assert 2 ** (29 * k) in sc.CANON and 2 ** (29 * k) - 1 in sc.CANON
    for k in range(1, 8):
        assert 2 ** (32 * k) in sc.CANON and 2 ** (32 * k) - 1 in sc.CANON
    for v in (2 ** 128, 2 ** 32 - 1, 2 ** 64 - 1):                    # with the named ones: the values the eight-word ops were given before
        assert v in sc.CANON
    for v in (L, L + 1, 2 * L - 1, 2 ** 253 - 1, 2 ** 255, 2 ** 256 - 1):
        assert v in sc.NONCANON and (v,) in sc.cases("unpack") and (v,) in sc.cases("unpack5")
    assert all(t[0] < 2 ** 253 for t in sc.cases("unpack10")) and (2 ** 253 - 1,) in sc.cases("unpack10")
    N = sc.NORMALISED
    assert (sc.M29,) * 9 in N and all(sc.unpack_s(w, 0) in N for w in sc.WORDS)
    for i in range(9):
        for x in (1, sc.M29):
            assert tuple(x if k == i else 0 for k in range(9)) in N
        for pool, b in ((sc.LOOSE_A, sc.B_A), (sc.LOOSE_B, sc.B_B)):
            for x in (b, b - 1):
                assert tuple(x if k == i else 0 for k in range(9)) in pool
    for t in sc.TOPS:
        assert sum(v[8] == t for v in N) >= 3 and (sc.M29,) * 8 + (t,) in N and (0,) * 8 + (t,) in N
    for pool, b in ((sc.LOOSE_A, sc.B_A), (sc.LOOSE_B, sc.B_B)):
        assert (b,) * 9 in pool and max(max(v) for v in pool) == b
    mul = sc.cases("mul")
    classes = {c: sum(sc.mul_class(a, b) == c for a, b in mul) for c in ("NA", "AN", "BB")}
    assert min(classes.values()) > 1000, classes
    assert ((sc.M29,) * 9, (sc.B_A,) * 9) in mul and ((sc.B_A,) * 9, (sc.M29,) * 9) in mul and ((sc.B_B,) * 9, (sc.B_B,) * 9) in mul
    hot = lambda i, x: tuple(x if k == i else 0 for k in range(9))
    for x, y in ((sc.M29, sc.M29), (sc.M29, sc.B_A), (sc.B_A, sc.M29), (sc.B_B, sc.B_B)):
        assert all((hot(i, x), hot(j, y)) in mul for i in range(9) for j in range(9))
    for K in sc.KS:
        top = sc.limbs_of(K * L - 2 ** 232 - 1)
        c = sc.cases("sub_kl%d" % K)
        assert any(b == top for _, b in c) and any(a == top and b == top for a, b in c)
        assert any(max(a) > sc.M29 for a, _ in c)                     # loose minuends too
    assert all((sc.unpack_s(a, 5), sc.unpack_s(b, 5)) in sc.cases("sub_kl128") for a, b in sc.CANON_PAIRS[::37])
    for op in ("mul", "mul9", "fold9") + tuple("sub_kl%d" % K for K in sc.KS):
        assert len(sc.cases(op)) > 1024 and len(sc.cases(op)) % 64    # more than one workgroup, a ragged last wave
    assert set(sc.OPS) == set(sc.PRECONDITION)


@pytest.mark.parametrize("op", sc.OPS)
def test_every_case_satisfies_its_operations_precondition(op):
    c = sc.cases(op)
    assert len(c) == len(set(c)) or op == "fold9"
    bad = [t for t in c if not sc.PRECONDITION[op](*t)]
    assert not bad, (op, len(bad), bad[:3])


def test_restated_product_stands_for_the_value_and_its_columns_stay_below_2_64():
    top, limb = 0, 0
    pairs = list(sc.cases("mul")) + [(a[0], a[0]) for a in sc.cases("mul_self")]
    pairs += [(sc.unpack_s(a, 5), sc.unpack_s(b, 0)) for a, b in sc.cases("mul9")]
    for x0, x2, r in sc.cases("fold9"):
        a = sc.unpack_s(x0, 0)
        pairs.append((sc.unpack_s(r, 5), sc.sub_kl(2, sc.unpack_s(x2, 0), a)))
    for a, b in pairs:
        assert sc.mul_class(a, b) is not None                         # fold9's and mul9's products are within the header's classes as well
        r, t = sc.mul_columns(a, b)
        top, limb = max(top, t), max(limb, max(a), max(b))
        va, vb, vr = sc.value(a), sc.value(b), sc.value(r)
        assert all(x <= sc.M29 for x in r[:8]) and r[8] < 2 ** 32
        assert vr * 2 ** 261 % L == va * vb % L and vr < va * vb // 2 ** 261 + L + 1
    assert top < 2 ** 64 and limb == sc.B_A
    assert top > 2 ** 63.9, math.log2(top)                            # ... and some case comes within a tenth of a bit of the accumulator's end


def test_restated_folds_and_differences_stand_for_the_value():
    for (a,) in sc.cases("fold_top"):
        r = sc.fold_top(a)
        assert sc.normalised(r) and sc.value(r) % L == sc.value(a) % L and 0 < sc.value(r) < 2 * L
    for K in sc.KS:
        for a, b in sc.cases("sub_kl%d" % K):
            r = sc.sub_kl(K, a, b)
            assert all(0 <= x < 2 ** 32 for x in r) and sc.value(r) == sc.value(a) - sc.value(b) + K * L
    for (a,) in sc.cases("norm"):
        r = sc.norm(a)
        assert sc.normalised(r) and sc.value(r) == sc.value(a)
    for t, (w, l) in zip(sc.cases("fold9"), sc.expected_all("fold9")):
        assert sc.normalised(l) and sc.value(l) < 3 * L and sc.value(l) % L == w
    for t, (w, l) in zip(sc.cases("mul9"), sc.expected_all("mul9")):
        assert sc.normalised(l) and sc.value(l) < 2 * L and sc.value(l) % L == w


def test_plain_c_bodies_of_fr9_h_equal_the_reference_on_every_case(tmp_path):
    """tests/limb9_check.cpp over the case file: unpack*, mul, mul_self, add, norm, sub_kl<K>, fold_top, shl5, pack_*, canon, mul9, fold9"""
    path = tmp_path / "scalar_cases.txt"
    n = sc.write_case_file(str(path))
    assert n == sum(len(sc.cases(op)) for op in sc.OPS)
    exe = tmp_path / "limb9_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "otti_amd", "csrc"), os.path.join(ROOT, "tests", "limb9_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "0", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "case file: %d cases" % n in r.stdout and "limb9 check: 0 failures" in r.stdout


def test_arrays_for_the_device_are_what_the_cases_say():
    a = np.frombuffer(b"".join(sc.words(v) for v in sc.WORDS), dtype=np.uint8).reshape(-1, 32)
    assert [int.from_bytes(r.tobytes(), "little") for r in a] == list(sc.WORDS)
