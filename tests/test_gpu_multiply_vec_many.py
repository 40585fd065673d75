"""The many-vector sparse product (k_sparse.hip k_spmv3_many_*, otti_k_multiply_vec_many) on the hand-built instances of sparse_cases.py: every
variant — row per lane / per quad, coefficient codes on / off, segmented long rows — at the ladder of list lengths (63 / 64 / 65 and
2047 / 2048 / 2049 / 4096 / 4097 among them) and at the ends of fr_mul_small's range.  Each case first asserts through Instance.device_info WHICH
kernels it runs.  K vectors go through tiles of four: K = 1 (one slot live), 4 (a full tile), 5 (a full tile and a tile of one), and on one case per
layout 2, 3 and 9.  Expected: the case's reference in Python integers, exact in GF(l), and bit equality with the single-vector kernels."""
import numpy as np
import pytest

import otti_amd as oa
import orc
import sparse_cases as sc

pytestmark = pytest.mark.gpu
K = oa.kernels
L = sc.L
EDGE_WORDS = (0, 1, L - 1, 2 ** 252 - 1, 2 ** 252, 2 ** 252 + 1)


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def vectors(case, n):
    """n vectors of the case's length.  0: case.z itself.  1: all zero.  k >= 2: case.z with variable i scaled and shifted by k, z_i (k + 1) + k, and
    its k-th run of odd slots overwritten so that the KERNEL's word there is one of EDGE_WORDS (as sparse_cases._vectors does for slot run 0)."""
    out = [list(case.z), [0] * len(case.z)]
    for k in range(2, n):
        z = list(case.z)
        for i in range(case.nv):
            z[i] = (z[i] * (k + 1) + k) % L
        for i, w in enumerate(EDGE_WORDS):
            slot = 2 * (len(EDGE_WORDS) * k + i) + 1
            assert slot < case.nv
            z[slot] = w * sc.R_INV % L
        out.append(z)
    return out[:n]


def _check(case, ks):
    inst = oa.Instance.new(case.nc, case.nv, case.ni, *case.arrays())
    info, want_variant = inst.device_info(), case.variant()
    print(case.name, info)
    assert {k: info[k] for k in want_variant} == want_variant, (case.name, info, want_variant)
    zs = vectors(case, max(ks))
    z32 = [orc.fr_from_ints(z) for z in zs]
    want = [[orc.fr_from_ints(m) for m in case.multiply_vec(z)] for z in zs]        # the integer reference, once per vector
    single = [K.multiply_vec(inst, z)[:3] for z in z32]
    for k, z in enumerate(zs):
        for j in range(3):
            assert np.array_equal(single[k][j], want[k][j]), (case.name, "single multiply_vec", k, "ABC"[j])
    assert not any(m.any() for m in want[1])                                        # the zero vector's products are zero words
    for n in ks:
        got = K.multiply_vec_many(inst, z32[:n])[:3]
        for j in range(3):
            assert got[j].shape == (n, case.ncp, 32)
            for k in range(n):
                bad = np.nonzero((got[j][k] != want[k][j]).any(axis=1))[0]
                assert not bad.size, "%s: K = %d, vector %d, %sz differs in %d rows, first %s (list lengths %s)" % (
                    case.name, n, k, "ABC"[j], bad.size, bad[:6].tolist(), case.lengths()[:, bad[:6]].tolist())
    return info


LADDER = [(layout, which, "codes_with_wide") for layout in ("lane", "quad") for which in range(3)] + \
         [(layout, 0, mix) for layout in ("lane", "quad") for mix in ("codes", "nocodes", "wide_with_codes")]


@pytest.mark.parametrize("layout,which,mix", LADDER)
def test_ladder(layout, which, mix):
    case = sc.ladder_case(layout, which, mix)
    more = (2, 3, 9) if (which, mix) == (1, "codes_with_wide") else ()              # one lane case and one quad case
    info = _check(case, (1, 4, 5) + more)
    assert (info["quad"], info["use_small"], info["n_heavy"], info["n_seg"]) == (layout == "quad", mix in ("codes", "codes_with_wide"), 6, 10)


@pytest.mark.parametrize("layout", ["lane", "quad"])
def test_code_edges(layout):
    case = sc.code_edge_case(layout)
    info = _check(case, (4,))
    assert info["use_small"] and info["quad"] == (layout == "quad")
