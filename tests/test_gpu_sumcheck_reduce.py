"""The round kernels' in-launch reduction (k_sumcheck.hip block_reduce_dealt: the two or three sums of a round dealt out over the lanes of a
wave, the waves' totals met in LDS, the workgroups' partial sums met in the last workgroup) against the oracle, bit-exact.  Tables that are
zero except for ONE item make the round's sums that item's terms alone: whichever lane, wave and workgroup holds the item, every one of the
sums has to come through — a term routed to the wrong slot or dropped on the way shows, where random tables would only show that something did."""
import numpy as np
import pytest

import otti_amd as oa
import orc

pytestmark = pytest.mark.gpu
K = oa.kernels

# items of a one-workgroup launch: lane 0, both sides of every lane bit the dealing splits on (16, 32), the last lane of a wave, the other waves
ONE_WORKGROUP = [0, 1, 15, 16, 17, 31, 32, 47, 48, 63, 64, 130, 255]


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _only_item(rng, n, stride, j, count):
    """`count` tables of length n, zero except for the entries of item j (entries j, j + stride, ...)"""
    out = []
    for _ in range(count):
        t = orc.fr_from_ints([0] * n)
        t[j::stride] = orc.rand_fr(rng, len(range(j, n, stride)))
        out.append(t)
    return out


def _cubic3_want(E, B, C, D):
    return orc.sc_cubic_evals(np.concatenate([E, E]), B, C, D)


@pytest.mark.parametrize("n,items", [(512, ONE_WORKGROUP), (1 << 12, [0, 300, 1024, 2047])])
def test_evaluation_rounds_with_one_nonzero_item(rng, n, items):
    """n = 512: 256 items, one workgroup, a thread each; 2^12: eight workgroups, the item in the first, the second, the fifth and the last"""
    tau = orc.rand_fr(rng, n.bit_length() - 2); E = orc.eq_evals(tau)
    for j in items:
        A, B, C = _only_item(rng, n, n // 2, j, 3)
        want2, want3 = orc.sc_quad_evals(A, B), _cubic3_want(E, A, B, C)
        assert any(orc.fr_to_ints(want2)) and any(orc.fr_to_ints(want3))
        assert eq(K.sc_quad_round(A, B)[0], want2), j
        assert eq(K.sc_cubic3_round(A, B, C, tau)[0], want3), j
        assert eq(K.sc_cubic_round(C, A, B, A)[0], orc.sc_cubic_evals(C, A, B, A)), j


@pytest.mark.parametrize("n,items", [(1024, [0, 16, 33, 48, 200, 255]), (1 << 13, [5, 600, 2047])])
def test_fold_rounds_with_one_nonzero_item(rng, n, items):
    tau = orc.rand_fr(rng, n.bit_length() - 3); E = orc.eq_evals(tau); r = orc.rand_fr(rng, 1)
    for j in items:
        A, B, C = _only_item(rng, n, n // 4, j, 3)
        fa, fb, fc = (orc.fold_top(x, r) for x in (A, B, C))
        out2, e2, _ = K.sc_quad_fold_round(A, B, r)
        assert eq(out2[0], fa) and eq(out2[1], fb) and eq(e2, orc.sc_quad_evals(fa, fb)), j
        out3, e3, _ = K.sc_cubic3_fold_round(A, B, C, r, tau)
        assert eq(out3[0], fa) and eq(out3[2], fc) and eq(e3, _cubic3_want(E, fa, fb, fc)), j


def test_sums_of_the_largest_elements_over_a_full_grid(rng):
    """every term l - 1 or near it, 2^19 items on the widest grid the plan gives a 2^20 proof: the additions' conditional subtractions at every step"""
    n, l = 1 << 20, orc.L_ORDER
    A = np.repeat(orc.fr_from_ints([l - 1]), n, axis=0); B = np.repeat(orc.fr_from_ints([1]), n, axis=0)
    assert eq(K.sc_quad_round(A, B)[0], orc.sc_quad_evals(A, B))
    assert eq(K.sc_quad_round(A, A)[0], orc.sc_quad_evals(A, A))
