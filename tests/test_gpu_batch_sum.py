"""The batch verifier's device pass alone (dev_batch_sum through otti_k_batch_sum: one k_decode_niels_sets launch over sets lying one behind the
other, one k_msm_var_many launch whose jobs span consecutive sets), against the reference test_gpu_row_sum_many.py uses: points whose sums the
oracle can state (snark_verify_many_cases.RowBank).  With two sets or more the entry decodes the last one ahead and holds it resident, as the
verifier holds the generators."""
import numpy as np
import pytest

import otti_amd as oa
import orc
import snark_verify_many_cases as sm

pytestmark = pytest.mark.gpu
K = oa.kernels
L = orc.L_ORDER
ZEROS32 = np.zeros(32, dtype=np.uint8)


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def eq(a, b):
    return np.array_equal(np.asarray(a, dtype=np.uint8).reshape(-1), np.asarray(b, dtype=np.uint8).reshape(-1))


def _rand(rnd, k):
    return orc.fr_to_ints(orc.rand_fr(rnd, k))


def _set(B, n, first=0):
    return [B.D + (first + i) % sm.BANK_POINTS for i in range(n)]


def _run(B, sets, jobs):
    """sets: lists of bank indices; jobs: [(first set, number of sets, integer scalars)] -> (sums, codes), each sum held against the oracle's"""
    sums, codes, ms = K.batch_sum([B.points[np.asarray(ix)] for ix in sets], [(f, c, orc.fr_from_ints(s)) for f, c, s in jobs])
    assert ms > 0
    for j, (f, c, s) in enumerate(jobs):
        idx = [i for ix in sets[f:f + c] for i in ix]
        assert len(idx) == len(s)
        if codes[j] == 0:
            assert eq(sums[j], B.want(idx, s)), j
    return sums, codes


@pytest.mark.parametrize("n", [1, 2048, 2049])
def test_one_set_one_job(n):
    """one point; 2048 and 2049 points: one split and two (the seam of kVarChunk)"""
    B = sm.row_bank(); rnd = np.random.default_rng(n)
    _, codes = _run(B, [_set(B, n)], [(0, 1, _rand(rnd, n))])
    assert codes == [0]


def test_a_job_over_three_sets_the_same_sets_as_three_jobs_and_the_resident_set_twice():
    B = sm.row_bank(); rnd = np.random.default_rng(3)
    sets = [_set(B, 5), _set(B, 2049, first=7), _set(B, 1, first=3), _set(B, 16, first=100)]      # the last one is resident
    s = [_rand(rnd, len(ix)) for ix in sets]
    jobs = [(0, 3, s[0] + s[1] + s[2]), (0, 1, s[0]), (1, 1, s[1]), (2, 1, s[2]), (3, 1, s[3]), (3, 1, _rand(rnd, 16)), (1, 2, s[1] + s[2])]
    sums, codes = _run(B, sets, jobs)
    assert codes == [0] * len(jobs)
    assert not eq(sums[4], sums[5])
    whole = B.want([i for ix in sets[:3] for i in ix], s[0] + s[1] + s[2])
    assert eq(sums[0], whole)


def test_special_scalars_and_a_pair_that_cancels():
    B = sm.row_bank(); rnd = np.random.default_rng(5)
    special = [0, 1, L - 1, 2 ** 128 - 1]
    sets = [_set(B, 4), [B.D + 9, B.D + 9], _set(B, 8, first=20)]
    k = _rand(rnd, 1)[0]
    jobs = [(0, 1, special), (1, 1, [k, L - k]), (0, 2, special + [k, L - k]), (0, 1, [0] * 4), (2, 1, special + special)]
    sums, codes = _run(B, sets, jobs)
    assert codes == [0] * 5
    assert eq(sums[1], ZEROS32) and eq(sums[3], ZEROS32)                  # s P + (l - s) P, and all-zero scalars: the identity
    assert eq(sums[2], sums[0])


def test_exactly_the_jobs_over_an_undecodable_set_report_it():
    B = sm.row_bank(); rnd = np.random.default_rng(11)
    sets = [_set(B, 40), _set(B, 300, first=5), _set(B, 7, first=9), _set(B, 16, first=50)]
    C = [B.points[np.asarray(ix)].copy() for ix in sets]
    C[1][100] = np.frombuffer(sm.UNDECODABLE, dtype=np.uint8)
    s = [_rand(rnd, len(ix)) for ix in sets]
    jobs = [(0, 1, s[0]), (1, 1, s[1]), (2, 1, s[2]), (0, 3, s[0] + s[1] + s[2]), (3, 1, s[3]), (0, 1, s[0])]
    sums, codes, _ = K.batch_sum(C, [(f, c, orc.fr_from_ints(x)) for f, c, x in jobs])
    assert codes == [0, sm.DECOMPRESS, 0, sm.DECOMPRESS, 0, 0]
    for j, (f, c, x) in enumerate(jobs):
        assert eq(sums[j], B.want([i for ix in sets[f:f + c] for i in ix], x) if codes[j] == 0 else ZEROS32), j
    C[1] = B.points[np.asarray(sets[1])].copy(); C[3][15, 31] |= 0x80       # now the resident set holds a non-canonical field element
    sums, codes, _ = K.batch_sum(C, [(f, c, orc.fr_from_ints(x)) for f, c, x in jobs])
    assert codes == [0, 0, 0, 0, sm.DECOMPRESS, 0]


def test_refusals():
    B = sm.row_bank()
    C = B.points[np.asarray(_set(B, 8))]
    s = orc.fr_from_ints([1] * 8)
    for jobs in ([(1, 1, s)], [(0, 2, s)], [(0, 0, s)]):                    # sets that are not there; a job of no sets
        with pytest.raises(oa.SpartanError) as e:
            K.batch_sum([C], jobs)
        assert e.value.code == sm.BAD_ARG
    with pytest.raises(oa.SpartanError) as e:                               # the resident set together with an uploaded one
        K.batch_sum([C, C], [(0, 2, orc.fr_from_ints([1] * 16))])
    assert e.value.code == sm.BAD_ARG
    lib, ptr = oa.lib, oa.api._ptr
    comp = np.ascontiguousarray(C); sc = np.ascontiguousarray(s); out = np.zeros((1, 32), dtype=np.uint8); codes = (oa.api._i32 * 1)()
    f, c = np.zeros(1, dtype=np.uint32), np.ones(1, dtype=np.uint32)
    good = np.array([0, 8], dtype=np.uint64)
    assert lib.otti_k_batch_sum(1, ptr(comp), ptr(good), 1, ptr(f), ptr(c), ptr(sc), ptr(out), codes, None) == 0
    for args in ((1, None, ptr(good), 1, ptr(f), ptr(c), ptr(sc), ptr(out), codes, None), (1, ptr(comp), None, 1, ptr(f), ptr(c), ptr(sc), ptr(out), codes, None),
                 (1, ptr(comp), ptr(good), 1, None, ptr(c), ptr(sc), ptr(out), codes, None), (1, ptr(comp), ptr(good), 1, ptr(f), None, ptr(sc), ptr(out), codes, None),
                 (1, ptr(comp), ptr(good), 1, ptr(f), ptr(c), None, ptr(out), codes, None), (1, ptr(comp), ptr(good), 1, ptr(f), ptr(c), ptr(sc), None, codes, None),
                 (1, ptr(comp), ptr(good), 1, ptr(f), ptr(c), ptr(sc), ptr(out), None, None), (0, ptr(comp), ptr(good), 1, ptr(f), ptr(c), ptr(sc), ptr(out), codes, None),
                 (1, ptr(comp), ptr(good), 0, ptr(f), ptr(c), ptr(sc), ptr(out), codes, None)):
        assert lib.otti_k_batch_sum(*args) == sm.BAD_ARG
    for off in ([0, 0, 8], [1, 8], [0, (1 << 20) + 1]):                     # an empty set; offsets that do not start at 0; more than 2^20 points
        o = np.array(off, dtype=np.uint64)
        assert lib.otti_k_batch_sum(len(off) - 1, ptr(comp), ptr(o), 1, ptr(f), ptr(c), ptr(sc), ptr(out), codes, None) == sm.BAD_ARG
