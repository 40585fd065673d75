"""The batched variable-base row sums (k_decode_niels_sets + k_msm_var_many through otti_k_row_sum_many): against otti_k_row_sum, the single launch
they share their body with, byte for byte; against the oracle's commitments, over points whose sums it can state (snark_verify_many_cases.RowBank:
every point is the oracle's commitment to a row of integers over 16 generators); per-set decode failures; and the entry's refusals."""
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
    """n distinct bank points"""
    return [B.D + first + i for i in range(n)]


@pytest.mark.parametrize("n", [256, 257, 2049])
def test_one_job_gives_the_single_launchs_bytes(n):
    B = sm.row_bank(); rnd = np.random.default_rng(n)
    idx, s = _set(B, n), _rand(rnd, n)
    C, sc = B.points[np.asarray(idx)], orc.fr_from_ints(s)
    sums, codes = K.row_sum_many([C], [(0, sc)])
    assert codes == [0]
    assert eq(sums[0], K.row_sum(C, sc)) and eq(sums[0], B.want(idx, s))


def test_sets_of_five_sizes_and_seven_jobs_in_one_call():
    B = sm.row_bank(); rnd = np.random.default_rng(7)
    sizes = [1, 255, 256, 257, 2049]
    sets = [_set(B, n, first=k) for k, n in enumerate(sizes)]
    special = [0, 1, L - 1, 2 ** 252, int("80" * 31, 16)]
    jobs = [(0, _rand(rnd, 1)), (1, _rand(rnd, 255)), (2, _rand(rnd, 256)), (3, [0] * 257), (4, _rand(rnd, 2049)), (4, _rand(rnd, 2049)),
            (3, special + _rand(rnd, 257 - len(special)))]
    assert jobs[4][1] != jobs[5][1]
    sums, codes = K.row_sum_many([B.points[np.asarray(ix)] for ix in sets], [(k, orc.fr_from_ints(s)) for k, s in jobs])
    assert codes == [0] * 7
    for j, (k, s) in enumerate(jobs):
        assert eq(sums[j], B.want(sets[k], s)), j
    assert eq(sums[3], ZEROS32)                                  # all-zero scalars: the identity
    for j in (2, 4, 6):                                          # at the sizes the single launch takes: its bytes
        k, s = jobs[j]
        assert eq(sums[j], K.row_sum(B.points[np.asarray(sets[k])], orc.fr_from_ints(s))), j


def test_exactly_the_jobs_over_an_undecodable_set_report_it():
    B = sm.row_bank(); rnd = np.random.default_rng(11)
    sets = [_set(B, 300), _set(B, 256, first=5), _set(B, 257, first=9), _set(B, 40)]
    C = [B.points[np.asarray(ix)].copy() for ix in sets]
    C[1][256 // 3] = np.frombuffer(sm.UNDECODABLE, dtype=np.uint8)          # s = 1 is odd: not a ristretto255 encoding
    C[2][256, 31] |= 0x80                                                   # a non-canonical field element
    jobs = [(0, _rand(rnd, 300)), (1, _rand(rnd, 256)), (2, _rand(rnd, 257)), (3, _rand(rnd, 40)), (1, _rand(rnd, 256)), (0, _rand(rnd, 300))]
    sums, codes = K.row_sum_many(C, [(k, orc.fr_from_ints(s)) for k, s in jobs])
    assert codes == [0, sm.DECOMPRESS, sm.DECOMPRESS, 0, sm.DECOMPRESS, 0]
    for j, (k, s) in enumerate(jobs):
        assert eq(sums[j], B.want(sets[k], s) if codes[j] == 0 else ZEROS32), j


def test_equal_points_and_opposite_pairs_in_one_launch():
    B = sm.row_bank(); rnd = np.random.default_rng(13)
    n = 257
    same = [B.D + 5] * n
    pair_s = _rand(rnd, n // 2)
    pairs = [x for i in range(n // 2) for x in (B.D + i, B.N + i)] + [B.zero]
    s_pairs = [x for k in pair_s for x in (k, k)] + [L - 1]
    s_same = _rand(rnd, n)
    sums, codes = K.row_sum_many([B.points[np.asarray(same)], B.points[np.asarray(pairs)]], [(0, orc.fr_from_ints(s_same)), (1, orc.fr_from_ints(s_pairs))])
    assert codes == [0, 0]
    assert eq(sums[0], B.want(same, s_same))
    assert eq(sums[1], ZEROS32) and eq(sums[1], B.want(pairs, s_pairs))


def test_forty_jobs_over_one_set():
    """40 jobs of one split each over 256 shared points: the flattened grid's block rows walk the whole prefix table"""
    B = sm.row_bank(); rnd = np.random.default_rng(17)
    idx = _set(B, 256)
    ss = [_rand(rnd, 256) for _ in range(40)]
    sums, codes = K.row_sum_many([B.points[np.asarray(idx)]], [(0, orc.fr_from_ints(s)) for s in ss])
    assert codes == [0] * 40
    for j, s in enumerate(ss):
        assert eq(sums[j], B.want(idx, s)), j


def test_refusals():
    B = sm.row_bank()
    C = B.points[np.asarray(_set(B, 8))]
    s = orc.fr_from_ints([1] * 8)
    sums, codes = K.row_sum_many([C], [(0, s)])                  # fewer than 256 points are allowed here
    assert codes == [0] and eq(sums[0], B.want(_set(B, 8), [1] * 8))
    with pytest.raises(oa.SpartanError) as e:
        K.row_sum_many([C], [(1, s)])                            # a set index out of range
    assert e.value.code == sm.BAD_ARG
    lib, ptr = oa.lib, oa.api._ptr
    comp = np.ascontiguousarray(C); sc = np.ascontiguousarray(s); out = np.zeros((1, 32), dtype=np.uint8); codes = (oa.api._i32 * 1)()
    js = np.zeros(1, dtype=np.uint32)
    good = np.array([0, 8], dtype=np.uint64)
    assert lib.otti_k_row_sum_many(1, ptr(comp), ptr(good), 1, ptr(js), ptr(sc), ptr(out), codes) == 0
    for args in ((1, None, ptr(good), 1, ptr(js), ptr(sc), ptr(out), codes), (1, ptr(comp), None, 1, ptr(js), ptr(sc), ptr(out), codes),
                 (1, ptr(comp), ptr(good), 1, None, ptr(sc), ptr(out), codes), (1, ptr(comp), ptr(good), 1, ptr(js), None, ptr(out), codes),
                 (1, ptr(comp), ptr(good), 1, ptr(js), ptr(sc), None, codes), (1, ptr(comp), ptr(good), 1, ptr(js), ptr(sc), ptr(out), None),
                 (0, ptr(comp), ptr(good), 1, ptr(js), ptr(sc), ptr(out), codes), (1, ptr(comp), ptr(good), 0, ptr(js), ptr(sc), ptr(out), codes)):
        assert lib.otti_k_row_sum_many(*args) == sm.BAD_ARG
    empty = np.array([0, 0, 8], dtype=np.uint64)                 # an empty set
    assert lib.otti_k_row_sum_many(2, ptr(comp), ptr(empty), 1, ptr(js), ptr(sc), ptr(out), codes) == sm.BAD_ARG
    big = np.array([0, (1 << 20) + 1], dtype=np.uint64)          # more than 2^20 points: refused before the memory is looked at
    assert lib.otti_k_row_sum_many(1, ptr(comp), ptr(big), 1, ptr(js), ptr(sc), ptr(out), codes) == sm.BAD_ARG
