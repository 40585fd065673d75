"""The expansion of product-form generator runs on the device (k_msm.hip k_gen_runs through otti_k_gen_runs / oa.kernels.gen_runs), against Python
integers: out[j][i] = base[j][i] + sum over the runs r of job j with i < 2^lg_r of c_r * prod_{t < lg_r, bit t of i set} f_r[t]  (mod l).  The
kernel stages a job's runs through LDS eight at a time (device.h kGenRunTile) and gives a slot to one thread, so the shapes below are: the empty
product, every small power of two, a vector longer than every run in it (and longer than one workgroup's 256 slots), jobs without runs and
without a base, runs of different lg in one job, many jobs in one launch, and more runs in one job than a tile holds."""
import numpy as np
import pytest

import otti_amd as oa
import orc

pytestmark = pytest.mark.gpu
K = oa.kernels
L = orc.L_ORDER
TILE = 8


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def _rand(rnd, k):
    return orc.fr_to_ints(orc.rand_fr(rnd, k))


def _expand(c, f):
    s = [c % L]
    for x in f:                                             # factor t doubles the vector: bit t set multiplies by f[t]
        s += [v * x % L for v in s]
    return s


def _want(n, base, runs):
    out = list(base) if base is not None else [0] * n
    for c, f in runs:
        for i, v in enumerate(_expand(c, f)):
            out[i] = (out[i] + v) % L
    return out


def _check(jobs):
    """jobs: [(n, base ints or None, [(c, [f ..])])]"""
    got, ms = K.gen_runs([(n, None if b is None else orc.fr_from_ints(b), [(orc.fr_from_ints([c]), orc.fr_from_ints(f)) for c, f in runs]) for n, b, runs in jobs])
    assert ms > 0 and len(got) == len(jobs)
    for j, (n, b, runs) in enumerate(jobs):
        assert got[j].shape == (n, 32)
        have, want = orc.fr_to_ints(got[j]), _want(n, b, runs)
        bad = [i for i in range(n) if have[i] != want[i]]
        assert not bad, "job %d: %d of %d slots differ, the first at %d" % (j, len(bad), n, bad[0])


@pytest.mark.parametrize("n", [1, 2, 4, 64, 256, 512])
def test_one_run_over_the_whole_vector(n):
    """n = 1: lg = 0, the product is empty and the slot gets base + c"""
    rnd = np.random.default_rng(n); lg = n.bit_length() - 1
    _check([(n, _rand(rnd, n), [(_rand(rnd, 1)[0], _rand(rnd, lg))])])
    _check([(n, None, [(_rand(rnd, 1)[0], _rand(rnd, lg))])])


def test_a_vector_longer_than_every_run_in_it():
    """515 slots, runs of 512 and of 4: slots 512 .. 514 keep their base, the second workgroup's tail stays inside the vector"""
    rnd = np.random.default_rng(515)
    _check([(515, _rand(rnd, 515), [(_rand(rnd, 1)[0], _rand(rnd, 9)), (_rand(rnd, 1)[0], _rand(rnd, 2))])])
    _check([(515, None, [(_rand(rnd, 1)[0], _rand(rnd, 9))])])


def test_jobs_with_no_run_and_with_no_base():
    rnd = np.random.default_rng(7)
    _check([(300, _rand(rnd, 300), []), (8, None, [(_rand(rnd, 1)[0], _rand(rnd, 3))]), (5, None, []), (257, _rand(rnd, 257), [])])


def test_three_runs_of_different_lg_in_one_job():
    rnd = np.random.default_rng(9107)
    _check([(1026, _rand(rnd, 1026), [(_rand(rnd, 1)[0], _rand(rnd, lg)) for lg in (9, 10, 7)])])


def test_sixteen_jobs_of_three_runs():
    """the localisation shape: a job per proof, the proof's three closing equations as its runs"""
    rnd = np.random.default_rng(16)
    _check([(130 + j, _rand(rnd, 130 + j) if j % 3 else None, [(_rand(rnd, 1)[0], _rand(rnd, lg)) for lg in (7, 5, 6)]) for j in range(16)])


def test_more_runs_in_one_job_than_a_tile_holds():
    """2 * TILE + 3 runs: two full tiles and a short one, lg cycling so that a tile mixes lengths; its neighbour has exactly one tile"""
    rnd = np.random.default_rng(19)
    many = [(_rand(rnd, 1)[0], _rand(rnd, k % 7)) for k in range(2 * TILE + 3)]
    _check([(70, _rand(rnd, 70), many), (64, None, [(_rand(rnd, 1)[0], _rand(rnd, 6)) for _ in range(TILE)])])


def test_zero_coefficient_zero_factor_and_l_minus_one():
    rnd = np.random.default_rng(23)
    f = _rand(rnd, 6)
    zero_f = list(f); zero_f[2] = 0                          # every slot with bit 2 set gets nothing from this run
    top = [L - 1] * 6                                        # (-1)^popcount(i)
    _check([(64, [L - 1] * 64, [(0, f), (_rand(rnd, 1)[0], zero_f), (L - 1, top)]),
            (64, None, [(L - 1, top)]),
            (1, [L - 1], [(L - 1, [])])])


def test_refusals_before_the_device_is_touched():
    one = orc.fr_from_ints([1])
    with pytest.raises(oa.SpartanError):
        K.gen_runs([(4, None, [(one, orc.fr_from_ints([1, 2, 3]))])])              # 8 slots in a job of 4
    with pytest.raises(oa.SpartanError):
        K.gen_runs([])
