"""CPU tests of the host's sum of a small MSM's chunk results (k_msm_small mails each workgroup's sum in cached form; the prover
adds them up, split over its helper threads): the mail path, with AVX-512 IFMA where the CPU has it and in the scalar form, against
the generic point code, on random points and on edge cases (identity, negatives, repeated points, non-canonical coordinates)."""
import hashlib

import pytest

import otti_amd.api as oa

P = 2**255 - 19


def _fe(b, k):
    return int.from_bytes(b[32 * k:32 * k + 32], "little")


def _pt(x, y, z, t):
    return b"".join((v % P).to_bytes(32, "little") for v in (x, y, z, t))


def _rand_point(i):
    return oa.host_point_from_uniform(hashlib.sha512(b"host-point-sum-%d" % i).digest())


def _neg(pt):
    x, y, z, t = (_fe(pt, k) for k in range(4))
    return _pt(-x, y, z, -t)


def _scaled(pt, lam):
    """the same group element with the projective coordinates multiplied by lam"""
    return _pt(*(_fe(pt, k) * lam for k in range(4)))


IDENTITY = _pt(0, 1, 1, 0)


def _check(pts, parts=(1, 2, 3)):
    want = oa.host_point_sum(b"".join(pts), 0)
    for path in (1, 2):
        for k in parts:
            assert oa.host_point_sum(b"".join(pts), path, k) == want, (path, k)
    return want


@pytest.mark.parametrize("n", [1, 2, 7, 26, 52, 64, 103])
def test_random_points(n):
    _check([_rand_point(i) for i in range(n)], parts=(1, 2, 4))


def test_identity_and_empty():
    assert _check([]) == bytes(32)
    assert _check([IDENTITY] * 5) == bytes(32)
    a = _rand_point(1)
    assert _check([IDENTITY, a, IDENTITY]) == oa.host_point_sum(a, 0)


def test_negatives_cancel():
    pts = [_rand_point(i) for i in range(6)]
    assert _check(pts + [_neg(p) for p in reversed(pts)]) == bytes(32)
    assert _check([pts[0], _neg(pts[0]), pts[1]]) == oa.host_point_sum(pts[1], 0)


def test_repeated_points_double():
    a, c = _rand_point(3), _rand_point(4)
    _check([a] * 8, parts=(1, 2, 4, 8))
    _check([a, c, a, c, a])
    assert _check([a, a]) != oa.host_point_sum(a, 0)


def test_other_representatives():
    # projective rescaling and coordinates >= p (the device's loosely reduced form) give the same group element
    pts = [_rand_point(i) for i in range(10)]
    alt = [_scaled(p, 12345 + 7 * i) for i, p in enumerate(pts)]
    assert _check(alt) == _check(pts)
    x, y, z, t = (_fe(pts[0], k) for k in range(4))
    loose = b"".join(((v % P) + P).to_bytes(32, "little") if (v % P) + P < 2**256 else (v % P).to_bytes(32, "little") for v in (x, y, z, t))
    assert _check([loose] + pts[1:]) == _check(pts)


def test_stale_mail_is_not_taken():
    pts = [_rand_point(i) for i in range(5)]
    with pytest.raises(Exception):
        oa.host_point_sum(b"".join(pts), 3)


def test_bench_runs():
    ifma, scalar = oa.host_point_sum_bench(52, 50)
    assert scalar > 0 and ifma >= 0
