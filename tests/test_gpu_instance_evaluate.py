"""A, B, C at several points in one pass (k_sparse.hip k_eval_*; otti_k_instance_evaluate), variant by variant, against Python integers:
    M_k(rx_t, ry_t) = sum over M_k's entries (r, c, v) of v * eq(rx_t)[r] * eq(ry_t)[c']        c' = c shifted by the variable padding
eq tables come from the oracle (orc.eq_evals), held once against the product formula, MSB first.  Exact in GF(l): no tolerance; results are compared
as canonical integers.  Every case first asserts through Instance.device_info WHICH kernels it runs (row per lane / per quad, codes on / off, the
segmented long lists), as test_gpu_sparse_edges.py does.  The tile holds four points: K = 5 is a full tile and a tail of one, K = 9 crosses the
chunk of eight resident points."""
import functools

import numpy as np
import pytest

import otti_amd as oa
import orc
import sparse_cases as sc

pytestmark = pytest.mark.gpu
K = oa.kernels
L = sc.L
KINDS = ("random", "rx_zero", "edge")


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def _points(name, nrx, nry, count):
    """count points (rx, ry) as integer lists: uniform / rx all zero (eq(rx) is the indicator of row 0) / coordinates from {0, 1, l - 1}, in turn"""
    rng = sc._rng("points", name, count)
    pts = []
    for i in range(count):
        kind = KINDS[i % 3]
        if kind == "edge":
            rx, ry = [rng.choice((0, 1, L - 1)) for _ in range(nrx)], [rng.choice((0, 1, L - 1)) for _ in range(nry)]
        else:
            rx, ry = sc._field(rng, nrx), sc._field(rng, nry)
            if kind == "rx_zero":
                rx = [0] * nrx
        pts.append((rx, ry))
    return pts


def _eq_ints(r):
    return orc.fr_to_ints(orc.eq_evals(orc.fr_from_ints(r))) if r else [1]


def _eq_by_formula(r):
    """EqPolynomial::evals by its definition: index bits MSB first over r"""
    ell = len(r)
    out = []
    for i in range(1 << ell):
        x = 1
        for j in range(ell):
            x = x * (r[j] if (i >> (ell - 1 - j)) & 1 else (1 - r[j])) % L
        out.append(x)
    return out


def _expected(ents_shifted, pts):
    """[(A, B, C) per point] over entry lists whose columns are already shifted"""
    out = []
    for rx, ry in pts:
        ex, ey = _eq_ints(rx), _eq_ints(ry)
        out.append(tuple(sum(v * ex[r] * ey[c] for r, c, v in m) % L for m in ents_shifted))
    return out


def _evaluate(inst, pts):
    nrx, nry = len(pts[0][0]), len(pts[0][1])
    rx = orc.fr_from_ints([x for p in pts for x in p[0]]).reshape(len(pts), nrx, 32)
    ry = orc.fr_from_ints([x for p in pts for x in p[1]]).reshape(len(pts), nry, 32)
    out, ms = K.instance_evaluate(inst, rx, ry)
    assert out.shape == (len(pts), 3, 32) and ms >= 0
    return [tuple(orc.fr_to_ints(out[t])) for t in range(len(pts))]


def _assert_variant(inst, case):
    info = inst.device_info()
    longest = case.lengths().max(axis=0)
    heavy = [int(n) for n in longest if n > 64]
    print(case.name, info)
    assert info["rows"] == case.ncp and info["entries"] == tuple(len(m) for m in case.ents)
    assert info["use_small"] == case.codes and info["quad"] == (case.layout == "quad"), (case.name, info)
    assert info["n_heavy"] == len(heavy) and info["n_seg"] == sum((n + 2047) // 2048 for n in heavy), (case.name, info, heavy)
    return info


@functools.lru_cache(maxsize=4)
def _built(builder, *args):
    case = builder(*args)
    inst = oa.Instance.new(case.nc, case.nv, case.ni, *case.arrays())
    assert inst.dims == (case.ncp, case.nvp, case.ni)
    shifted = [[(r, case.col_shifted(c), v) for r, c, v in m] for m in case.ents]
    return case, inst, shifted


def _check_case(case, inst, shifted, count):
    nrx, nry = case.ncp.bit_length() - 1, (2 * case.nvp).bit_length() - 1
    pts = _points(case.name, nrx, nry, count)
    got, want = _evaluate(inst, pts), _expected(shifted, pts)
    for t in range(count):
        for k in range(3):
            assert got[t][k] == want[t][k], "%s: %s at point %d of %d (%s): got %x want %x" % (case.name, "ABC"[k], t, count, KINDS[t % 3], got[t][k], want[t][k])


def test_oracle_eq_tables_are_the_product_formula_msb_first():
    rng = sc._rng("eq-formula")
    for r in (sc._field(rng, 1), sc._field(rng, 6), [0, 1, L - 1, 5, 0, 1, L - 2]):
        assert _eq_ints(r) == _eq_by_formula(r)
    zero = _eq_ints([0] * 5)
    assert zero[0] == 1 and not any(zero[1:])                                          # rx all zero: the indicator of row 0


# ------------------------------------------------------------------------------------------------ (a) every by-row ladder case, a full tile and a tail
# between them k_eval_light<true/false>, k_eval_quad<true/false>, k_eval_heavy_seg<true/false>, k_eval_heavy_combine and k_eval_finish over lists of
# 0 .. 4097 entries at word and wave edges
@pytest.mark.parametrize("layout,which,mix", [(l, w, m) for l, w, m, tr in sc.ladder_params() if not tr])
def test_ladder_at_five_points(layout, which, mix):
    case, inst, shifted = _built(sc.ladder_case, layout, which, mix)
    info = _assert_variant(inst, case)
    assert (info["quad"], info["use_small"], info["n_heavy"], info["n_seg"]) == (layout == "quad", mix in ("codes", "codes_with_wide"), 6, 10)
    _check_case(case, inst, shifted, 5)


# ------------------------------------------------------------------------------------------------ (b) the point count: one point, short tiles, the chunk bound
@pytest.mark.parametrize("layout", ["lane", "quad"])
def test_point_counts_around_tile_and_chunk(layout):
    case, inst, shifted = _built(sc.ladder_case, layout, 0, "codes_with_wide")
    _assert_variant(inst, case)
    for count in (1, 3, 4, 8, 9):
        _check_case(case, inst, shifted, count)


# ------------------------------------------------------------------------------------------------ (c) fr_mul_small at its ends, applied to a tile
@pytest.mark.parametrize("layout", ["lane", "quad"])
def test_code_edges_at_four_points(layout):
    case, inst, shifted = _built(sc.code_edge_case, layout)
    info = _assert_variant(inst, case)
    assert info["use_small"] and info["quad"] == (layout == "quad")
    _check_case(case, inst, shifted, 4)


# ------------------------------------------------------------------------------------------------ (d) many workgroups: the sum over their partials is real
def test_synthetic_instance_over_many_workgroups():
    n = 1 << 14
    r = oa.synth_r1cs(n, 10, 1)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    ncp, nvp, _ = inst.dims
    info = inst.device_info()
    print("synth 2^14", info)
    assert info["rows"] == ncp == n and not info["quad"] and info["n_heavy"] == 0 and ncp // 256 > 1
    nv = r["num_vars"]
    shifted = [[(int(e["row"]), int(e["col"]) + (nvp - nv if int(e["col"]) >= nv else 0), int.from_bytes(e["val"].tobytes(), "little")) for e in m] for m in (r["A"], r["B"], r["C"])]
    pts = _points("synth14", ncp.bit_length() - 1, (2 * nvp).bit_length() - 1, 4)
    assert _evaluate(inst, pts) == _expected(shifted, pts)


def test_argument_refusals():
    case, inst, _ = _built(sc.code_edge_case, "quad")
    out, ms = K.instance_evaluate(inst, np.zeros((0, 32), dtype=np.uint8), np.zeros((0, 32), dtype=np.uint8))       # K = 0: nothing done
    assert out.shape == (0, 3, 32)
    assert oa.lib.otti_k_instance_evaluate(None, None, None, 0, None, None) == -21
    assert oa.lib.otti_k_instance_evaluate(inst._h, None, None, 2, None, None) == -21
