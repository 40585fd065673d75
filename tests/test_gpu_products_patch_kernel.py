"""The kept-products patch at kernel level (otti_k_products_patch: k_prod_mark / k_prod_mark_heavy, the compaction, k_prod_rows / k_prod_rows_heavy,
and the full pass behind the cut-over), on the hand-built instances of sparse_cases.py and products_cases.py, against SparseCase.multiply_vec in
Python integers.  Exact in GF(l): no tolerance.

How a patch is judged: the stale vectors handed in are filled with a marker word that no sum can equal (0xa5.., above l; asserted absent from the
reference), the bitmap and count are those of the OLD z.  Afterwards every touched row holds the reference word of the NEW z bit for bit, every
other row still holds the marker, the listed rows are exactly the model's touched set in ascending order, and bitmap and count are those of the
new z.  OTTI_PRODUCTS_FULL_SHARE=1 pins the patch (a long column touches half of the rows); the cut-over test lifts it.

The ladder over COLUMNS exists in the lane layout only (sparse_cases.ladder_case builds its transposed twin for that layout alone), so the by-column
set's quad layout, which has no long column there, is met on column_quad_case; the ladder over ROWS runs in both layouts."""
import numpy as np
import pytest

import otti_amd as oa
import orc
import products_cases as pc
import sparse_cases as sc

pytestmark = pytest.mark.gpu
K = oa.kernels
L = sc.L


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(autouse=True)
def _patch_pinned(monkeypatch):
    monkeypatch.setenv("OTTI_PRODUCTS_FULL_SHARE", "1")


_instances = {}


def _instance(case, variant=""):
    """(the instance, the reference of the case's own z): built and computed once per case, never changed.  variant: tells cases of one name apart"""
    key = case.name + variant
    if key not in _instances:
        inst = oa.Instance.new(case.nc, case.nv, case.ni, *case.arrays())
        assert inst.dims == (case.ncp, case.nvp, case.ni)
        _instances[key] = (inst, case.multiply_vec())
    return _instances[key]


def _words(ints):
    return orc.fr_from_ints(ints)


def _patch(case, inst, old_abc, z_new, cols, stale=None, range_form=None, expect_full=False):
    """one otti_k_products_patch call judged as the module docstring says; returns the new reference (abc as integers)"""
    n = case.ncp
    new_abc = case.multiply_vec(z_new)
    want_rows = pc.touched_rows(case, cols)
    want32 = [_words(v) for v in new_abc]
    marker = pc.marker_rows(n)
    for w in want32:
        assert not (w == marker).all(axis=1).any()              # the marker is absent from the reference
    old_fail, new_fail = pc.failing_of(old_abc), pc.failing_of(new_abc)
    stale = [marker] * 3 if stale is None else stale
    kw = dict(cols=np.array(cols, dtype=np.uint64)) if range_form is None else dict(first=range_form[0], count=range_form[1])
    a, b, c, bits, unsat, rows, full, ms = K.products_patch(inst, _words(z_new), stale[0], stale[1], stale[2], pc.bitmap(old_fail, n), len(old_fail), **kw)
    print("%s: cols %s.. -> %d rows touched, full=%s, %.3f ms, failing %d -> %d" % (case.name, list(cols)[:4], len(rows), full, ms, len(old_fail), unsat))
    assert rows.tolist() == want_rows, (case.name, cols, rows[:8].tolist(), want_rows[:8])
    assert full == expect_full
    touched = np.zeros(n, dtype=bool)
    touched[want_rows] = True
    for k, got in enumerate((a, b, c)):
        keep = np.ones(n, dtype=bool) if expect_full else touched
        bad = np.nonzero((got[keep] != want32[k][keep]).any(axis=1))[0]
        assert not bad.size, "%s: %sz differs from the reference in %d rows it should hold, first %s" % (case.name, "ABC"[k], bad.size, np.nonzero(keep)[0][bad[:4]].tolist())
        assert (got[~keep] == stale[k][~keep]).all(), "%s: %sz was written outside the touched rows" % (case.name, "ABC"[k])
    want_bits = pc.bitmap(new_fail, n)
    assert np.array_equal(bits, want_bits), (case.name, np.nonzero(bits != want_bits)[0][:4].tolist())
    assert unsat == len(new_fail)
    return new_abc


# ------------------------------------------------------------------------------------------------ (a) column-length cut-overs (the mark kernels)
# the by-column set of the transposed ladder: lists of 0 .. 64 entries go a column per lane (k_prod_mark<false>), 65 .. 4097 a workgroup per column
# (k_prod_mark_heavy: kHeavyRow, and kHeavySeg of the segmented product passes); every constraint row is short, so k_prod_rows<codes, false> recomputes
@pytest.mark.parametrize("mix", ["codes", "nocodes"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_column_length_cut_overs(which, mix):
    case = sc.ladder_case("lane", which, mix, transposed=True)
    inst, ref = _instance(case)
    info = inst.device_info(by_col=True)
    assert (info["quad"], info["use_small"], info["n_heavy"]) == (False, mix == "codes", 6)
    for n, col in pc.columns_by_length(case, which):
        z_new = pc.changed_z(case, case.z, [col])
        assert len(pc.touched_rows(case, [col])) >= min(n, 1)
        _patch(case, inst, ref, z_new, [col])


# the by-column set in the quad layout (k_prod_mark<true>: four lanes per column), columns of 5 .. 9 entries per matrix; the by-row set is quad too
@pytest.mark.parametrize("mix", ["codes", "nocodes"])
def test_columns_in_the_quad_layout(mix):
    case = sc.column_quad_case(mix)
    inst, ref = _instance(case)
    assert inst.device_info(by_col=True)["quad"] and inst.device_info()["quad"] and inst.device_info()["use_small"] == (mix == "codes")
    for cols in ([0], [5, 6, 7, 900], list(range(64, 192))):
        _patch(case, inst, ref, pc.changed_z(case, case.z, cols), cols)


# ------------------------------------------------------------------------------------------------ (b) row-length cut-overs (the recompute kernels)
# the untransposed ladder: the changed column sits in the row of each length, so k_prod_rows<codes, quad> meets rows of 0 .. 64 entries and
# k_prod_rows_heavy<codes> those of 65 .. 4097
@pytest.mark.parametrize("mix", ["codes", "nocodes"])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("layout", ["lane", "quad"])
def test_row_length_cut_overs(layout, which, mix):
    case = sc.ladder_case(layout, which, mix)
    inst, ref = _instance(case)
    info = inst.device_info()
    assert (info["quad"], info["use_small"], info["n_heavy"]) == (layout == "quad", mix == "codes", 6)
    ln = case.lengths()[which]
    for n, col in pc.columns_by_row_length(case, which):
        assert any(ln[r] == n for r in pc.touched_rows(case, [col]))
        _patch(case, inst, ref, pc.changed_z(case, case.z, [col]), [col])


# ------------------------------------------------------------------------------------------------ (c) the ends of the touched bitmap
def test_bitmap_edges():
    case = pc.edges_case()
    inst, ref = _instance(case)
    for name, (cols, rows) in pc.EDGE_CHANGES.items():
        assert pc.touched_rows(case, cols) == rows, name
        _patch(case, inst, ref, pc.changed_z(case, case.z, cols), cols)


# ------------------------------------------------------------------------------------------------ (d) verdict transitions
@pytest.mark.parametrize("layout,codes", [("lane", True), ("lane", False), ("quad", True), ("quad", False)])
def test_verdict_transitions(layout, codes):
    sat = sc.SatLadder(layout, codes)
    case = sat.with_failing([])
    inst, ref0 = _instance(case)
    assert not pc.failing_of(ref0)
    cols = pc.sat_changes(sat, case)
    assert len(cols) >= 6
    z1, z2 = pc.changed_z(case, case.z, cols, 1), pc.changed_z(case, case.z, cols, 2)
    ref1 = _patch(case, inst, ref0, z1, cols)                   # sat -> unsat
    n1 = len(pc.failing_of(ref1))
    assert n1 >= len(cols)
    ref2 = _patch(case, inst, ref1, z2, cols)                   # unsat -> unsat, with other values
    assert len(pc.failing_of(ref2)) == n1 and ref2[0] != ref1[0]
    ref3 = _patch(case, inst, ref2, case.z, cols)               # unsat -> sat
    assert not pc.failing_of(ref3) and ref3 == ref0
    # from a state in which OTHER rows fail as well: their bits and their share of the count stay
    bad = sat.with_failing([1, 62, 200])
    inst_b, ref_b = _instance(bad, " failing 1, 62, 200")
    assert pc.failing_of(ref_b) == [1, 62, 200]
    _patch(bad, inst_b, ref_b, pc.changed_z(bad, bad.z, cols, 3), cols)


def test_padding_rows_stay_clear():
    sat = sc.SatLadder("quad", False, 12, 8)                    # 12 constraints in a word of 16 padded rows
    case = sat.with_failing([3])
    inst, ref = _instance(case, " failing 3")
    assert case.ncp == 16 and pc.failing_of(ref) == [3]
    cols = [0, 3]
    new = _patch(case, inst, ref, pc.changed_z(case, case.z, cols), cols)
    assert all(r < 12 for r in pc.failing_of(new)) and all(r < 12 for r in pc.touched_rows(case, cols))


# ------------------------------------------------------------------------------------------------ (e) the cut-over
def test_cut_over(monkeypatch):
    case = sc.ladder_case("lane", 0, "codes", transposed=True)
    inst, ref = _instance(case)
    cols = sorted(c for _, c in pc.columns_by_length(case, 0))[:8]
    z_new = pc.changed_z(case, case.z, cols)
    old32 = [_words(v) for v in ref]
    outs = {}
    for share in ("0", "1"):
        monkeypatch.setenv("OTTI_PRODUCTS_FULL_SHARE", share)
        old_fail = pc.failing_of(ref)
        outs[share] = K.products_patch(inst, _words(z_new), old32[0], old32[1], old32[2], pc.bitmap(old_fail, case.ncp), len(old_fail), cols=np.array(cols, dtype=np.uint64))
        assert outs[share][6] == (share == "0")                 # took_full_pass
    for x, y in zip(outs["0"][:6], outs["1"][:6]):
        assert np.array_equal(x, y)
    new_abc = case.multiply_vec(z_new)
    for k in range(3):
        assert np.array_equal(outs["1"][k], _words(new_abc[k]))
    # under the full pass the marker survives nowhere
    monkeypatch.setenv("OTTI_PRODUCTS_FULL_SHARE", "0")
    _patch(case, inst, ref, z_new, cols, expect_full=True)
    # ... and the rule itself: 4097 of 8192 rows touched is above any share below one half, one row is below it
    monkeypatch.setenv("OTTI_PRODUCTS_FULL_SHARE", "0.25")
    _patch(case, inst, ref, pc.changed_z(case, case.z, [0]), [0], expect_full=True)
    _patch(case, inst, ref, pc.changed_z(case, case.z, [5]), [5], expect_full=False)


# ------------------------------------------------------------------------------------------------ (f) the range form
def test_range_form_equals_the_list_form():
    case = sc.ladder_case("lane", 2, "nocodes", transposed=True)
    inst, ref = _instance(case)
    for first, count in ((0, 8), (60, 10), (case.nvp - 3, 6), (case.nvp, 1 + case.ni), (7, 0)):
        cols = list(range(first, first + count))
        z_new = pc.changed_z(case, case.z, cols)
        _patch(case, inst, ref, z_new, cols, range_form=(first, count))
        _patch(case, inst, ref, z_new, cols)
