"""The sparse kernels (k_sparse.hip) at their edges, variant by variant: multiply_vec, eval_table_sparse and the satisfiability pass on the hand-built
instances of sparse_cases.py, against its reference in Python integers (test_sparse_cases_host.py shows inputs and reference right without a GPU).
Exact in GF(l): no tolerance.  Every case first asserts, through Instance.device_info, WHICH kernels it runs — the layout (k_*_light / k_*_quad), the
coefficient path (<true>: 4-byte codes and fr_mul_small, <false>: the nine-limb product) and the segmented path (k_spmv3_heavy_seg, then
k_spmv3_heavy_combine or k_sat_heavy_check) — so a change to a selection rule or to a builder cannot move coverage from one kernel to another unseen."""
import numpy as np
import pytest

import otti_amd as oa
import orc
import sparse_cases as sc

pytestmark = pytest.mark.gpu
K, KD = oa.kernels, oa.kernels_dev
L = sc.L
POISON = 0xa5


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def _instance(case):
    inst = oa.Instance.new(case.nc, case.nv, case.ni, *case.arrays())
    assert inst.dims == (case.ncp, case.nvp, case.ni)
    return inst


def _assert_variant(inst, case):
    """device_info reports the variant the case was built for, by row and by column; the long lists and their segments are counted here"""
    for by_col, layout in ((False, case.layout), (True, case.layout_col)):
        info = inst.device_info(by_col=by_col)
        longest = case.lengths(by_col).max(axis=0)
        heavy = [int(n) for n in longest if n > 64]
        print(case.name, "by_col" if by_col else "by_row", info)
        assert info["rows"] == (2 * case.nvp if by_col else case.ncp) and info["entries"] == tuple(len(m) for m in case.ents)
        assert info["use_small"] == case.codes, (case.name, info)
        if layout is not None:
            assert info["quad"] == (layout == "quad"), (case.name, by_col, info)
        assert info["n_heavy"] == len(heavy) and info["n_seg"] == sum((n + 2047) // 2048 for n in heavy), (case.name, by_col, info, heavy)
    return inst.device_info()


def _assert_rows_equal(case, what, got32, want_ints, lengths):
    """element for element; a mismatch names the rows and their three list lengths"""
    want32 = orc.fr_from_ints(want_ints)
    assert got32.shape == want32.shape, (case.name, what)
    bad = np.nonzero((got32 != want32).any(axis=1))[0]
    if bad.size:
        got = orc.fr_to_ints(got32[bad[:8]])
        detail = ["row %d (lengths A, B, C = %s): got %x want %x" % (r, lengths[:, r].tolist(), g, want_ints[r]) for r, g in zip(bad[:8].tolist(), got)]
        pytest.fail("%s: %s differs in %d of %d rows\n  %s" % (case.name, what, bad.size, len(want_ints), "\n  ".join(detail)))


def _poisoned(n):
    return oa.DeviceArray.from_host(np.full((n, 32), POISON, dtype=np.uint8))


def _check_products(inst, case, stream=None):
    z32, eq32, coef32 = orc.fr_from_ints(case.z), orc.fr_from_ints(case.eq), orc.fr_from_ints(case.coef)
    want_abc, want_t = case.multiply_vec(), case.eval_table()
    ln_row, ln_col = case.lengths(), case.lengths(by_col=True)
    ga, gb, gc, _ = K.multiply_vec(inst, z32)
    for k, g in enumerate((ga, gb, gc)):
        _assert_rows_equal(case, "multiply_vec %sz" % "ABC"[k], g, want_abc[k], ln_row)
    got, _ = K.eval_table_sparse(inst, eq32, coef32)
    _assert_rows_equal(case, "eval_table_sparse", got, want_t, ln_col)
    pad = case.nvp + 1 + case.ni
    assert not got[pad:].any() and not any(want_t[pad:])                                  # the empty padded half: written, and zero
    if stream is None:
        return
    # the same launches into buffers filled with a pattern beforehand: an element no kernel writes shows as the pattern, whatever the allocator hands out
    dz, deq = oa.DeviceArray.from_host(z32), oa.DeviceArray.from_host(eq32)
    out = [_poisoned(case.ncp) for _ in range(3)] + [_poisoned(2 * case.nvp)]
    KD.multiply_vec(inst, dz, out[0], out[1], out[2], stream)
    KD.eval_table_sparse(inst, deq, coef32, out[3], stream)
    KD.stream_sync(stream)
    for k in range(3):
        _assert_rows_equal(case, "multiply_vec %sz (device pointers)" % "ABC"[k], out[k].to_host(), want_abc[k], ln_row)
    _assert_rows_equal(case, "eval_table_sparse (device pointers)", out[3].to_host(), want_t, ln_col)


def _check_sat(inst, case, max_rows=64):
    """the pass's bitmap word for word (into a buffer filled with a pattern: every word is written, padding bits are clear) and its count; then the
    resident form's rows and values"""
    want_rows, want_abc = case.failing()
    words = (case.ncp + 63) // 64
    want_bits = np.zeros(words, dtype=np.uint64)
    for r in want_rows:
        want_bits[r >> 6] |= np.uint64(1 << (r & 63))
    z = oa.DeviceArray.from_host(orc.fr_from_ints(case.z))
    bits = oa.DeviceArray(words, 8)
    oa.lib.otti_dev_upload(bits.ptr, np.full(words, 0xa5a5a5a5a5a5a5a5, dtype=np.uint64).ctypes.data_as(oa.api._vp), words * 8)
    n = KD.check_sat(inst, z, bits)
    got_bits = bits.to_host().reshape(-1).view(np.uint64)
    bad = np.nonzero(got_bits != want_bits)[0]
    assert not bad.size, "%s: bitmap words %s: got %s want %s" % (case.name, bad[:4].tolist(), [hex(int(x)) for x in got_bits[bad[:4]]], [hex(int(x)) for x in want_bits[bad[:4]]])
    assert n == len(want_rows), (case.name, n, len(want_rows))
    assert case.is_assignment()
    wit = oa.Witness(inst, oa.VarsAssignment.new(case.vars32()), oa.InputsAssignment.new(case.inputs32()))
    rep = wit.check_sat(inst, max_rows=max_rows, values=True)
    assert rep.n_unsat == len(want_rows) and rep.rows.tolist() == want_rows[:max_rows], (case.name, rep.n_unsat, rep.rows.tolist()[:8], want_rows[:8])
    assert rep.values.shape == (len(rep.rows), 3, 32)
    for i, r in enumerate(rep.rows.tolist()):
        assert tuple(int.from_bytes(rep.values[i, j].tobytes(), "little") for j in range(3)) == want_abc[r], (case.name, "values of row", r)
    return rep


@pytest.fixture(scope="module")
def stream():
    s = KD.stream_create()
    yield s
    KD.stream_sync(s)
    KD.stream_destroy(s)


# ------------------------------------------------------------------------------------------------ (a) the ladder of list lengths
# between them: k_spmv3_light<true/false>, k_spmv3_quad<true/false>, k_spmv3_heavy_seg<true/false> and k_spmv3_heavy_combine, by row and by column
@pytest.mark.parametrize("layout,which,mix,transposed", sc.ladder_params())
def test_ladder(stream, layout, which, mix, transposed):
    case = sc.ladder_case(layout, which, mix, transposed)
    inst = _instance(case)
    _assert_variant(inst, case)
    info = inst.device_info(by_col=transposed)
    assert (info["quad"], info["use_small"], info["n_heavy"], info["n_seg"]) == (layout == "quad", mix in ("codes", "codes_with_wide"), 6, 10)
    _check_products(inst, case, stream)


# the by-column set in the quad layout (k_spmv3_quad over 2 * num_vars rows of which the padded half is empty)
@pytest.mark.parametrize("mix", sc.MIXES)
def test_column_set_in_the_quad_layout(stream, mix):
    case = sc.column_quad_case(mix)
    inst = _instance(case)
    _assert_variant(inst, case)
    info = inst.device_info(by_col=True)
    assert info["quad"] and info["n_heavy"] == 0 and info["rows"] == 2 * case.nvp and info["use_small"] == (mix in ("codes", "codes_with_wide"))
    _check_products(inst, case, stream)


# ------------------------------------------------------------------------------------------------ (b) fr_mul_small at its ends
@pytest.mark.parametrize("layout", ["lane", "quad"])
def test_code_edges(stream, layout):
    case = sc.code_edge_case(layout)
    inst = _instance(case)
    info = _assert_variant(inst, case)
    assert info["use_small"] and info["quad"] == (layout == "quad") and inst.device_info(by_col=True)["use_small"]
    _check_products(inst, case, stream)
    # every row that holds entries is reported with its values: k_sat_light / k_sat_quad <true> and k_sat_report<true> over the same products
    want_rows, _ = case.failing()
    assert len(want_rows) >= len(sc.edge_words()) - 2
    rep = _check_sat(inst, case, max_rows=case.ncp)
    assert len(rep.rows) == len(want_rows)


# ------------------------------------------------------------------------------------------------ (c) the decision for codes at its boundary
@pytest.mark.parametrize("layout", ["lane", "quad"])
@pytest.mark.parametrize("total,n_small", sc.BOUNDARIES)
def test_code_decision_boundary(stream, layout, total, n_small):
    case = sc.boundary_case(layout, total, n_small)
    inst = _instance(case)
    info = _assert_variant(inst, case)
    assert info["use_small"] == (total >= 1024 and 2 * n_small >= total)               # the rule of classify_coefficients
    assert sum(info["entries"]) == total
    _check_products(inst, case, stream)
    _check_sat(inst, case, max_rows=case.ncp)


# ------------------------------------------------------------------------------------------------ (d) the satisfiability pass where its writers meet
# lane / quad x codes / none: k_sat_light<true/false>, k_sat_quad<true/false>, each with k_spmv3_heavy_seg and k_sat_heavy_check behind it, whose
# atomicOr lands in a word the first launch has stored
@pytest.mark.parametrize("layout,codes", [("lane", True), ("lane", False), ("quad", True), ("quad", False)])
def test_sat_pass_on_the_satisfiable_ladder(rng, layout, codes):
    sat = sc.SatLadder(layout, codes)
    sets = sat.failing_sets()
    # besides the named sets: a random one drawn here, a third of the rows, every long row among them or not by the draw
    sets["random_third"] = sorted(int(r) for r in rng.choice(sat.nc, size=sat.nc // 3, replace=False))
    for name, rows in sets.items():
        case = sat.with_failing(rows)
        inst = _instance(case)
        info = _assert_variant(inst, case)
        assert (info["quad"], info["use_small"], info["n_heavy"]) == (layout == "quad", codes, 6), (name, info)
        rep = _check_sat(inst, case)
        assert rep.n_unsat == len(rows) and bool(rep) == (not rows), name
        if name == "none":
            _check_products(inst, case)


@pytest.mark.parametrize("nc", [2, 16])
def test_sat_pass_on_one_partly_filled_word(nc):
    sat = sc.SatLadder("quad", False, nc, 8)
    for name, rows in sat.failing_sets().items():
        case = sat.with_failing(rows)
        inst = _instance(case)
        info = _assert_variant(inst, case)
        assert info["quad"] and not info["use_small"] and info["rows"] == nc and info["n_heavy"] == 0
        rep = _check_sat(inst, case)                                                     # one word: bits nc .. 63 must come back clear
        assert rep.n_unsat == len(rows), name
        _check_products(inst, case)
