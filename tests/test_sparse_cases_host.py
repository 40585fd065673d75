"""The inputs and the reference of the sparse kernels' edge tests (sparse_cases.py), shown right without a GPU: for every builder the integer
reference equals the C oracle's multiply_vec and eval_table_sparse, the expected failing set equals the oracle's, and the instance has the
properties it was built for (list lengths, word properties, entry counts, and the variant the selection rules give)."""
import pytest

import otti_amd as oa
import orc
import sparse_cases as sc

L = sc.L


def _oracle(case):
    A, B, C = case.arrays()
    o = orc.OInstance(case.nc, case.nv, case.ni, A, B, C)
    assert (o.num_cons, o.num_vars) == (case.ncp, case.nvp)
    return o


def _check_against_oracle(case):
    o = _oracle(case)
    want = case.multiply_vec()
    got = orc.multiply_vec(o, orc.fr_from_ints(case.z))
    for k in range(3):
        assert orc.fr_to_ints(got[k]) == want[k], (case.name, "multiply_vec", k)
    tabs = [orc.fr_to_ints(t) for t in orc.eval_table_sparse(o, orc.fr_from_ints(case.eq))]
    assert tabs == case.eval_tables(), (case.name, "eval_table_sparse")
    c = case.coef
    assert case.eval_table() == [(c[0] * a + c[1] * b + c[2] * d) % L for a, b, d in zip(*tabs)]
    # the failing set, from the oracle's products and from the oracle's own verdict
    a, b, d = (orc.fr_to_ints(x) for x in got)
    rows, abc = case.failing()
    assert rows == [r for r in range(case.ncp) if a[r] * b[r] % L != d[r]]
    assert all(abc[r] == (a[r], b[r], d[r]) for r in rows)
    if case.is_assignment():
        assert o.is_sat(case.vars32(), case.inputs32()) == (not rows)
    return o


def _check_declared_variant(case):
    v, vc = case.variant(), case.variant(by_col=True)
    assert v["quad"] == (case.layout == "quad") and (case.layout_col is None or vc["quad"] == (case.layout_col == "quad")), (case.name, v, vc)
    assert v["use_small"] == vc["use_small"] == case.codes, (case.name, v, case.counts())
    assert v["rows"] == case.ncp and vc["rows"] == 2 * case.nvp


def test_entry_dtype_and_constants_are_the_products():
    assert sc.ENTRY_DTYPE == oa.ENTRY_DTYPE and sc.L == oa.L_ORDER == orc.L_ORDER
    assert orc.fr_to_ints(orc.fr_from_ints([5, L - 1])) == [5, L - 1]
    assert sc.mont_words([1, 2]) == [int.from_bytes(b.tobytes(), "little") for b in orc.fr_from_ints([1, 2])]
    assert sc.from_mont_words(sc.mont_words([0, 7, L - 3])) == [0, 7, L - 3]
    for v, small in ((0, True), (1, True), (L - 1, True), (2 ** 31 - 2, True), (L - (2 ** 31 - 2), True), (2 ** 31 - 1, False), (L - (2 ** 31 - 1), False),
                     (2 ** 31, False), (L - 2 ** 31, False), (2 ** 32 - 1, False), ((L + 1) // 2, False), ((L - 1) // 2, False)):
        assert sc.is_small(v) == small, v


@pytest.mark.parametrize("layout,which,mix,transposed", sc.ladder_params())
def test_ladder_case(layout, which, mix, transposed):
    case = sc.ladder_case(layout, which, mix, transposed)
    _check_declared_variant(case)
    ln = case.lengths(by_col=transposed)
    places = sc.ladder_places(case.nv if transposed else case.nc)
    assert sorted(places.values()) == sorted(sc.LADDER) and {0, 63, 64, 127, (case.nv if transposed else case.nc) - 1} <= set(places)
    fill = 4 if layout == "quad" else 1
    for j, n in places.items():
        assert ln[which][j] == n, (j, n)
        assert all(ln[k][j] == fill for k in range(3) if k != which)                  # the long list is in ONE matrix: the others end before its second segment
        # distinct minor indices within the ladder's lists
        minor = [(r if transposed else c) for r, c, _ in case.ents[which] if (c if transposed else r) == j]
        assert len(minor) == n == len(set(minor))
    v = case.variant(by_col=transposed)
    assert v["n_heavy"] == 6 and v["n_seg"] == 1 + 1 + 1 + 2 + 2 + 3
    other = case.variant(by_col=not transposed)
    assert other["n_heavy"] == 0 or not transposed
    # the coefficient mix, list by list: a quarter of the other kind in every ladder list of four or more
    total, n_small = case.counts()
    for j, n in places.items():
        kinds = [sc.is_small(val) for r, c, val in case.ents[which] if (c if transposed else r) == j]
        if mix == "codes":
            assert all(kinds)
        elif mix == "nocodes":
            assert not any(kinds)
        elif n >= 4:
            minority = sum(kinds) if mix == "wide_with_codes" else n - sum(kinds)
            assert n // 4 <= minority <= n // 4 + 1, (j, n, minority)
    assert (2 * n_small >= total) == case.codes
    # the repeated pair and the explicit zero
    pairs = [(r, c) for r, c, _ in case.ents[which]]
    assert pairs.count((3, 11)) >= 2 and any(val == 0 for _, _, val in case.ents[which])
    _check_against_oracle(case)


@pytest.mark.parametrize("mix", sc.MIXES)
def test_column_quad_case(mix):
    case = sc.column_quad_case(mix)
    _check_declared_variant(case)
    ln = case.lengths(by_col=True)
    used = case.nv + 1 + case.ni
    assert ln[:, :case.nv].min() >= 5 and ln.max() <= 9 and not ln[:, case.nvp + 1 + case.ni:].any() and ln[:, case.nvp:case.nvp + 1 + case.ni].all()
    assert used < 2 * case.nvp and case.variant(True)["n_heavy"] == 0 and case.variant()["n_heavy"] == 0
    _check_against_oracle(case)


@pytest.mark.parametrize("layout", ["lane", "quad"])
def test_code_edge_case(layout):
    case = sc.code_edge_case(layout)
    _check_declared_variant(case)
    total, n_small = case.counts()
    assert total >= 1024 and 2 * n_small >= total and case.variant()["n_heavy"] == 0 and case.variant(True)["n_heavy"] == 0
    words, over = sc.edge_words(), sc.overshoot_words()
    assert all(w < L for w in words) and {0, 1, L - 1, L - 2, 2 ** 252 - 1, 2 ** 252, 2 ** 252 + 1} <= set(words)
    assert len({m for m, _ in over}) >= 5
    for m, w in over:
        assert 0 < m <= sc.CODE_MAX and w * m % 2 ** 252 < m
        assert (w * m) >> 252 == w * m // L + 1                                        # the estimate is one too large: the subtraction has to wrap
    # the kernels' words ARE these: z and eq in Montgomery form start with them
    assert sc.mont_words(case.z[:len(words)]) == words and sc.mont_words(case.eq[:len(words)]) == words
    coefs = {c for m in case.ents for _, _, c in m}
    assert set(sc.EDGE_COEFS) <= coefs and {x for m in sc.EDGE_MAGS for x in (m, L - m)} <= coefs
    # every coefficient meets every word, in its row (z) and in its column (eq)
    met = {(i, c) for m in case.ents for i, j, c in m if i == j}
    assert met == {(i, c) for i in range(len(words)) for c in coefs}
    # codes and wide values share rows in each matrix
    for m in case.ents:
        row0 = [sc.is_small(c) for r, _, c in m if r == 0]
        assert any(row0) and not all(row0)
    _check_against_oracle(case)


@pytest.mark.parametrize("layout", ["lane", "quad"])
@pytest.mark.parametrize("total,n_small", sc.BOUNDARIES)
def test_boundary_case(layout, total, n_small):
    case = sc.boundary_case(layout, total, n_small)
    _check_declared_variant(case)
    assert case.counts() == (total, n_small)
    assert case.codes == {(1023, 1023): False, (1024, 512): True, (1024, 511): False}[(total, n_small)]
    assert case.lengths().max() <= sc.HEAVY_ROW and case.lengths(True).max() <= sc.HEAVY_ROW
    _check_against_oracle(case)


@pytest.mark.parametrize("layout,codes,nc,nv", [("lane", True, None, None), ("lane", False, None, None), ("quad", True, None, None), ("quad", False, None, None),
                                                ("quad", False, 2, 8), ("quad", False, 16, 8)])
def test_satisfiable_ladder(layout, codes, nc, nv):
    sat = sc.SatLadder(layout, codes, nc, nv)
    sets = sat.failing_sets()
    if nc is None:
        assert sat.heavy_rows == [0, 63, 64, 127, 130, sat.nc - 1]
        assert set(sets) == {"none", "heavy_bit0", "heavy_bit63", "last_row", "heavy_with_light", "heavy_passes_alone", "all"}
        hw = sets["heavy_with_light"]
        assert len({r >> 6 for r in hw}) == 1 and set(hw) & set(sat.heavy_rows) and set(hw) - set(sat.heavy_rows)
        alone = sets["heavy_passes_alone"]
        assert len(alone) == 63 and {r >> 6 for r in alone} == {1} and 64 in sat.heavy_rows and 64 not in alone
    for name, rows in sets.items():
        case = sat.with_failing(rows)
        _check_declared_variant(case)
        assert case.is_assignment()
        assert all(len([1 for r, c, _ in case.ents[2] if r == q]) == 1 for q in (0, sat.nc - 1)) and all(c == sat.nv for _, c, _ in case.ents[2])
        got, abc = case.failing()
        assert got == sorted(rows), name
        assert all(abc[r][2] == (abc[r][0] * abc[r][1] + 1) % L for r in got)
        if name in ("none", "heavy_with_light", "all", "first"):
            _check_against_oracle(case)
