"""Kernel-level parity for SNARK mode's kernels (k_snark.hip: the batched sum-check round, its hand-over and persistent tail, product-circuit
layers, the hash layer, the evaluations' dot products; k_sumcheck.hip: the chunked bound) — each through the launch function the prover calls,
against the oracle's restatement of the operation or plain Python integers mod l, bit for bit.  A SNARK proof that differs from the oracle's
says nothing about where; these do.  Batches, table lengths and grids are chosen here, not by the prover: 1 .. 20 instances with product
circuits and triples interleaved, lengths on both sides of every switch (one workgroup / the last-workgroup reduction, one eq pyramid / two,
the grid cap), a rank's residue class of a sharded layer, the tail at every W, and tables made of the values at the ends of the field."""
import numpy as np
import pytest

import otti_amd as oa
import orc
from test_gpu_kernels import _edge_tables

pytestmark = pytest.mark.gpu
K = oa.kernels
l = orc.L_ORDER
BAD_ARG = -21


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def zeros(n):
    return np.zeros((n, 32), dtype=np.uint8)


def frand(rng, n):
    """n random elements without a Python loop: any 32 bytes below 2^252 are a Montgomery-form element"""
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x0f
    return a


def rolled(rng, n, count):
    """count different tables of n elements: one random block rotated by a different amount each (no two equal)"""
    if n < 1 << 12:
        return [frand(rng, n) for _ in range(count)]
    block = frand(rng, n)
    return [np.roll(block, 1 + 3 * k, axis=0) for k in range(count)]


_POOL = {}
_M29 = (1 << 29) - 1
# stored WORDS (Montgomery form as it lies in memory, every one below l) whose 29-bit limbs sit at their ends: all eight low limbs full with the largest
# top limb (2^252 - 1), full low limbs alone, full and empty limbs alternating both ways, l - 1 as a word — what the nine-limb unpack hands the products
_LIMB_WORDS = [(1 << 252) - 1, (1 << 232) - 1, sum(_M29 << (29 * i) for i in range(0, 8, 2)), sum(_M29 << (29 * i) for i in range(1, 8, 2)) | (0xfffff << 232),
               l - 1, 1, 1 << 251]


def _word_table(rng, n, choices):
    words = np.array([np.frombuffer(w.to_bytes(32, "little"), dtype=np.uint8) for w in choices])
    return words[rng.integers(0, len(choices), n)]


def edge_table(k, n):
    """table k of n elements from a pool of twelve, rotated by k: eight tables of edge VALUES (l - 1, 0, mixtures, limb boundaries:
    test_gpu_kernels._edge_tables) and four of edge WORDS (_LIMB_WORDS: all 2^252 - 1, mixtures with 0)"""
    if not _POOL:
        r = np.random.default_rng(977)
        _POOL["t"] = _edge_tables(r, 1 << 13, 8) + [_word_table(r, 1 << 13, _LIMB_WORDS[:1]), _word_table(r, 1 << 13, _LIMB_WORDS),
                                                    _word_table(r, 1 << 13, _LIMB_WORDS[:4] + [0]), _word_table(r, 1 << 13, [_LIMB_WORDS[0], 0])]
    return np.resize(np.roll(_POOL["t"][k % 12], 37 * k, axis=0), (n, 32))


def edge_scalars(rng):
    return [l - 1, 1, 0, int(rng.integers(0, 2 ** 62)) ** 4 % l]


def make_batch(kinds, tables):
    """kinds: a string of 'p' (product circuit: no third table) and 't' (triple); tables: an iterator of tables"""
    A, B, C = [], [], []
    for k in kinds:
        A.append(next(tables)); B.append(next(tables)); C.append(next(tables) if k == "t" else None)
    return A, B, C


def want_sums(E, a, b, c):
    if c is None:                                                  # the eq table is constant in the bound variable
        return orc.sc_cubic_evals(np.concatenate([E, E]), a, b, zeros(len(a)))
    return orc.sc_cubic_evals(a, b, c, zeros(len(a)))


def check_pc_round(A, B, C, tau, r=None, G=1, rk=0):
    e, folded, _ = K.pc_round(A, B, C, tau, r, G, rk)
    E = orc.eq_evals(tau)[rk::G]
    for y in range(len(A)):
        a, b, c = A[y], B[y], C[y]
        if r is not None:
            a, b, c = orc.fold_top(a, r), orc.fold_top(b, r), None if c is None else orc.fold_top(c, r)
            assert eq(folded[0][y], a) and eq(folded[1][y], b), ("folded A, B of instance", y)
            assert c is None or eq(folded[2][y], c), ("folded C of instance", y)
        assert eq(e[y], want_sums(E, a, b, c)), ("sums of instance", y, "product circuit" if c is None else "triple")


# ------------------------------------------------------------------------------------------------ k_pc_round<false / true>, finish_many
BATCHES = {"1p": "p", "4p": "pppp", "12p+6t": "ppt" * 6, "20mixed": "ptpp" * 5, "6t": "tttttt"}


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("n", [2, 1024, 1 << 13, 1 << 14])
def test_pc_round_shapes(rng, batch, n):
    """n without a fold and 2 n with one (the same number of items).  2: one pair, and with one instance the single-workgroup mail; 1024: the first
    multi-workgroup grid, so the last workgroup's reduction (20 instances: 60 of its 64 output slots); 2^13 / 2^14: one eq pyramid / the product of two"""
    kinds = BATCHES[batch]
    tau = orc.rand_fr(rng, n.bit_length() - 2)
    check_pc_round(*make_batch(kinds, iter(rolled(rng, n, 3 * len(kinds)))), tau)
    check_pc_round(*make_batch(kinds, iter(rolled(rng, 2 * n, 3 * len(kinds)))), tau, orc.rand_fr(rng, 1))


@pytest.mark.parametrize("fold,kind", [(False, "random"), (True, "random"), (False, "edge"), (True, "edge")], ids=["False", "True", "False-edge", "True-edge"])
def test_pc_round_at_the_grid_cap(rng, fold, kind):
    """18 instances with 2^15 items each: 128 workgroups per instance wanted, 2048 / 18 = 113 given — the grid-stride loop runs a second time under the
    library's own block cap (walks of 2 .. 1024 items, with the sweep and the fold of pc_acc_step: tests/test_gpu_pc_round_walks.py).  edge: the tables of edge_table (values and stored words at the ends
    of their ranges, a 2^13 block repeated: the stride of 113 * 256 items is no multiple of it, so a thread's two items differ), folded by l - 1"""
    kinds = "pppppppptppppppppt" if fold else "ppt" * 6
    n = 1 << 17 if fold else 1 << 16
    tables = (edge_table(k, n) for k in range(3 * len(kinds))) if kind == "edge" else iter(rolled(rng, n, 3 * len(kinds)))
    A, B, C = make_batch(kinds, tables)
    r = (orc.fr_from_ints([l - 1]) if kind == "edge" else orc.rand_fr(rng, 1)) if fold else None
    check_pc_round(A, B, C, orc.rand_fr(rng, 15), r)


@pytest.mark.parametrize("G", [2, 4])
def test_pc_round_on_a_ranks_residue_class(rng, G):
    """item i of rank rk's tables is element i G + rk of the layer: the eq factor is taken there (EqSrc.stride / offset)"""
    kinds, n = "pptppt", 1024
    for rk in range(G):
        for fold in (False, True):
            A, B, C = make_batch(kinds, iter(rolled(rng, n, 3 * len(kinds))))
            tau = orc.rand_fr(rng, (n // (4 if fold else 2) * G).bit_length() - 1)
            check_pc_round(A, B, C, tau, orc.rand_fr(rng, 1) if fold else None, G, rk)


@pytest.mark.parametrize("tau_kind", ["l-1", "1", "0", "random"])
@pytest.mark.parametrize("n,shift", [(8, 0), (1 << 11, 1), (1 << 15, 2)])
def test_pc_round_on_values_at_the_ends_of_the_field(rng, n, shift, tau_kind):
    """12 product circuits + 6 triples on tables of l - 1, 0, mixtures and limb-boundary values (rotated over A, B, C by `shift`), eq tables of
    l - 1 / 1 / 0 in every variable, folds by l - 1, 1, 0: the nine-limb paths' offsets and accumulations (abe_accum9, abc_accum9) at their extremes.
    (What these cannot tell apart: abe_accum9 with and without the carry sweep of dv.  With every limb of v, b_hi at 2^29 - 1 and u = b_lo = 0 the
    largest column of fr9_mul(dv, db) is 0.66 * 2^64, so the product of the unswept limbs is the same integer: that sweep is margin, not a need.)"""
    kinds = "ppt" * 6
    A, B, C = make_batch(kinds, (edge_table(k + shift, n) for k in range(3 * len(kinds))))
    nv = n.bit_length() - 2
    tau = orc.rand_fr(rng, nv) if tau_kind == "random" else orc.fr_from_ints([{"l-1": l - 1, "1": 1, "0": 0}[tau_kind]] * nv)
    check_pc_round(A, B, C, tau)
    for r_int in edge_scalars(rng):
        check_pc_round(A, B, C, tau[1:], orc.fr_from_ints([r_int]))


# ------------------------------------------------------------------------------------------------ k_pc_tail
def tail_w(ninst, wkind, t_out_is_w):
    """W, t_out of a case; "max": the largest power of two with ninst * W <= min(160, CUs) and W <= t_out"""
    if wkind != "max":
        W = int(wkind)
        return W, (W if t_out_is_w else 64)
    W = 1
    while 2 * W * ninst <= 160 and (t_out_is_w or 2 * W <= 64):
        W *= 2
    return W, (W if t_out_is_w else 64)


def tail_reference(A, B, C, tau, rs):
    """per round: the sums of every instance (the eq table a real third table, folded with the others), and the tables before that round's fold"""
    E = orc.eq_evals(tau)
    T = [[A[y], B[y], E if C[y] is None else C[y]] for y in range(len(A))]
    sums, tables = [], []
    for j in range(len(rs) + 1):
        tables.append(T)
        if j == len(rs):
            break
        sums.append([orc.sc_cubic_evals(t[0], t[1], t[2], zeros(len(t[0]))) for t in T])
        T = [[orc.fold_top(x, rs[j:j + 1]) for x in t] for t in T]
    return sums, tables


@pytest.mark.parametrize("kind", ["random", "edge"])
@pytest.mark.parametrize("per", [16, 64, 1024])
@pytest.mark.parametrize("wkind", ["1", "2", "max"])
@pytest.mark.parametrize("ninst", [1, 4, 18])
def test_pc_tail(rng, ninst, wkind, per, kind):
    """every round's sums of every instance and the handed-over tables in natural order, for t_out in {W, 64} x tables as they are / folded on load x the eq
    table's first variable in the table / as EqSrc.top — all against ONE reference (the folded-on-load run is given the unfolded tables, the plain run
    the oracle's fold of them).  per = len0 / W: below a wave (the shortened shuffle tree), a wave, kTailCap.  Geometries dev_pc_tail rejects
    (len0 <= t_out) are left out.  Tails follow one another in one process: the mail lines' numbers carry over."""
    kinds = {1: "t" if per == 64 else "p", 4: "ptpp", 18: "ppt" * 6}[ninst]
    ran = 0
    for W, t_out in sorted({tail_w(ninst, wkind, tw) for tw in (True, False)}):
        while True:
            try:
                ran += run_tails(rng, kinds, kind, W, per * W, t_out)
                break
            except oa.SpartanError as ex:                          # fewer CUs than workgroups (the library checks before it launches): the next W down
                if not (wkind == "max" and W > 1 and ex.code == BAD_ARG and "CUs" in str(ex)):
                    raise
                t_out, W = (W // 2 if t_out == W else t_out), W // 2
    assert ran


def run_tails(rng, kinds, kind, W, len0, t_out):
    if len0 <= t_out:
        return 0
    ninst = len(kinds)
    if kind == "random":
        S = make_batch(kinds, iter(rolled(rng, 2 * len0, 3 * ninst))); fold_r = orc.rand_fr(rng, 1)
    else:                                                          # a fold by 1 keeps the upper half: the plain run sees edge values too
        S = make_batch(kinds, (edge_table(k, 2 * len0) for k in range(3 * ninst))); fold_r = orc.fr_from_ints([1])
    F = tuple([None if t is None else orc.fold_top(t, fold_r) for t in X] for X in S)
    nt = len0.bit_length() - 1; rounds = nt - (t_out.bit_length() - 1)
    tau = orc.rand_fr(rng, nt); rs = orc.rand_fr(rng, rounds)
    special = orc.fr_from_ints([l - 1, 0, 1] if kind == "edge" else [1, 0, l - 1])
    rs[:min(3, rounds)] = special[:min(3, rounds)]
    want_s, want_t = None, None
    for fold in (False, True):
        for top in (False, True):
            src = S if fold else F
            sums, out = K.pc_tail(*src, W, t_out, tau, rs, fold_r if fold else None, top)
            if want_s is None:
                want_s, want_t = tail_reference(*F, tau, rs)
            for j in range(rounds):
                for y in range(ninst):
                    assert eq(sums[j][y], want_s[j][y]), ("sums", dict(W=W, t_out=t_out, fold=fold, top=top, round=j, instance=y))
            for y in range(ninst):
                for t in range(3):
                    if src[2][y] is None and t == 2:
                        assert out[y][2] is None
                    else:
                        assert eq(out[y][t], want_t[rounds][y][t]), ("handed-over table", dict(W=W, t_out=t_out, fold=fold, top=top, instance=y, table=t))
    return 4


# ------------------------------------------------------------------------------------------------ k_pc_export
@pytest.mark.parametrize("n_out", [1, 2, 64, 128])
def test_pc_export(rng, n_out):
    kinds = "ppt" * 6
    for fold in (False, True):
        n = 2 * n_out if fold else n_out
        A, B, C = make_batch(kinds, iter(rolled(rng, n, 3 * len(kinds))))
        r = orc.rand_fr(rng, 1) if fold else None
        out = K.pc_export(A, B, C, r)
        for y in range(len(kinds)):
            for t, X in enumerate((A, B, C)):
                if X[y] is None:
                    assert out[y][t] is None
                else:
                    assert eq(out[y][t], orc.fold_top(X[y], r) if fold else X[y]), (fold, y, t)


def test_pc_export_up_to_the_result_buffer(rng):
    """128 + 3 * ninst * n_out <= 8192 result slots: 20 x 128 and 10 x 256 are the largest batches that fit, 11 x 256 is the first that does not"""
    for ninst, n_out in ((20, 128), (10, 256)):
        A, B, C = make_batch("t" * ninst, iter(rolled(rng, n_out, 3 * ninst)))
        out = K.pc_export(A, B, C)
        assert all(eq(out[y][t], X[y]) for y in range(ninst) for t, X in enumerate((A, B, C)))
    A, B, C = make_batch("t" * 11, iter(rolled(rng, 256, 33)))
    with pytest.raises(oa.SpartanError) as ex:
        K.pc_export(A, B, C)
    assert ex.value.code == BAD_ARG
    A, B, C = make_batch("t" * 11, iter(rolled(rng, 512, 33)))     # the folded tables are what has to fit
    with pytest.raises(oa.SpartanError) as ex:
        K.pc_export(A, B, C, orc.fr_from_ints([0]))
    assert ex.value.code == BAD_ARG
    out = K.pc_export(A[:10], B[:10], C[:10], orc.fr_from_ints([0]))
    assert all(eq(out[y][t], X[y][:256]) for y in range(10) for t, X in enumerate((A, B, C)))


# ------------------------------------------------------------------------------------------------ k_prod_layer
@pytest.mark.parametrize("ninst", [1, 16])
@pytest.mark.parametrize("q", [1, 255, 256, 257, 1 << 12])
def test_prod_layer(rng, q, ninst):
    for kind in ("random", "edge"):
        if kind == "random":
            Lt, Rt = rolled(rng, 2 * q, ninst), rolled(rng, 2 * q, ninst)
        else:
            Lt, Rt = [edge_table(2 * y, 2 * q) for y in range(ninst)], [edge_table(2 * y + 1 + q % 3, 2 * q) for y in range(ninst)]
        got, _ = K.prod_layer(Lt, Rt)
        for y in range(ninst):
            a, b = orc.fr_to_ints(Lt[y]), orc.fr_to_ints(Rt[y])
            prod = orc.fr_from_ints([x * z % l for x, z in zip(a, b)])
            assert eq(got[y][0], prod[:q]) and eq(got[y][1], prod[q:]), (kind, y)


# ------------------------------------------------------------------------------------------------ k_hash_mem, k_hash_ops
def hash_scalars(rng, kind):
    r, g = {"random": (int(rng.integers(0, 2 ** 62)) ** 4 % l, int(rng.integers(0, 2 ** 62)) ** 4 % l), "l-1": (l - 1, l - 1), "0,1": (0, 1), "1,0": (1, 0)}[kind]
    return r, g


def timestamps(rng, n):
    ts = [int(x) for x in rng.integers(0, 1 << 32, n)]
    ts[:3] = [0, 1, (1 << 32) - 1][:n]
    ts[-1] = (1 << 32) - 1
    return ts


@pytest.mark.parametrize("kind", ["random", "l-1", "0,1", "1,0"])
@pytest.mark.parametrize("M", [4, 256, 1024, 1 << 13])
def test_hash_mem(rng, M, kind):
    """init[i] = eval[i] r + i - gamma, audit[i] = init[i] + ts[i] r^2 at the GLOBAL index i; a rank's output is the elements i = rk (mod G)"""
    r, g = hash_scalars(rng, kind)
    ev = orc.rand_fr(rng, M) if kind == "random" else edge_table(M % 7, M)
    ts = timestamps(rng, M)
    evi = orc.fr_to_ints(ev)
    init = [(evi[i] * r + i - g) % l for i in range(M)]
    want_i, want_a = orc.fr_from_ints(init), orc.fr_from_ints([(init[i] + ts[i] * r * r) % l for i in range(M)])
    for G in (1, 2, 4):
        if M // G < 2:
            continue
        for rk in range(G):
            gi, ga, _ = K.hash_mem(ev, orc.fr_from_ints(ts), orc.fr_from_ints([r]), orc.fr_from_ints([g]), G, rk)
            assert eq(gi, want_i[rk::G]) and eq(ga, want_a[rk::G]), (G, rk)


@pytest.mark.parametrize("kind", ["random", "l-1", "0,1", "1,0"])
@pytest.mark.parametrize("N", [4, 256, 1024, 1 << 13])
def test_hash_ops(rng, N, kind):
    """read[i] = ts[i] r^2 + deref[i] r + addr[i] - gamma, write[i] = read[i] + r^2"""
    r, g = hash_scalars(rng, kind)
    de = orc.rand_fr(rng, N) if kind == "random" else edge_table(N % 5, N)
    addr = [int(x) for x in rng.integers(0, N, N)]; addr[0], addr[-1] = 0, N - 1
    ts = timestamps(rng, N)
    dei = orc.fr_to_ints(de)
    read = [(ts[i] * r * r + dei[i] * r + addr[i] - g) % l for i in range(N)]
    want_r, want_w = orc.fr_from_ints(read), orc.fr_from_ints([(x + r * r) % l for x in read])
    for G in (1, 2, 4):
        if N // G < 2:
            continue
        for rk in range(G):
            gr, gw, _ = K.hash_ops(orc.fr_from_ints(addr), de, orc.fr_from_ints(ts), orc.fr_from_ints([r]), orc.fr_from_ints([g]), G, rk)
            assert eq(gr, want_r[rk::G]) and eq(gw, want_w[rk::G]), (G, rk)
            assert orc.fr_to_ints(gw) == [(x + r * r) % l for x in orc.fr_to_ints(gr)]


# ------------------------------------------------------------------------------------------------ k_dot_many, k_sum3, k_reduce_many
@pytest.mark.parametrize("n,count", [(1, 3), (256, 3), (257, 6), (1 << 12, 6)])
def test_dot_many_and_sum3(rng, n, count):
    for kind in ("random", "edge"):
        T = [orc.rand_fr(rng, n) for _ in range(3 * count + 1)] if kind == "random" else [edge_table(k + n % 4, n) for k in range(3 * count + 1)]
        Ti = [orc.fr_to_ints(t) for t in T]
        got, _ = K.dot_many(T[0], T[1:count + 1])
        assert eq(got, orc.fr_from_ints([sum(e * p for e, p in zip(Ti[0], Ti[1 + y])) % l for y in range(count)])), kind
        A, B, C = T[1:count + 1], T[count + 1:2 * count + 1], T[2 * count + 1:]
        got, _ = K.sum3(A, B, C)
        assert eq(got, orc.fr_from_ints([sum(a * b * c for a, b, c in zip(Ti[1 + y], Ti[count + 1 + y], Ti[2 * count + 1 + y])) % l for y in range(count)])), kind


@pytest.mark.parametrize("count", [21, 15])
def test_dot_many_and_sum3_at_the_grid_cap(rng, count):
    """2^16 elements: 256 workgroups per polynomial wanted, 2048 / 21 = 97 and 2048 / 15 = 136 given (the loop strides; k_reduce_many adds that many
    partials per polynomial).  Every table is one random block rotated, so the reference converts 2^16 elements once.  sum3 takes at most 20 triples."""
    n = 1 << 16
    blk = frand(rng, n); bi = np.array(orc.fr_to_ints(blk), dtype=object)
    E = frand(rng, n); ei = np.array(orc.fr_to_ints(E), dtype=object)
    shifts = [1 + 5 * k for k in range(count)]
    got, _ = K.dot_many(E, [np.roll(blk, s, axis=0) for s in shifts])
    assert eq(got, orc.fr_from_ints([int(np.dot(ei, np.roll(bi, s))) % l for s in shifts]))
    k3 = min(count, 20)
    A = [np.roll(blk, s, axis=0) for s in shifts[:k3]]; B = [np.roll(blk, s + 1, axis=0) for s in shifts[:k3]]; C = [np.roll(E, s, axis=0) for s in shifts[:k3]]
    got, _ = K.sum3(A, B, C)
    assert eq(got, orc.fr_from_ints([int(np.dot(np.roll(bi, s) * np.roll(bi, s + 1) % l, np.roll(ei, s))) % l for s in shifts[:k3]]))


# ------------------------------------------------------------------------------------------------ dev_poly_bound_chunks
@pytest.mark.parametrize("L,R,m", [(32, 64, 4), (128, 256, 16), (64, 64, 4), (256, 256, 16)])
def test_poly_bound_chunks(rng, L, R, m):
    """the prover's two geometries scaled down: L R = 8 N with chunks of L / 8 rows and L R = 16 N with chunks of L / 16, N = 2^8 and 2^12"""
    Z, lv = frand(rng, L * R), orc.rand_fr(rng, m)
    got = K.poly_bound_chunks(Z, L, R, lv)
    assert got is not None and got.shape[0] == L // m
    for c in range(L // m):
        assert eq(got[c], orc.poly_bound(Z[c * m * R:(c + 1) * m * R], m, R, lv)), c


def test_poly_bound_chunks_declines_chunks_smaller_than_a_slab(rng):
    """128 rows are 64 slabs of two: chunks of one row are no whole slabs, and 100 rows are no whole slabs at all — nothing is launched"""
    assert K.poly_bound_chunks(frand(rng, 128 * 8), 128, 8, orc.rand_fr(rng, 1)) is None
    assert K.poly_bound_chunks(frand(rng, 100 * 8), 100, 8, orc.rand_fr(rng, 4)) is None
