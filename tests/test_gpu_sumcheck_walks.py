"""The six sum-check round kernels (k_sumcheck.hip) where a thread walks SEVERAL items, against the oracle, bit-exact.

Each kernel is a grid-stride loop over nine-limb accumulators that are added to without reduction and carry-swept every fourth item.  The plan
(sc_plan.h) gives every item a thread of its own up to 2^18 items, so at the lengths of the other kernel-level tests the in-loop sweep never runs,
nothing is added onto an unswept accumulator and no thread meets the loop's condition twice.  Here the capacities the plan is told are replaced
(K.sc_caps) so that short tables walk 2 .. 64 items per thread — 64 is the most the plan gives any length up to 2^26 on 256 CUs — or spread over
the widest grid of 2048 workgroups, whose partial sums the last workgroup gathers eight per thread.  Every test asserts the grid and the walk it
means through K.sc_plan: a later change of the plan makes it say so instead of quietly testing one item per thread again.

Tables are (n, 32) uint8 stored words (Montgomery form as it lies in memory); kernel and oracle read the same bytes, so a corner of the limbs'
range is written as a raw word."""
import itertools

import numpy as np
import pytest

import otti_amd as oa
import orc
from test_gpu_kernels import _cubic3_want
from test_gpu_sumcheck_reduce import _only_item

pytestmark = pytest.mark.gpu
K = oa.kernels
l = orc.L_ORDER
EVALS, FOLDS = ("quad_eval", "cubic3_eval", "cubic4_eval"), ("quad_fold", "cubic3_fold", "cubic4_fold")
ONE_WORKGROUP = (1, 1)                    # num_cu, resident: one workgroup whatever the length
THREE_WORKGROUPS = (2, 3)                 # min(3 resident, 2 per CU x 2 CUs) = 3
WIDEST = (1024, 2048)                     # min(2048 resident, 2 x 1024): the 2048 rows of the partial-sum buffer


@pytest.fixture(autouse=True)
def device_caps_afterwards():
    """whatever a test did to the capacities, the next one starts from the device's own"""
    yield
    K.sc_caps_restore()


@pytest.fixture(scope="module")
def own_rng():
    return np.random.default_rng(20261020)


@pytest.fixture(scope="module")
def pool(own_rng):
    """four random tables of 2^16 elements; a test takes the first n of each (made once: rand_fr is a Python loop)"""
    return orc.rand_fr(own_rng, 4 << 16).reshape(4, 1 << 16, 32)


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def word(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8)


def expect_plan(kinds, n, workgroups, per_thread):
    for kind in kinds:
        assert K.sc_plan(kind, n) == (workgroups, per_thread), (kind, n)


def check_evals(A, B, C, D, taus, tag=None, which=EVALS):
    """quad on (A, B); cubic3 on (B, C, D) with every tau (a pair (tau, its eq table) where the caller has the table already); the four-table cubic on all"""
    if "quad_eval" in which:
        assert eq(K.sc_quad_round(A, B)[0], orc.sc_quad_evals(A, B)), (tag, "quad")
    if "cubic3_eval" in which:
        for tau in taus:
            tau, E = tau if isinstance(tau, tuple) else (tau, orc.eq_evals(tau))
            assert eq(K.sc_cubic3_round(B, C, D, tau)[0], _cubic3_want(E, B, C, D)), (tag, "cubic3")
    if "cubic4_eval" in which:
        assert eq(K.sc_cubic_round(A, B, C, D)[0], orc.sc_cubic_evals(A, B, C, D)), (tag, "cubic4")


def check_folds(A, B, C, D, r, taus, tag=None, which=FOLDS, folded=None):
    """the same three with the fold by r in front: every folded table and the sums over the folded tables"""
    fa, fb, fc, fd = folded if folded is not None else (orc.fold_top(x, r) for x in (A, B, C, D))
    if "quad_fold" in which:
        out, e, _ = K.sc_quad_fold_round(A, B, r)
        assert eq(out[0], fa) and eq(out[1], fb), (tag, "quad: folded tables")
        assert eq(e, orc.sc_quad_evals(fa, fb)), (tag, "quad")
    if "cubic3_fold" in which:
        for tau in taus:
            tau, E = tau if isinstance(tau, tuple) else (tau, orc.eq_evals(tau))
            out, e, _ = K.sc_cubic3_fold_round(B, C, D, r, tau)
            assert eq(out[0], fb) and eq(out[1], fc) and eq(out[2], fd), (tag, "cubic3: folded tables")
            assert eq(e, _cubic3_want(E, fb, fc, fd)), (tag, "cubic3")
    if "cubic4_fold" in which:
        out, e, _ = K.sc_cubic_fold_round(A, B, C, D, r)
        assert all(eq(out[k], f) for k, f in enumerate((fa, fb, fc, fd))), (tag, "cubic4: folded tables")
        assert eq(e, orc.sc_cubic_evals(fa, fb, fc, fd)), (tag, "cubic4")


def two_taus(rng, m):
    """a random tau, and the one of all (l + 1) / 2 = 1/2: a constant eq table"""
    return [orc.rand_fr(rng, m), orc.fr_from_ints([(l + 1) // 2] * m)]


# ------------------------------------------------------------------------------------------------ the seam itself
def test_caps_override_sets_the_plan_and_goes_away():
    own = [K.sc_plan(k, 1 << 20) for k in EVALS + FOLDS]
    with K.sc_caps(*ONE_WORKGROUP):
        expect_plan(EVALS, 1 << 13, 1, 16)
        expect_plan(FOLDS, 1 << 13, 1, 8)
        assert K.sc_plan("quad_fold", 1 << 20, armed=True) == (1, 1024)
    assert [K.sc_plan(k, 1 << 20) for k in EVALS + FOLDS] == own
    with K.sc_caps(256, [1024, 512, 1792, 1024, 1024, 512]):                 # six capacities by kind: rows that tests/sc_plan_check.cpp pins
        assert K.sc_plan("cubic4_fold", 1 << 22) == (512, 8) and K.sc_plan("cubic3_eval", 1 << 23) == (2048, 8)
        assert K.sc_plan("quad_fold", 1 << 18, armed=True) == (64, 4)
    with pytest.raises(RuntimeError):
        with K.sc_caps(*THREE_WORKGROUPS):
            assert K.sc_plan("quad_eval", 1 << 12) == (3, 3)
            raise RuntimeError("out of the block by an exception")
    assert [K.sc_plan(k, 1 << 20) for k in EVALS + FOLDS] == own
    for caps in [(0, 1), (1, 0), (4, [1, 1, 1, 0, 1, 1])]:
        with pytest.raises(oa.SpartanError):
            with K.sc_caps(*caps):
                pass
        assert [K.sc_plan(k, 1 << 20) for k in EVALS + FOLDS] == own         # a refused override leaves the device's own in force
    with pytest.raises(oa.SpartanError):
        K.sc_plan("quad_fold", 2)


def test_plan_of_a_2p20_proof_under_the_capacities_the_host_check_assumes():
    """the rows tests/sc_plan_check.cpp pins for a 2^20 proof, through the library's own sc_plan.  Under stated capacities, not the device's: what the
    occupancy query answers is the HIP runtime's business — asked first thing in a process it gives these rows on 256 CUs, in a process that loaded
    torch's runtime after the library it reports one resident workgroup per CU for the three largest kernels, and the plan follows (256 workgroups)"""
    with K.sc_caps(256, [1024, 512, 1792, 1024, 1024, 512]):
        assert K.sc_plan("cubic3_eval", 1 << 20) == (512, 4)
        assert K.sc_plan("cubic3_fold", 1 << 20) == (512, 2)
        assert K.sc_plan("cubic3_fold", 1 << 19) == (512, 1)
        assert K.sc_plan("cubic3_fold", 1 << 16, armed=True) == (64, 1)
        assert K.sc_plan("quad_eval", 1 << 20) == (512, 4)
        assert K.sc_plan("quad_fold", 1 << 20) == (512, 2)
        assert K.sc_plan("quad_fold", 1 << 16, armed=True) == (64, 1)
        assert K.sc_plan("cubic4_eval", 1 << 20) == (512, 4)


# ------------------------------------------------------------------------------------------------ a. one workgroup, walks of 2 .. 64 items
@pytest.mark.parametrize("walk", [2, 4, 8, 16, 64])
def test_evaluations_on_one_workgroup(own_rng, pool, walk):
    """lengths 2^10 .. 2^15; from a walk of 4 the in-loop sweep runs, at 2^15 cubic3 takes its eq factor from the product of two pyramids"""
    n = 512 * walk
    A, B, C, D = pool[:, :n]
    with K.sc_caps(*ONE_WORKGROUP):
        expect_plan(EVALS, n, 1, walk)
        check_evals(A, B, C, D, two_taus(own_rng, n.bit_length() - 2))


@pytest.mark.parametrize("walk", [2, 4, 8, 16, 64])
def test_folds_on_one_workgroup(own_rng, pool, walk):
    """lengths 2^11 .. 2^16"""
    n = 1024 * walk
    A, B, C, D = pool[:, :n]
    with K.sc_caps(*ONE_WORKGROUP):
        expect_plan(FOLDS, n, 1, walk)
        check_folds(A, B, C, D, orc.rand_fr(own_rng, 1), two_taus(own_rng, n.bit_length() - 3))


# ------------------------------------------------------------------------------------------------ b. ragged walks on three workgroups
def ragged_items(items):
    """a thread's first pass (both ends), the second, the last full pass (both ends), the partial last pass (both ends)"""
    stride = 3 * 256
    full = items // stride
    return sorted({0, stride - 1, stride, (full - 1) * stride, full * stride - 1, full * stride, items - 1})


def test_ragged_items_are_the_ones_meant():
    assert ragged_items(2048) == [0, 767, 768, 1535, 1536, 2047]
    assert ragged_items(4096) == [0, 767, 768, 3072, 3839, 3840, 4095]


@pytest.mark.parametrize("items,walk", [(2048, 3), (4096, 6)])
def test_evaluations_on_ragged_walks(own_rng, pool, items, walk):
    """2048 items on 3 x 256 threads: walks of 3 and 2, the sweep never reached; 4096: walks of 6 and 5, a sweep at four and then one or two unswept
    additions.  Random tables, and tables of ONE non-zero item: a term the stride loop skips or counts twice is then the whole sum"""
    n = 2 * items
    with K.sc_caps(*THREE_WORKGROUPS):
        expect_plan(EVALS, n, 3, walk)
        taus = [orc.rand_fr(own_rng, n.bit_length() - 2)]
        taus = [(taus[0], orc.eq_evals(taus[0]))]
        check_evals(*pool[:, :n], taus)
        for j in ragged_items(items):
            A, B, C, D = _only_item(own_rng, n, items, j, 4)
            assert any(orc.fr_to_ints(orc.sc_quad_evals(A, B))) and any(orc.fr_to_ints(orc.sc_cubic_evals(A, B, C, D)))
            check_evals(A, B, C, D, taus, tag=j)


@pytest.mark.parametrize("items,walk", [(2048, 3), (4096, 6)])
def test_folds_on_ragged_walks(own_rng, pool, items, walk):
    n = 4 * items
    with K.sc_caps(*THREE_WORKGROUPS):
        expect_plan(FOLDS, n, 3, walk)
        r = orc.rand_fr(own_rng, 1)
        taus = [orc.rand_fr(own_rng, n.bit_length() - 3)]
        taus = [(taus[0], orc.eq_evals(taus[0]))]
        check_folds(*pool[:, :n], r, taus)
        for j in ragged_items(items):
            A, B, C, D = _only_item(own_rng, n, items, j, 4)
            folded = [orc.fold_top(x, r) for x in (A, B, C, D)]
            assert any(orc.fr_to_ints(orc.sc_quad_evals(*folded[:2]))) and any(orc.fr_to_ints(orc.sc_cubic_evals(*folded)))
            check_folds(A, B, C, D, r, taus, tag=j, folded=folded)


# ------------------------------------------------------------------------------------------------ c. corners of the stored word, walks of 16 and 64
# Each half (evaluations) or quarter (folds) of a table is one word, so every item of a thread's walk pushes its accumulators the same way.
# The limbs see the stored word: l - 1 as a WORD is the largest a table holds (the integer l - 1 is stored as the small word 16 (l - 2^252)).
HALVES = [(0, 0), (0, 1), (1, 0), (1, 1)]                                      # which halves hold the corner word (else 0)
QUARTERS = [(0, 0, 1, 1), (1, 1, 0, 0), (0, 1, 1, 0), (1, 0, 0, 1)]
_PIECES = {}


def pieces(n, patterns, m=l - 1):
    """the tables of length n whose halves / quarters hold the word m where the pattern says so, made once"""
    key = (n, len(patterns[0]), m)
    if key not in _PIECES:
        rows = np.stack([word(0), word(m)])
        _PIECES[key] = [np.repeat(rows[list(p)], n // len(p), axis=0) for p in patterns]
    return _PIECES[key]


_FOLDED = {}


def folded_piece(n, k, r_word, m=l - 1):
    key = (n, k, r_word, m)
    if key not in _FOLDED:
        _FOLDED[key] = orc.fold_top(pieces(n, QUARTERS, m)[k], word(r_word).reshape(1, 32))
    return _FOLDED[key]


def corner_tau(n_vars):
    return orc.rand_fr(np.random.default_rng(7 + n_vars), n_vars)                # one tau (and one eq table) per length, whichever test asks first


_TAUS = {}


def tau_and_table(n_vars):
    if n_vars not in _TAUS:
        tau = corner_tau(n_vars)
        _TAUS[n_vars] = (tau, orc.eq_evals(tau))
    return _TAUS[n_vars]


@pytest.mark.parametrize("walk", [16, 64])
def test_corner_words_quad_and_cubic3_evaluations(walk):
    """every assignment of {0, l - 1} (stored) to the halves: 16 cases for quad, 64 for cubic3 with a random tau"""
    n = 512 * walk
    P = pieces(n, HALVES); taus = [tau_and_table(n.bit_length() - 2)]
    with K.sc_caps(*ONE_WORKGROUP):
        expect_plan(EVALS, n, 1, walk)
        for a, b in itertools.product(range(4), repeat=2):
            check_evals(P[a], P[b], None, None, taus, tag=(a, b), which=("quad_eval",))
        for b, c, d in itertools.product(range(4), repeat=3):
            check_evals(None, P[b], P[c], P[d], taus, tag=(b, c, d), which=("cubic3_eval",))


@pytest.mark.parametrize("a", range(4))
@pytest.mark.parametrize("walk", [16, 64])
def test_corner_words_cubic4_evaluation(walk, a):
    """256 cases a walk, 64 per value of `a` (the halves of the first table).  The third accumulator of a walk of 64 passes 2^261 here (fr9_canon's range)"""
    n = 512 * walk
    P = pieces(n, HALVES)
    with K.sc_caps(*ONE_WORKGROUP):
        expect_plan(("cubic4_eval",), n, 1, walk)
        for b, c, d in itertools.product(range(4), repeat=3):
            check_evals(P[a], P[b], P[c], P[d], (), tag=(a, b, c, d), which=("cubic4_eval",))


@pytest.mark.parametrize("r_word", [l - 1, 1], ids=["r=l-1", "r=1"])
@pytest.mark.parametrize("walk", [16, 64])
def test_corner_words_quad_and_cubic3_folds(walk, r_word):
    """each table one of four quarter patterns of {0, l - 1}, folded by the stored words l - 1 and 1: 16 / 64 cases"""
    n = 1024 * walk
    P = pieces(n, QUARTERS); F = [folded_piece(n, k, r_word) for k in range(4)]
    r = word(r_word).reshape(1, 32); taus = [tau_and_table(n.bit_length() - 3)]
    with K.sc_caps(*ONE_WORKGROUP):
        expect_plan(FOLDS, n, 1, walk)
        for a, b in itertools.product(range(4), repeat=2):
            check_folds(P[a], P[b], None, None, r, taus, tag=(a, b), which=("quad_fold",), folded=(F[a], F[b], None, None))
        for b, c, d in itertools.product(range(4), repeat=3):
            check_folds(None, P[b], P[c], P[d], r, taus, tag=(b, c, d), which=("cubic3_fold",), folded=(None, F[b], F[c], F[d]))


@pytest.mark.parametrize("r_word", [l - 1, 1], ids=["r=l-1", "r=1"])
@pytest.mark.parametrize("a", range(4))
@pytest.mark.parametrize("walk", [16, 64])
def test_corner_words_cubic4_fold(walk, a, r_word):
    n = 1024 * walk
    P = pieces(n, QUARTERS); F = [folded_piece(n, k, r_word) for k in range(4)]
    r = word(r_word).reshape(1, 32)
    with K.sc_caps(*ONE_WORKGROUP):
        expect_plan(("cubic4_fold",), n, 1, walk)
        for b, c, d in itertools.product(range(4), repeat=3):
            check_folds(P[a], P[b], P[c], P[d], r, (), tag=(a, b, c, d), which=("cubic4_fold",), folded=(F[a], F[b], F[c], F[d]))


@pytest.mark.parametrize("m", [1, (1 << 252) - 1, 1 << 232, (1 << 29) - 1], ids=["1", "2^252-1", "2^232", "2^29-1"])
@pytest.mark.parametrize("walk", [16, 64])
def test_other_corner_words_on_alternating_halves(walk, m):
    """other words in the place of l - 1 — the smallest, every limb full, the top limb's lowest bit alone, the lowest limb full — with the tables'
    halves (quarters) alternating from one table to the next; all six kernels, the folds by the word itself and by 1"""
    with K.sc_caps(*ONE_WORKGROUP):
        n = 512 * walk
        expect_plan(EVALS, n, 1, walk)
        P = pieces(n, HALVES, m)
        check_evals(P[1], P[2], P[1], P[2], [tau_and_table(n.bit_length() - 2)], tag="evaluate")
        n = 1024 * walk
        expect_plan(FOLDS, n, 1, walk)
        P = pieces(n, QUARTERS, m)
        for r_word in (m, 1):
            F = [folded_piece(n, k, r_word, m) for k in range(4)]
            check_folds(P[2], P[3], P[2], P[3], word(r_word).reshape(1, 32), [tau_and_table(n.bit_length() - 3)], tag=("fold by", r_word), folded=(F[2], F[3], F[2], F[3]))


# ------------------------------------------------------------------------------------------------ d. the widest grid: 2048 workgroups, an item each thread
# The last workgroup gathers the 2048 partial sums eight per thread (finish_in_kernel: b = threadIdx.x, + 256, ...): the item sits in workgroups at
# both ends of a thread's eight and in the last slot of all.  Tables are zeros plus one item's rows (rand_fr at this length would be a Python loop).
@pytest.fixture(scope="module")
def wide_tau():
    tau = orc.rand_fr(np.random.default_rng(19), 19)
    return tau, orc.eq_evals(tau)


def one_item(rng, n, pieces_per_table, j, count):
    out = []
    for _ in range(count):
        t = np.zeros((n, 32), dtype=np.uint8)
        t[j::n // pieces_per_table] = orc.rand_fr(rng, pieces_per_table)
        out.append(t)
    return out


@pytest.mark.parametrize("workgroup,thread", [(0, 0), (255, 255), (256, 0), (1023, 100), (2047, 255)])
def test_one_item_on_the_widest_grid(own_rng, wide_tau, workgroup, thread):
    n = 1 << 20
    with K.sc_caps(*WIDEST):
        expect_plan(("quad_eval", "cubic3_eval"), n, 2048, 1)
        A, B, C = one_item(own_rng, n, 2, 256 * workgroup + thread, 3)
        want2, want3 = orc.sc_quad_evals(A, B), _cubic3_want(wide_tau[1], A, B, C)
        assert any(orc.fr_to_ints(want2)) and any(orc.fr_to_ints(want3))
        assert eq(K.sc_quad_round(A, B)[0], want2)
        assert eq(K.sc_cubic3_round(A, B, C, wide_tau[0])[0], want3)


def test_one_item_fold_on_the_widest_grid(own_rng):
    n = 1 << 21
    with K.sc_caps(*WIDEST):
        expect_plan(("quad_fold",), n, 2048, 1)
        r = orc.rand_fr(own_rng, 1)
        for workgroup, thread in [(300, 7), (2047, 255)]:
            A, B = one_item(own_rng, n, 4, 256 * workgroup + thread, 2)
            fa, fb = orc.fold_top(A, r), orc.fold_top(B, r)
            want = orc.sc_quad_evals(fa, fb)
            assert any(orc.fr_to_ints(want))
            out, e, _ = K.sc_quad_fold_round(A, B, r)
            assert eq(out[0], fa) and eq(out[1], fb) and eq(e, want), workgroup


# ------------------------------------------------------------------------------------------------ e. the device's own plan at 2^20
@pytest.fixture(scope="module")
def cyclic_tables(own_rng):
    """a random block of 1021 elements repeated to 2^20: 1021 is prime, so the items the stride puts on one thread differ"""
    blocks = orc.rand_fr(own_rng, 4 * 1021).reshape(4, 1021, 32)
    return [np.resize(b, (1 << 20, 32)) for b in blocks]


def test_evaluations_under_the_devices_own_plan(own_rng, cyclic_tables):
    n = 1 << 20
    for kind in EVALS:
        assert K.sc_plan(kind, n)[1] >= 2, kind
    check_evals(*cyclic_tables, [orc.rand_fr(own_rng, 19)])


def test_folds_under_the_devices_own_plan(own_rng, cyclic_tables):
    n = 1 << 20
    for kind in FOLDS:
        assert K.sc_plan(kind, n)[1] >= 2, kind
    check_folds(*cyclic_tables, orc.rand_fr(own_rng, 1), [orc.rand_fr(own_rng, 18)])
