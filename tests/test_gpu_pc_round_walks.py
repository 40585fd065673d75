"""The batched sum-check round kernel (k_snark.hip k_pc_round) where a thread walks MANY items, against the oracle and closed forms, bit-exact.

The kernel is a grid-stride loop over three nine-limb accumulators per thread that are added to without reduction, carry-swept every fourth item,
folded back below 2 l every kPcWalkMax = 256 items (pc_accum9.h pc_acc_step) and made canonical once at the end.  Its grid (pc_plan.h pc_round_grid:
min(ceil(items / 256), 2048 / ninst) workgroups per instance) does not grow with the tables, so a thread's walk does: 19 items for the 18-instance
layer of a 2^20 proof, 1160 at the longest tables the library accepts.  The other kernel-level tests give it at most two.  Here the block cap is
replaced (K.pc_grid_cap) so that short tables walk 2 .. 1024 items per thread; every test asserts the grid and the walk it means through K.pc_plan,
so a later change of the rule says so instead of quietly testing one item per thread again.

The corner (section c).  tests/pc_accum_check.cpp walks the same accumulation on the host beside exact integers, over every assignment of the stored
words {0, 1, l - 1, 2^252 - 1, 2^232, 2^29 - 1} to the halves of the tables: limb 8 of a triple's third sum, only swept and never folded, first
wraps after 596 items with A (0, l - 1), B (0, l - 1), C (2^232, l - 1) as (lower, upper) stored words — WORST below (an earlier, narrower search
gave 632 with (1, 2^252 - 1) in every table; that assignment and (0, l - 1) everywhere, 644, are walked too); a product circuit's after 3736.
Before the fold was added to the step, six cases of section c failed on the device, each with a triple's "sums of instance" wrong: the evaluation at
a walk of 1024, three of the four folds at 1024 (quarters (0, 0, lo, hi) folded by l - 1, (lo, hi, lo, hi) by 1 and by l - 1), the 683-item walk on
three workgroups and the corner triple between random product circuits; every walk up to 256 passed, and so did the product circuits.

Tables are (n, 32) uint8 stored words (Montgomery form as it lies in memory); kernel and references read the same bytes."""
import itertools

import numpy as np
import pytest

import otti_amd as oa
import orc
from test_gpu_snark_kernels import check_pc_round, edge_table, frand, make_batch, rolled, want_sums
from test_gpu_sumcheck_reduce import _only_item
from test_gpu_sumcheck_walks import ragged_items

pytestmark = pytest.mark.gpu
K = oa.kernels
l = orc.L_ORDER
OWN_CAP = 2048
W252 = (1 << 252) - 1
WORST = ((0, l - 1), (0, l - 1), (1 << 232, l - 1))            # tests/test_pc_accum_host.py WORST_TRIPLE
ISSUE_632 = ((1, W252),) * 3
ALL_TOP = ((0, l - 1),) * 3


@pytest.fixture(autouse=True)
def device_cap_afterwards():
    """whatever a test did to the block cap, the next one starts from the device's own"""
    yield
    K.pc_grid_cap_restore()


@pytest.fixture(scope="module")
def own_rng():
    return np.random.default_rng(20261021)


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def word(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8)


_VAL = {}


def val(w):
    """the field element a stored word stands for"""
    if w not in _VAL:
        _VAL[w] = orc.fr_to_ints(word(w).reshape(1, 32))[0]
    return _VAL[w]


def pieces_table(n, words):
    """n elements in len(words) equal pieces, piece k all the stored word words[k]"""
    return np.repeat(np.stack([word(w) for w in words]), n // len(words), axis=0)


def half_tau(m):
    """(l + 1) / 2 = 1/2 in every variable: the eq table is the constant 2^-m"""
    return orc.fr_from_ints([(l + 1) // 2] * m)


def closed_sums(items, halves, triple):
    """sums at t = 0, 2, 3 of an instance whose tables hold the VALUES halves[k] = (lower, upper) throughout: a triple's items . A(t) B(t) C(t);
    a product circuit's, under the constant eq table 2^-m over items = 2^m, A(t) B(t).  X(t) = x_lo + t (x_hi - x_lo)"""
    out = []
    for t in (0, 2, 3):
        p = items % l if triple else 1
        for lo, hi in halves:
            p = p * (lo + t * (hi - lo)) % l
        out.append(p)
    return orc.fr_from_ints(out)


def fold_values(quarters, r):
    """(lower, upper) values of a table of four constant quarters folded by the value r"""
    x0, x1, x2, x3 = quarters
    return (x0 + r * (x2 - x0)) % l, (x1 + r * (x3 - x1)) % l


def run_corners(walk, cases, r_word=None, workgroups=1, items=None, oracle=False):
    """one launch over the batch `cases`: (kind 'p' / 't', per table the stored words of its halves — quarters with a fold), 256 * walk items on one
    workgroup per instance unless told otherwise.  Sums (and folded tables) against the closed forms; oracle=True: against orc as well"""
    pieces = 2 if r_word is None else 4
    items = 256 * walk if items is None else items
    n = pieces * items
    A, B, C = [], [], []
    for kind, tabs in cases:
        assert len(tabs) == (3 if kind == "t" else 2) and all(len(t) == pieces for t in tabs)
        A.append(pieces_table(n, tabs[0])); B.append(pieces_table(n, tabs[1])); C.append(pieces_table(n, tabs[2]) if kind == "t" else None)
    tau = half_tau(items.bit_length() - 1)
    r = None if r_word is None else word(r_word).reshape(1, 32)
    with K.pc_grid_cap(workgroups * len(cases)):
        assert K.pc_plan(len(cases), items) == (workgroups, walk)
        e, folded, _ = K.pc_round(A, B, C, tau, r)
        if oracle:
            check_pc_round(A, B, C, tau, r)
    for y, (kind, tabs) in enumerate(cases):
        if r is None:
            halves = [(val(t[0]), val(t[1])) for t in tabs]
        else:
            halves = [fold_values([val(w) for w in t], val(r_word)) for t in tabs]
            for k, h in enumerate(halves):
                assert eq(folded[k][y], np.repeat(orc.fr_from_ints(list(h)), n // 4, axis=0)), ("folded table", k, "of instance", y, kind, tabs)
        assert eq(e[y], closed_sums(items, halves, kind == "t")), ("sums of instance", y, kind, tabs, "walk", walk, "fold by", r_word)


# ------------------------------------------------------------------------------------------------ the seam itself
def test_grid_cap_sets_the_plan_and_goes_away():
    rows = [(1, 1 << 20), (18, 1 << 19), (20, 1 << 19), (18, 1 << 15)]
    own = [K.pc_plan(*row) for row in rows]
    assert own == [(2048, 2), (113, 19), (102, 21), (113, 2)]                    # rows tests/pc_plan_check.cpp pins
    with K.pc_grid_cap(18):
        assert K.pc_plan(18, 256 * 64) == (1, 64) and K.pc_plan(18, 1 << 18) == (1, 1024)
    assert [K.pc_plan(*row) for row in rows] == own
    with K.pc_grid_cap(6):
        assert K.pc_plan(2, 2048) == (3, 3) and K.pc_plan(2, 4096) == (3, 6)
    with K.pc_grid_cap(1):                                                       # a cap below the instances still gives each its workgroup
        assert K.pc_plan(18, 1 << 12) == (1, 16)
    assert [K.pc_plan(*row) for row in rows] == own
    with pytest.raises(RuntimeError):
        with K.pc_grid_cap(3):
            assert K.pc_plan(1, 1 << 19) == (3, 683)
            raise RuntimeError("out of the block by an exception")
    assert [K.pc_plan(*row) for row in rows] == own
    with pytest.raises(oa.SpartanError):                                         # the partial sums' buffers end at the device's own cap
        with K.pc_grid_cap(OWN_CAP + 1):
            pass
    assert [K.pc_plan(*row) for row in rows] == own
    with K.pc_grid_cap(0):                                                       # 0: the device's own
        assert [K.pc_plan(*row) for row in rows] == own
    for bad in [(0, 4), (65, 4), (1, 0)]:
        with pytest.raises(oa.SpartanError):
            K.pc_plan(*bad)


# ------------------------------------------------------------------------------------------------ a. one workgroup per instance, walks of 2 .. 64 items
def batches_at(walk):
    return ["p", "t", "ptpp"] + (["ppt" * 6] if walk in (4, 16) else [])


@pytest.mark.parametrize("walk", [2, 4, 8, 16, 64])
def test_evaluations_on_one_workgroup(own_rng, walk):
    """tables of 2^10 .. 2^15 elements; from a walk of 4 the in-loop sweep runs, at 2^15 the eq factor is the product of two pyramids"""
    n = 512 * walk
    tau = orc.rand_fr(own_rng, (n // 2).bit_length() - 1)
    for kinds in batches_at(walk):
        with K.pc_grid_cap(len(kinds)):
            assert K.pc_plan(len(kinds), n // 2) == (1, walk), kinds
            check_pc_round(*make_batch(kinds, iter(rolled(own_rng, n, 3 * len(kinds)))), tau)


@pytest.mark.parametrize("walk", [2, 4, 8, 16, 64])
def test_folds_on_one_workgroup(own_rng, walk):
    """tables of 2^11 .. 2^16 elements"""
    n = 1024 * walk
    tau = orc.rand_fr(own_rng, (n // 4).bit_length() - 1)
    for kinds in batches_at(walk):
        with K.pc_grid_cap(len(kinds)):
            assert K.pc_plan(len(kinds), n // 4) == (1, walk), kinds
            check_pc_round(*make_batch(kinds, iter(rolled(own_rng, n, 3 * len(kinds)))), tau, orc.rand_fr(own_rng, 1))


# ------------------------------------------------------------------------------------------------ b. ragged walks on three workgroups per instance
@pytest.mark.parametrize("fold", [False, True], ids=["evaluate", "fold"])
@pytest.mark.parametrize("items,walk", [(2048, 3), (4096, 6)])
def test_ragged_walks(own_rng, items, walk, fold):
    """2048 items on 3 x 256 threads: walks of 3 and 2, the sweep never reached; 4096: walks of 6 and 5, a sweep at four and then one or two unswept
    additions.  Random tables, and tables of ONE non-zero item: a term the stride loop skips or counts twice is then the whole sum"""
    kinds, pieces = "pt", 4 if fold else 2
    n = pieces * items
    tau = orc.rand_fr(own_rng, items.bit_length() - 1); E = orc.eq_evals(tau)
    r = orc.rand_fr(own_rng, 1) if fold else None
    with K.pc_grid_cap(3 * len(kinds)):
        assert K.pc_plan(len(kinds), items) == (3, walk)
        check_pc_round(*make_batch(kinds, iter(rolled(own_rng, n, 5))), tau, r)
        for j in ragged_items(items):
            A, B, C = make_batch(kinds, iter(_only_item(own_rng, n, items, j, 5)))
            for y in range(len(kinds)):
                a, b, c = (None if t is None else (orc.fold_top(t, r) if fold else t) for t in (A[y], B[y], C[y]))
                assert any(orc.fr_to_ints(want_sums(E, a, b, c))), (j, y)
            check_pc_round(A, B, C, tau, r)


# ------------------------------------------------------------------------------------------------ c. corner words, constant halves / quarters
# Every item of a thread's walk pushes its sums the same way.  The limbs see the stored word: l - 1 as a WORD is the largest a table holds.
HALVES = [(0, 0), (0, l - 1), (l - 1, 0), (l - 1, l - 1)]
QUARTERS = [(0, 0, l - 1, l - 1), (l - 1, l - 1, 0, 0), (0, l - 1, l - 1, 0), (l - 1, 0, 0, l - 1)]


def every_assignment(patterns):
    """64 triples and 16 product circuits, in batches of at most 20 instances"""
    cases = [("t", tabs) for tabs in itertools.product(patterns, repeat=3)] + [("p", tabs) for tabs in itertools.product(patterns, repeat=2)]
    return [cases[k:k + 20] for k in range(0, len(cases), 20)]


@pytest.mark.parametrize("walk", [16, 64])
def test_every_assignment_of_the_largest_word_evaluation(walk):
    """every assignment of {0, l - 1} (stored) to the halves of the two or three tables; at a walk of 16 the closed form is held to the oracle too"""
    for batch in every_assignment(HALVES):
        run_corners(walk, batch, oracle=walk == 16)


@pytest.mark.parametrize("r_word", [l - 1, 1], ids=["r=l-1", "r=1"])
@pytest.mark.parametrize("walk", [16, 64])
def test_every_assignment_of_the_largest_word_fold(walk, r_word):
    """each table one of four quarter patterns of {0, l - 1}, folded by the stored words l - 1 and 1"""
    for batch in every_assignment(QUARTERS):
        run_corners(walk, batch, r_word=r_word, oracle=walk == 16)


def long_walk_batch(quarters=None):
    """the three corner assignments as triples, and the first two tables of each as product circuits; quarters: how a (lower, upper) pair becomes the
    four quarters of a table that is folded"""
    shape = (lambda h: h) if quarters is None else quarters
    triples = [("t", tuple(shape(h) for h in tabs)) for tabs in (WORST, ISSUE_632, ALL_TOP)]
    return triples + [("p", tabs[:2]) for _, tabs in triples]


@pytest.mark.parametrize("walk", [16, 256, 1024])
def test_long_walks_on_corner_words_evaluation(walk):
    """the assignment the host check found, (1, 2^252 - 1) and (0, l - 1) in all tables: tables of up to 2^19 elements on one workgroup per instance.
    A walk of 1024 passes the 596 / 632 / 644 items at which limb 8 of these triples' third sum would wrap if nothing folded it back"""
    run_corners(walk, long_walk_batch(), oracle=walk == 16)


@pytest.mark.parametrize("r_word", [1, l - 1], ids=["r=1", "r=l-1"])
@pytest.mark.parametrize("shape", ["0,0,lo,hi", "lo,hi,lo,hi"])
@pytest.mark.parametrize("walk", [16, 256, 1024])
def test_long_walks_on_corner_words_fold(walk, shape, r_word):
    """the same with a fold in front, tables of up to 2^20 elements: quarters (0, 0, lower, upper) — a fold by the stored word 1 hands the corner
    on as it is, one by l - 1 a multiple of it — and (lower, upper, lower, upper), which any fold leaves in place (as fold9's output, not the
    canonical word: below 1.2 l)"""
    quarters = (lambda h: (0, 0, h[0], h[1])) if shape == "0,0,lo,hi" else (lambda h: (h[0], h[1], h[0], h[1]))
    run_corners(walk, long_walk_batch(quarters), r_word=r_word, oracle=walk == 16)


def test_walks_of_683_items_on_three_workgroups():
    """2^19 items on 3 x 256 threads: walks of 683 and 682, two folds and an unswept tail"""
    run_corners(683, [("t", WORST), ("p", WORST[:2])], workgroups=3, items=1 << 19)


def test_a_corner_triple_between_random_product_circuits(own_rng):
    """batch "ptp" at a walk of 1024: the triple holds the corner, the product circuits random tables — the sums of every instance"""
    walk = 1024; items = 256 * walk; n = 2 * items
    R = rolled(own_rng, n, 4)
    A = [R[0], pieces_table(n, WORST[0]), R[2]]; B = [R[1], pieces_table(n, WORST[1]), R[3]]; C = [None, pieces_table(n, WORST[2]), None]
    tau = orc.rand_fr(own_rng, items.bit_length() - 1); E = orc.eq_evals(tau)
    with K.pc_grid_cap(3):
        assert K.pc_plan(3, items) == (1, walk)
        e, _, _ = K.pc_round(A, B, C, tau)
    for y in (0, 2):
        assert eq(e[y], want_sums(E, A[y], B[y], None)), ("sums of instance", y, "product circuit")
    assert eq(e[1], closed_sums(items, [(val(lo), val(hi)) for lo, hi in WORST], True)), ("sums of instance", 1, "triple")


# ------------------------------------------------------------------------------------------------ d. k_dot_many / k_sum3 under the same seam
@pytest.mark.parametrize("kind", ["random", "edge"])
def test_dot_many_and_sum3_walk_64_items(own_rng, kind):
    """one workgroup per polynomial over 2^14 elements.  Their sums are canonical at every step: this pins the stride loop alone"""
    n, count = 1 << 14, 3
    T = [frand(own_rng, n) for _ in range(3 * count + 1)] if kind == "random" else [edge_table(k, n) for k in range(3 * count + 1)]
    Ti = [orc.fr_to_ints(t) for t in T]
    with K.pc_grid_cap(count):
        assert K.pc_plan(count, n) == (1, 64)
        got, _ = K.dot_many(T[0], T[1:count + 1])
        assert eq(got, orc.fr_from_ints([sum(e * p for e, p in zip(Ti[0], Ti[1 + y])) % l for y in range(count)]))
        A, B, C = T[1:count + 1], T[count + 1:2 * count + 1], T[2 * count + 1:]
        got, _ = K.sum3(A, B, C)
        assert eq(got, orc.fr_from_ints([sum(a * b * c for a, b, c in zip(Ti[1 + y], Ti[count + 1 + y], Ti[2 * count + 1 + y])) % l for y in range(count)]))


# ------------------------------------------------------------------------------------------------ e. the library's own cap
def test_evaluation_under_the_librarys_own_cap(own_rng):
    """"ppt" x 6 at 2^17 elements: 2^16 items per instance on the 113 workgroups 2048 / 18 gives"""
    kinds, n = "ppt" * 6, 1 << 17
    workgroups, walk = K.pc_plan(len(kinds), n // 2)
    assert workgroups == 113 and walk >= 2
    check_pc_round(*make_batch(kinds, iter(rolled(own_rng, n, 3 * len(kinds)))), orc.rand_fr(own_rng, 16))
