"""otti_nizk_prove_many on the GPU, held against otti_nizk_prove_resident item by item: the seven witnesses of prove_many_cases.py (kept rows, kept
products, both, neither; unsatisfiable, all-zero, replaced inputs) at 2^6 and 2^12 uniform and on a compiler-like 2^12 instance (a constraint row of
some two hundred entries — the segmented kernels — and small values — the work-list MSM).  The front half's kernels themselves:
test_gpu_multiply_vec_many.py, test_gpu_prove_front.py."""
import threading

import pytest

import otti_amd as oa
import prove_many_cases as pm

pytestmark = pytest.mark.gpu
LABEL = pm.LABEL


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(scope="module")
def cases():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OTTI_MSM_WINDOW", "10")                     # narrow generator tables: tens of MB, built in milliseconds
        yield {name: pm.Case(name) for name in pm.INSTANCES}


@pytest.fixture(params=list(pm.INSTANCES))
def case(cases, request):
    return cases[request.param]


def test_the_cases_are_what_they_claim(cases):
    c = cases["compiler-like-2^12"]
    info = c.inst.device_info()
    assert info["n_heavy"] >= 1 and info["use_small"], info                         # a long row, coefficient codes
    assert all(x.inst.device_info()["quad"] == x.quad for x in cases.values())      # the layout the front-half rule asks about
    assert c.wits[0].info[2] > 0.25 and cases["uniform-2^12"].wits[0].info[2] < 0.25   # small values: the other MSM variant
    for c in cases.values():
        assert len(set(c.singles)) == 7
        assert c.wits[1].rows_info()[0] and c.wits[2].products_info()["kept"] and c.wits[3].rows_info()[0] and c.wits[3].products_info()["kept"]
        assert c.wits[4].check_sat(c.inst).n_unsat > 0 and c.wits[0].check_sat(c.inst).n_unsat == 0


# ---- (a) the bytes are the single prover's, (c) the front half served whom the plan says, (d) the handles are as before
@pytest.mark.parametrize("threads", [0, 1, 3])
def test_bytes_are_the_single_provers(case, threads):
    before = case.state()
    proofs, codes, info = case.many(threads=threads)
    print(case.name, threads, info)
    assert codes == [0] * 7
    case.assert_bytes(proofs)
    assert info["chunks"] == 1 and info["front_failed"] == 0 and info["workers"] == (1 if threads == 1 else 4 if threads == 0 else 3)
    assert (info["products_from_front"], info["rows_from_front"]) == case.from_front()
    assert info["product_tiles"] == (2 if case.quad else 0) and 1 <= info["row_jobs"] <= 2
    assert all(set(p.stage_ms) == set(oa.api.STAGES) and p.stage_ms["total"] > 0 for p in proofs)
    assert case.state() == before


def test_reversed_list_list_of_one_and_one_handle_twice(case):
    order = list(range(7))[::-1]
    proofs, codes, _ = case.many(order)
    assert codes == [0] * 7
    case.assert_bytes(proofs, order)
    for k in (0, 3, 5):
        proofs, codes, info = case.many([k])
        assert codes == [0] and info["workers"] == 1 and info["products_from_front"] == 0 and info["rows_from_front"] == 0
        case.assert_bytes(proofs, [k])
    # one handle twice, with two seeds: the seeds of witnesses 1 and 6
    proofs = oa.NIZK.prove_many(case.inst, [case.wits[0], case.wits[0]], case.gens, LABEL, seeds=[pm.seed(0), pm.seed(5)])
    assert proofs[0].bytes == case.singles[0]
    assert proofs[1].bytes == oa.NIZK.prove(case.inst, case.wits[0], None, case.gens, LABEL, pm.seed(5)).bytes != proofs[0].bytes


def test_with_the_rule_set_aside_both_passes_run_everywhere(case, monkeypatch):
    """OTTI_PROVE_MANY_RULE=0: the product tiles on the row-per-lane instances as well — five witnesses, a tile of four and a tile of one"""
    monkeypatch.setenv("OTTI_PROVE_MANY_RULE", "0")
    before = case.state()
    proofs, codes, info = case.many(threads=3)
    assert codes == [0] * 7 and info["product_tiles"] == 2 and info["front_failed"] == 0
    assert (info["products_from_front"], info["rows_from_front"]) == case.from_front(rule=False) == (5, 5)
    case.assert_bytes(proofs)
    assert case.state() == before


# ---- (b) the verifier's view
def test_verify_many_accepts_the_satisfying_ones(case):
    proofs = case.many(details=False)
    codes = oa.NIZK.verify_many(case.inst, proofs, case.item_inputs, case.gens, LABEL)
    assert [codes[k] for k in pm.SATISFYING] == [0] * 4 and codes[pm.UNSATISFIABLE] != 0
    for k in (5, 6):                                               # whatever the single proof of these earns
        assert codes[k] == oa.NIZK.verify_many(case.inst, [case.singles[k]], case.item_inputs[k], case.gens, LABEL)[0]


# ---- (c) without a front half
@pytest.mark.parametrize("switch", ["OTTI_PROVE_MANY_FRONT=0", "OTTI_PROVE_MANY_GB=0", "OTTI_PROVE_MANY_GB=0.001"])
def test_without_the_front_half_the_bytes_are_the_same(case, switch, monkeypatch):
    """0.001 GiB = 1 073 741 bytes.  On the compiler-like instance at 2^12 (N = V = 4096, L = 64) one tile alone is 4 * 2V * 32 = 1 048 576 bytes and a
    witness's products 96 N = 393 216: no two witnesses lacking products fit, and cut where they would meet, no chunk has two witnesses lacking rows
    either (witness 3, the only one that keeps products and lacks rows, shares its chunk with 2 and 4, which keep theirs): nothing runs jointly.  On
    the uniform instances only rows are summed jointly (prove_many.cpp front_rule), 128 L + 32 V = 139 264 bytes per witness at 2^12 and 3 072 at
    2^6: the five that lack rows fit, and the joint job runs as ever."""
    name, value = switch.split("=")
    monkeypatch.setenv(name, value)
    proofs, codes, info = case.many()
    print(case.name, switch, info)
    assert codes == [0] * 7
    case.assert_bytes(proofs)
    fits = switch == "OTTI_PROVE_MANY_GB=0.001" and not case.quad
    assert (info["products_from_front"], info["rows_from_front"]) == (case.from_front() if fits else (0, 0))
    assert (info["product_tiles"] + info["row_jobs"] > 0) == fits and info["front_failed"] == 0


# ---- (e) one item's failure is its own
def test_a_witness_of_other_dimensions_in_the_middle(cases, case):
    stranger = cases["uniform-2^6" if case.name != "uniform-2^6" else "uniform-2^12"].wits[0]
    wits = case.wits[:3] + [stranger] + case.wits[3:]
    proofs, codes, info = oa.NIZK.prove_many(case.inst, wits, case.gens, LABEL, seeds=[pm.seed(k) for k in (0, 1, 2, 0, 3, 4, 5, 6)], details=True)
    assert codes == [0, 0, 0, pm.INVALID_NUM_VARS, 0, 0, 0, 0] and proofs[3] is None       # (n_failed == 1: prove_many itself asserts the count)
    case.assert_bytes(proofs[:3] + proofs[4:])
    assert (info["products_from_front"], info["rows_from_front"]) == case.from_front()


# ---- (f) more than a chunk; the joint job that crosses into the bulk kernel
def test_eighteen_witnesses_are_two_chunks(cases):
    c = cases["uniform-2^6"]
    order = ([0, 4, 5, 6] * 5)[:18]                                # none of them keeps anything
    before = c.state()
    proofs, codes, info = c.many(order, threads=4)
    assert codes == [0] * 18 and info["chunks"] == 2 and info["row_jobs"] >= 2 and info["product_tiles"] == 0 and info["front_failed"] == 0
    assert (info["products_from_front"], info["rows_from_front"]) == (0, 18)        # (row per lane: the products are each proof's own)
    c.assert_bytes(proofs, order)
    assert c.state() == before


def test_eighteen_witnesses_with_the_rule_set_aside(cases, monkeypatch):
    monkeypatch.setenv("OTTI_PROVE_MANY_RULE", "0")
    c = cases["uniform-2^6"]
    order = ([0, 4, 5, 6] * 5)[:18]
    proofs, codes, info = c.many(order, threads=4)
    assert codes == [0] * 18 and info["chunks"] == 2 and info["product_tiles"] == 4 + 1 and (info["products_from_front"], info["rows_from_front"]) == (18, 18)
    c.assert_bytes(proofs, order)


def test_sixteen_witnesses_at_2_12_sum_their_rows_in_the_bulk_kernel(cases):
    c = cases["uniform-2^12"]
    seeds = [bytes([100 + k]) * 32 for k in range(16)]
    proofs, codes, info = oa.NIZK.prove_many(c.inst, [c.wits[0]] * 16, c.gens, LABEL, seeds=seeds, threads=4, details=True)
    print(info)
    assert codes == [0] * 16 and info["chunks"] == 1 and info["row_jobs"] == 1 and info["row_kernel"] == ["bulk"] and info["product_tiles"] == 0
    assert (info["products_from_front"], info["rows_from_front"]) == (0, 16)
    for k in (0, 7, 15):
        assert proofs[k].bytes == oa.NIZK.prove(c.inst, c.wits[0], None, c.gens, LABEL, seeds[k]).bytes


# ---- (g) two caller threads on the same handles
def test_two_caller_threads_on_the_same_handles(case):
    got = [None, None]

    def call(k):
        got[k] = case.many(range(7) if k == 0 else range(6, -1, -1), threads=2)

    th = [threading.Thread(target=call, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] is not None and got[1] is not None
    assert got[0][1] == [0] * 7 and got[1][1] == [0] * 7
    case.assert_bytes(got[0][0])
    case.assert_bytes(got[1][0], range(6, -1, -1))


# ---- (h) no seed: OS entropy
def test_a_null_seed_gives_a_proof_that_verifies(case):
    a = oa.NIZK.prove_many(case.inst, case.wits[:2], case.gens, LABEL)
    b = oa.NIZK.prove_many(case.inst, case.wits[:2], case.gens, LABEL, seeds=[None, pm.seed(1)])
    assert a[0].bytes != b[0].bytes and b[1].bytes == case.singles[1]
    assert oa.NIZK.verify_many(case.inst, a + b, case.inputs, case.gens, LABEL) == [0] * 4
