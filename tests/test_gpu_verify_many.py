"""otti_nizk_verify_many on the GPU: six proofs of one resident witness (six seeds: six different points) and the tamper list of
verify_many_cases.py, element by element against otti_nizk_verify on each item alone.  At 2^12 (uniform and compiler-like) the batched device
evaluation runs (the threshold of 4096 constraints is met) and the row sums stay on the host (64 row commitments); at 2^16 the 256 row commitments
are summed on the device, on the workers' own contexts.  The kernels of the batched evaluation themselves: test_gpu_instance_evaluate.py."""
import threading

import pytest

import otti_amd as oa
import verify_many_cases as vm

pytestmark = pytest.mark.gpu
LABEL = b"many"


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def _device_items(r):
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    inputs = oa.InputsAssignment.new(r["inputs"])
    wit = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), inputs)
    proofs = [oa.NIZK.prove(inst, wit, inputs, gens, LABEL, bytes([seed]) * 32).bytes for seed in range(1, 7)]
    assert len(set(proofs)) == 6
    nc, nv, _ = inst.dims
    return inst, gens, vm.tamper_list(proofs, r["inputs"], nc, nv)


CASES = {"uniform-2^12": lambda: oa.synth_r1cs(1 << 12, 10, 1), "compiler-like-2^12": lambda: oa.synth_r1cs_compiler_like(1 << 12, 10, 5),
         "uniform-2^16": lambda: oa.synth_r1cs(1 << 16, 10, 1)}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OTTI_MSM_WINDOW", "10")                     # a narrow generator table: tens of MB, built in milliseconds
        yield _device_items(CASES[request.param]())


def test_results_are_the_single_verifier_codes(case):
    inst, gens, items = case
    assert inst.dims[0] >= 4096                                # the batched device evaluation is what runs
    singles = vm.check_list(inst, gens, LABEL, items)
    assert singles[vm.KINDS.index("rx0_replaced")] != 0


def test_count_zero_and_argument_refusals(case):
    inst, gens, items = case
    vm.check_refusals(inst, gens, LABEL, items)


def test_two_caller_threads_on_the_same_handles(case):
    inst, gens, items = case
    want = [vm.single_code(inst, gens, LABEL, p, i) for p, i in items]
    got = [None, None]

    def call(k):
        got[k] = vm.many(inst, gens, LABEL, items if k == 0 else items[::-1], threads=2)

    th = [threading.Thread(target=call, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == want and got[1] == want[::-1]


def test_more_proofs_than_the_resident_chunk(case):
    """eleven good proofs (the six, some twice): the evaluation runs in a chunk of eight and one of three"""
    inst, gens, items = case
    good = [items[k] for k in (0, 1, 5)]
    many = (good * 4)[:11]
    assert vm.many(inst, gens, LABEL, many, threads=4) == [0] * 11


@pytest.mark.parametrize("name,make", [("uniform-2^20", lambda: oa.synth_r1cs(1 << 20, 10, 1)), ("compiler-like-2^18", lambda: oa.synth_r1cs_compiler_like(1 << 18, 10, 5))])
def test_sizes_at_which_a_thread_walks_several_rows(name, make):
    """Above 2^19 rows in the row-per-lane layout and above 2^17 in the row-per-quad one the evaluation's grid is capped and a thread walks several
    rows, which share the low factor of eq(rx): the verifier's closing equality holds only with the exact A, B, C at each proof's own point, so
    three good proofs are accepted, and one whose stored point is moved gets the single verifier's code."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OTTI_MSM_WINDOW", "10")
        r = make()
        inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
        info = inst.device_info()
        assert info["rows"] > (1 << 17 if info["quad"] else 1 << 19), info
        gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
        inputs = oa.InputsAssignment.new(r["inputs"])
        wit = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), inputs)
        proofs = [oa.NIZK.prove(inst, wit, inputs, gens, LABEL, bytes([seed]) * 32).bytes for seed in range(1, 4)]
    nc, nv, _ = inst.dims
    nrx, nry = nc.bit_length() - 1, (2 * nv).bit_length() - 1
    rx0 = len(proofs[1]) - (8 + 32 * nry) - 32 * nrx
    moved = bytearray(proofs[1]); moved[rx0:rx0 + 32] = (7).to_bytes(32, "little")
    items = [(proofs[0], r["inputs"]), (bytes(moved), r["inputs"]), (proofs[1], r["inputs"]), (proofs[2], r["inputs"])]
    singles = [vm.single_code(inst, gens, LABEL, p, i) for p, i in items]
    assert singles[0] == singles[2] == singles[3] == 0 and singles[1] != 0
    assert vm.many(inst, gens, LABEL, items) == singles
    assert vm.many(inst, gens, LABEL, items, threads=1) == singles
