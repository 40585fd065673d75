"""otti_snark_verify_many on the GPU: six proofs of one commitment (six seeds) and the tamper list of snark_verify_many_cases.py, element by element
against otti_snark_verify on each item alone.  At 2^12 (compiler-like: 512 rows of comm_derefs and comm_ops, 128 of comm_mem) the sums over the
first two go to the device and the third stays on the host: one call takes both routes.  At 2^14 (uniform) all three sums have at least 256
points and go to the device.  The kernels of the batched pass themselves: test_gpu_row_sum_many.py."""
import threading

import pytest

import otti_amd as oa
import snark_verify_many_cases as sm

pytestmark = pytest.mark.gpu
LABEL = b"many"


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def _device_items(r):
    nz = max(r["A"].size, r["B"].size, r["C"].size)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nz)
    prover_comm = oa.ComputationCommitment.encode(inst, gens)
    inputs = oa.InputsAssignment.new(r["inputs"])
    wit = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), inputs)
    proofs = [oa.SNARK.prove(inst, prover_comm, wit, None, gens, LABEL, bytes([seed]) * 32).bytes for seed in range(1, 7)]
    assert len(set(proofs)) == 6
    comm_bytes = prover_comm.bytes
    comm = oa.ComputationCommitment.from_bytes(comm_bytes)      # the verifier holds the commitment only
    return comm, comm_bytes, gens, sm.tamper_list(proofs, r["inputs"]), sm.derefs_offset(proofs[0])[1]


# name -> (instance, which of the sums over (comm_derefs, comm_ops, comm_mem) have at least 256 points)
CASES = {"compiler-like-2^12": (lambda: oa.synth_r1cs_compiler_like(1 << 12, 10, 5), (True, True, False)),
         "uniform-2^14": (lambda: oa.synth_r1cs(1 << 14, 10, 1), (True, True, True))}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    make, on_device = CASES[request.param]
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OTTI_MSM_WINDOW", "10")                     # narrow generator tables: tens of MB, built in milliseconds
        yield (*_device_items(make()), on_device)


def test_the_set_sizes_put_the_sums_where_the_case_says(case):
    """The rows of the three commitments, read from the bytes, are what SNARKGens::new gives them (2^(m / 2) rows for a polynomial of m variables:
    log2 nnz + 3 for derefs, + 4 for ops, max(log2 N, log2 2V) + 1 for mem), and they fall on the sides of the 256-point threshold the case is
    there for: at 2^12 the sum over comm_mem stays on the host while the others go to the device — one call takes both routes —, at 2^14 all go."""
    comm, comm_bytes, gens, items, n_derefs, on_device = case
    _, n_ops, n_mem = sm.comm_sizes(comm_bytes)
    print("rows: comm_derefs", n_derefs, "comm_ops", n_ops, "comm_mem", n_mem)
    nc, nv, _, n_entries = comm.dims
    lgnz, lgm = max(1, (n_entries - 1).bit_length()), max(nc.bit_length() - 1, (2 * nv).bit_length() - 1) + 1
    assert (n_derefs, n_ops, n_mem) == (1 << ((lgnz + 3) // 2), 1 << ((lgnz + 4) // 2), 1 << (lgm // 2))
    assert tuple(n >= 256 for n in (n_derefs, n_ops, n_mem)) == on_device, (n_derefs, n_ops, n_mem)
    assert any(on_device)                                      # never the host alone


def test_results_are_the_single_verifier_codes(case, monkeypatch):
    comm, comm_bytes, gens, items, _, _ = case
    sm.check_list(comm, gens, LABEL, items, monkeypatch)


def test_count_zero_and_argument_refusals(case):
    comm, comm_bytes, gens, items, _, _ = case
    sm.check_refusals(comm, gens, LABEL, items)


def test_two_caller_threads_on_the_same_handles(case):
    comm, comm_bytes, gens, items, _, _ = case
    want = [sm.single_code(comm, gens, LABEL, p, i) for p, i in items]
    fresh = oa.ComputationCommitment.from_bytes(comm_bytes)     # both callers race for the first decode of its points
    got = [None, None]

    def call(k):
        got[k] = sm.many(fresh, gens, LABEL, items if k == 0 else items[::-1], threads=2)

    th = [threading.Thread(target=call, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == want and got[1] == want[::-1]


def test_more_proofs_than_the_chunk(case, monkeypatch):
    """eleven good proofs with a chunk of four: passes of 4, 4 and 3 jobs over the cached commitment points"""
    comm, comm_bytes, gens, items, _, _ = case
    good = [items[k] for k in (0, 1)]
    monkeypatch.setenv("OTTI_SNARK_VERIFY_CHUNK", "4")
    assert sm.many(comm, gens, LABEL, (good * 6)[:11], threads=4) == [0] * 11


def test_a_commitment_with_an_undecodable_point(case):
    """comm_ops re-read from bytes with one point that does not decode: every otherwise good proof gets the single verifier's code"""
    comm, comm_bytes, gens, items, _, _ = case
    first, n_ops, _ = sm.comm_sizes(comm_bytes)
    bad = bytearray(comm_bytes); bad[first + 32 * (n_ops // 2):first + 32 * (n_ops // 2) + 32] = sm.UNDECODABLE
    bad_comm = oa.ComputationCommitment.from_bytes(bytes(bad))
    good = [items[k] for k in (0, 1)]
    singles = [sm.single_code(bad_comm, gens, LABEL, p, i) for p, i in good]
    assert all(c != 0 for c in singles)
    assert sm.many(bad_comm, gens, LABEL, good) == singles
    assert sm.many(bad_comm, gens, LABEL, good, threads=1) == singles
