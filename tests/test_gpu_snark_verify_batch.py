"""otti_snark_verify_batch on the GPU: SNARK proofs of one commitment verified as one randomised batch — the group equations of a chunk summed in
one device pass over the proofs' points and both generator handles, the closing equations' generator scalars expanded on the device (k_gen_runs) —
element by element against otti_snark_verify on each item alone.  The instances are test_gpu_snark_verify_many.py's: 2^12 compiler-like (the sum
over comm_mem stays on the host) and 2^14 uniform (all three row sums on the device), with narrow generator tables.  The field corpus
(proof_fields.steering over every struct member of the proof) is the test that shows soundness: it fails if a deferred equation of the evaluation
proof is dropped or left without its weight, because the mutant of that member is then accepted.  A run expanded in the wrong bit order is
another matter: every sum is then off the identity and the single verifier still settles every proof correctly, so what catches it are the
accepted_first_pass assertions of test_six_good_proofs_are_accepted_in_the_first_pass and test_more_proofs_than_the_chunk (and, kernel against
integers, test_gpu_gen_runs.py)."""
import threading
import time

import pytest

import otti_amd as oa
import proof_fields as pf
import proof_fields_cases as pc
import snark_verify_many_cases as sm

pytestmark = pytest.mark.gpu
LABEL = b"many"
SEED = bytes([0x5e]) * 32


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
    return oa.ComputationCommitment.from_bytes(comm_bytes), comm_bytes, gens, proofs, r["inputs"]


CASES = {"compiler-like-2^12": lambda: oa.synth_r1cs_compiler_like(1 << 12, 10, 5), "uniform-2^14": lambda: oa.synth_r1cs(1 << 14, 10, 1)}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OTTI_MSM_WINDOW", "10")                     # narrow generator tables: tens of MB, built in milliseconds
        yield _device_items(CASES[request.param]())


def batch(comm, gens, items, threads=0, details=False):
    return oa.SNARK.verify_batch(comm, [p for p, _ in items], [oa.InputsAssignment.new(i) for _, i in items], gens, LABEL, threads, SEED, details)


def _singles(comm, gens, items):
    return [sm.single_code(comm, gens, LABEL, p, i) for p, i in items]


def _mutant(proof, name, what):
    fields = pf.snark(proof)
    m = pf.substitute(proof, fields, next(f for f in fields if f[0] == name), what)
    assert m is not None and m != proof
    return m


def test_six_good_proofs_are_accepted_in_the_first_pass(case):
    comm, _, gens, proofs, inputs = case
    got, info = batch(comm, gens, [(p, inputs) for p in proofs], details=True)
    print(info)
    assert got == [0] * 6
    assert info["on_device"] == 1 and info["accepted_first_pass"] == 1 and info["localise_passes"] == 0 and info["singles_rerun"] == 0 and info["routed_to_many"] == 0
    assert info["live"] == 6 and info["sum_ms"] > 0
    # per proof: two equations per sum-check round, six sigma equations and four closing equations; a round names four points or more, a closing
    # equation 2 lg n + 4
    rounds = (comm.dims[0].bit_length() - 1) + (2 * comm.dims[1]).bit_length() - 1
    assert info["equations"] == 6 * (2 * rounds + 6 + 4)
    assert 6 * 4 * rounds <= info["points"] <= 6 * 40 * rounds
    # both handles: the sat handle's R row generators + 2, and the longest of the three evaluation sets + its two
    assert 64 + 2 + 256 + 2 <= info["gen_slots"] <= (1 << 15)


def test_the_tamper_list_gives_the_single_codes(case):
    comm, _, gens, proofs, inputs = case
    items = sm.tamper_list(proofs, inputs)
    want = _singles(comm, gens, items)
    for threads in (0, 1):
        got = batch(comm, gens, items[:8], threads) + batch(comm, gens, items[8:] + items[:2], threads)
        assert got == want + want[:2], threads
    assert batch(comm, gens, items[::-1]) == want[::-1]
    assert batch(comm, gens, []) == []


def test_the_field_corpus_in_batches_of_eight(case):
    """every struct member of the proof replaced once (proof_fields.steering), the mutants interleaved so that a batch's eight come from eight
    stretches of the wire form, a good proof in every batch: element by element the single verifier's codes, and no mutant accepted"""
    comm, _, gens, proofs, inputs = case
    proof = proofs[0]
    corpus = pf.steering(proof, pf.snark(proof))
    t0 = time.time()
    singles = [sm.single_code(comm, gens, LABEL, m, inputs) for _, _, m in corpus.mutants]
    t1 = time.time()
    assert all(c != 0 for c in singles), [m[:2] for m, c in zip(corpus.mutants, singles) if c == 0]
    order = pc.interleaved(len(corpus), 7)
    bad, passes, reruns = [], 0, 0
    for b in range(0, len(order), 7):
        part = order[b:b + 7]
        blobs = [corpus.mutants[i][2] for i in part]
        blobs.insert(len(blobs) // 2, proofs[1 + (b // 7) % 5])
        got, info = batch(comm, gens, [(x, inputs) for x in blobs], details=True)
        passes += info["localise_passes"]; reruns += info["singles_rerun"]
        want = [singles[i] for i in part]; want.insert(len(part) // 2, 0)
        names = ["%s / %s" % corpus.mutants[i][:2] for i in part]; names.insert(len(part) // 2, "good")
        bad += ["%s: single %d, batched %d" % (n, w, g) for n, w, g in zip(names, want, got) if w != g]
    print("%d mutants: singles %.1f s, batches of eight %.1f s, %d localisation passes, %d single reruns" % (len(corpus), t1 - t0, time.time() - t1, passes, reruns))
    assert not bad, "\n".join(bad[:40])
    assert passes >= 1                                          # members no hash sees (z1, z2, the sigma responses, ..) were localised, not walked into


@pytest.mark.parametrize("member", ["pe_mem.z2", "pok.z2"])
def test_a_culprit_visible_only_in_a_deferred_equation(case, member):
    """pe_mem.z2: the last closing equation over the evaluation handle; pok.z2: a sigma response over the sat handle.  Neither is hashed, so the
    walk meets no failure: the first sum is not the identity, one localisation pass names the proof, and the single verifier gives its code"""
    comm, _, gens, proofs, inputs = case
    blobs = list(proofs); blobs[3] = _mutant(proofs[3], member, "plus_one")
    items = [(b, inputs) for b in blobs]
    want = _singles(comm, gens, items)
    assert want[3] != 0 and [w for k, w in enumerate(want) if k != 3] == [0] * 5
    got, info = batch(comm, gens, items, details=True)
    print(member, info)
    assert got == want
    assert info["on_device"] == 1 and info["accepted_first_pass"] == 0 and info["localise_passes"] == 1 and info["singles_rerun"] == 1


def test_a_commitment_with_an_undecodable_point(case):
    comm, comm_bytes, gens, proofs, inputs = case
    first, n_ops, _ = sm.comm_sizes(comm_bytes)
    bad = bytearray(comm_bytes); bad[first + 32 * (n_ops // 2):first + 32 * (n_ops // 2) + 32] = sm.UNDECODABLE
    bad_comm = oa.ComputationCommitment.from_bytes(bytes(bad))
    good = [(proofs[0], inputs), (proofs[1], inputs)]
    singles = _singles(bad_comm, gens, good)
    assert all(c != 0 for c in singles)
    assert batch(bad_comm, gens, good) == singles
    assert batch(bad_comm, gens, good, threads=1) == singles


def test_more_proofs_than_the_chunk(case, monkeypatch):
    """eleven proofs with a chunk of four — sums over 4, 4 and 3 proofs —, the ninth with a wrong pe_ops.z1: only the last chunk is localised"""
    comm, _, gens, proofs, inputs = case
    monkeypatch.setenv("OTTI_SNARK_VERIFY_CHUNK", "4")
    blobs = (proofs * 2)[:11]; blobs[8] = _mutant(blobs[8], "pe_ops.z1", "plus_one")
    items = [(b, inputs) for b in blobs]
    got, info = batch(comm, gens, items, threads=4, details=True)
    print(info)
    assert [c == 0 for c in got] == [k != 8 for k in range(11)] and got[8] == sm.single_code(comm, gens, LABEL, blobs[8], inputs)
    assert info["live"] == 11 and info["localise_passes"] == 1 and info["singles_rerun"] == 1 and info["accepted_first_pass"] == 0
    assert batch(comm, gens, [(p, inputs) for p in (proofs * 2)[:11]], details=True)[1]["accepted_first_pass"] == 1


def test_two_caller_threads_on_the_same_handles(case):
    comm, comm_bytes, gens, proofs, inputs = case
    items = sm.tamper_list(proofs, inputs)
    want = _singles(comm, gens, items)
    fresh = oa.ComputationCommitment.from_bytes(comm_bytes)
    got = [None, None]

    def call(k):
        got[k] = batch(fresh, gens, items if k == 0 else items[::-1], threads=2)

    th = [threading.Thread(target=call, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == want and got[1] == want[::-1]


def test_the_host_sum_gives_the_same_list(case, monkeypatch):
    comm, _, gens, proofs, inputs = case
    items = sm.tamper_list(proofs, inputs)
    items[1] = (_mutant(proofs[1], "pe_derefs.z1", "plus_one"), inputs)
    on_dev, info_dev = batch(comm, gens, items, details=True)
    monkeypatch.setenv("OTTI_VERIFY_BATCH_SUM", "host")
    on_host, info_host = batch(comm, gens, items, details=True)
    assert on_host == on_dev == _singles(comm, gens, items) and on_dev[1] != 0
    assert info_dev["on_device"] == 1 and info_host["on_device"] == 0 and info_host["sum_ms"] == 0
    for k in ("live", "equations", "points", "gen_slots", "localise_passes", "singles_rerun"):
        assert info_dev[k] == info_host[k], k
