"""otti_nizk_verify_batch on the GPU, on the product's own proofs (asserted equal to the oracle's): the group equations of a batch as one sum on
the device.  At 2^12 the instance evaluation is queued on the device and the 64 row commitments stay on the host, so the decode and msm_var
launches the counters show are the batch pass's own; at 2^16 a proof's 256 row commitments are summed on the device as well, on the workers'
contexts.  The device pass by itself: test_gpu_batch_sum.py."""
import threading
import time

import pytest

import otti_amd as oa
import proof_fields as pf
import proof_fields_cases as pc
from verify_batch_cases import batch, corpus_in_batches

pytestmark = pytest.mark.gpu
SEEDS = [bytes([seed]) * 32 for seed in range(1, 7)]


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(scope="module", autouse=True)
def narrow_tables():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OTTI_MSM_WINDOW", "10")                     # narrow generator tables: tens of MB, built in milliseconds
        yield


def _launches(call):
    oa.stats_enable(True)
    try:
        out = call()
        st = oa.stats_read()
    finally:
        oa.stats_enable(False)
    return out, {k: v[0] for k, v in st.items() if v[0]}


def _run(n, pick, what):
    case = pc.NizkCase(oa.synth_r1cs(n, 10, 1))
    proof = case.device_proof()
    assert proof == case.oracle_proof(), "the device proof differs from the oracle's for the same seed"
    return pc.Run(case, proof, pick(proof, pf.nizk(proof)), what, skip_percent=None if pick is pf.steering else 1)


def _six_good(case):
    wit = oa.Witness(case.inst, oa.VarsAssignment.new(case.r["vars"]), oa.InputsAssignment.new(case.inputs))
    proofs = [oa.NIZK.prove(case.inst, wit, None, case.gens, pc.LABEL, s).bytes for s in SEEDS]
    assert len(set(proofs)) == 6
    return proofs


def _batch(case, blobs, **kw):
    return batch(case.inst, case.gens, pc.LABEL, [(b, case.inputs) for b in blobs], details=True, **kw)


# ------------------------------------------------------------------------------------------------ 2^12
@pytest.fixture(scope="module")
def nizk_4096():
    return _run(1 << 12, pf.one_per_field, "NIZK 2^12, one mutant per field")


def test_4096_good_proofs_take_one_device_pass(nizk_4096):
    case = nizk_4096.case
    assert case.inst.dims[0] >= 4096
    proofs = _six_good(case)
    assert _batch(case, proofs[:3])[0] == [0] * 3                                           # the generators' decoded set is made by the handle's first batch
    (codes, info), ran = _launches(lambda: _batch(case, proofs, threads=1))
    print(info, ran)
    assert codes == [0] * 6
    assert info["on_device"] == 1 and info["accepted_first_pass"] == 1 and info["singles_rerun"] == 0 and info["sum_ms"] > 0
    assert ran.get("decode", 0) == 1 and ran.get("msm_var", 0) == 1, ran                 # one decode launch, one sum launch


def test_4096_field_corpus_in_batches_of_eight(nizk_4096):
    run, case = nizk_4096, nizk_4096.case
    t0 = time.time()
    got, infos = corpus_in_batches(run, lambda blobs: _batch(case, blobs, seed=None))
    print("%d batches in %.1f s" % (len(infos), time.time() - t0))
    bad = run.many_differences(got)
    assert not bad, "%d:\n%s" % (len(bad), "\n".join(bad[:40]))
    assert all(i["on_device"] == 1 for i in infos if i["equations"])
    mid = len(run.corpus) // 2
    mutants = got[1:1 + mid] + got[2 + mid:-1]
    accepted = [(m[:2], o) for m, o, g in zip(run.corpus.mutants, run.oracle, mutants) if g == 0 and o != 0]
    assert not accepted, accepted[:20]
    print("localised %d, singles rerun %d of %d mutants" % (sum(i["localise_passes"] for i in infos), sum(i["singles_rerun"] for i in infos), len(mutants)))


def test_4096_a_batch_with_a_culprit_shows_both_passes(nizk_4096):
    run, case = nizk_4096, nizk_4096.case
    mutant = next(m for n, w, m in run.corpus.mutants if n == "sc1.proofs[0].z[0]")
    blobs = [run.proof, mutant, run.proof]
    (codes, info), ran = _launches(lambda: _batch(case, blobs, threads=1))
    print(info, ran)
    assert codes == [0, case.product(mutant), 0] and codes[1] != 0
    assert info["on_device"] == 1 and info["localise_passes"] == 1 and info["singles_rerun"] == 1
    assert ran.get("decode", 0) == 1 and ran.get("msm_var", 0) == 2, ran                 # nothing is decoded twice; one more sum launch


def test_4096_two_caller_threads_on_the_same_handles(nizk_4096):
    run, case = nizk_4096, nizk_4096.case
    blobs = [run.proof] + [m for _, _, m in run.corpus.mutants[:40:5]] + [run.proof]
    want = [case.product(b) for b in blobs]
    got = [None, None]

    def call(k):
        got[k] = _batch(case, blobs if k == 0 else blobs[::-1], threads=2, seed=None)[0]

    th = [threading.Thread(target=call, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == want and got[1] == want[::-1]


# ------------------------------------------------------------------------------------------------ 2^16
@pytest.fixture(scope="module")
def nizk_65536():
    return _run(1 << 16, pf.steering, "NIZK 2^16, steering")


def test_65536_six_good_proofs_accepted_in_the_first_pass(nizk_65536):
    case = nizk_65536.case
    assert pf.value(nizk_65536.proof, pf.nizk(nizk_65536.proof), "comm_vars.len") == 256  # the row sum goes to the device
    codes, info = _batch(case, _six_good(case))
    print(info)
    assert codes == [0] * 6 and info["on_device"] == 1 and info["accepted_first_pass"] == 1 and info["singles_rerun"] == 0 and info["localise_passes"] == 0


def test_65536_row_commitment_substitutes_between_good_proofs(nizk_65536):
    run, case = nizk_65536, nizk_65536.case
    good = _six_good(case)
    subs = [(n, w, m) for n, w, m in run.corpus.mutants if n.startswith("comm_vars[")]
    assert len(subs) >= 8
    blobs = good[:3] + [m for _, _, m in subs] + good[3:]
    want = [0] * 3 + [case.product(m) for _, _, m in subs] + [0] * 3
    assert all(w != 0 for w in want[3:-3])
    codes, info = _batch(case, blobs)
    print(info, list(zip([(n, w) for n, w, _ in subs], codes[3:-3])))
    assert codes == want
    # A row commitment is hashed before the first challenge: a substitute that decodes moves every challenge, so the walk's rx / ry differ from the
    # proof's and the single verifier is asked for the code; one that does not decode dies in the row sum, on the hashed path.  Neither reaches the
    # sum, which holds the six good proofs alone and accepts them in one pass: only the culprits are rerun.
    undecodable = sum(1 for _, w, _ in subs if w == "undecodable")
    assert undecodable >= 1 and info["live"] == len(blobs)
    assert info["singles_rerun"] == len(subs) - undecodable
    assert info["on_device"] == 1 and info["equations"] == 6 * (2 * (16 + 17) + 7) and info["accepted_first_pass"] == 1 and info["localise_passes"] == 0


def test_65536_a_deferred_only_culprit_is_found_by_the_localisation_pass(nizk_65536):
    run, case = nizk_65536, nizk_65536.case
    good = _six_good(case)
    name = "sc2.proofs[16].z_beta"
    off, kind = next((o, k) for f, o, k in pf.nizk(good[2]) if f == name)
    mutant = bytearray(good[2]); mutant[off:off + 32] = (5).to_bytes(32, "little")
    blobs = good[:2] + [bytes(mutant)] + good[3:]
    codes, info = _batch(case, blobs)
    print(info)
    assert codes == [0, 0, case.product(bytes(mutant)), 0, 0, 0] and codes[2] != 0
    assert info["on_device"] == 1 and info["accepted_first_pass"] == 0 and info["localise_passes"] == 1 and info["singles_rerun"] == 1


def test_65536_two_live_proofs_take_verify_manys_path(nizk_65536, monkeypatch):
    run, case = nizk_65536, nizk_65536.case
    off = next(o for f, o, k in pf.nizk(run.proof) if f == "sc1.proofs[0].z[0]")
    mutant = bytearray(run.proof); mutant[off:off + 32] = (5).to_bytes(32, "little"); mutant = bytes(mutant)
    blobs = [run.proof, run.proof[:-7], mutant]
    want = [0, -12, case.product(mutant)]
    codes, info = _batch(case, blobs)
    assert codes == want and want[2] != 0 and info["live"] == 2 and info["routed_to_many"] == 1 and info["equations"] == 0
    monkeypatch.setenv("OTTI_VERIFY_BATCH_RULE", "0")
    codes, info = _batch(case, blobs)
    assert codes == want and info["routed_to_many"] == 0 and info["on_device"] == 1 and info["singles_rerun"] == 1
