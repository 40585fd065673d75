"""otti_snark_verify_batch without a GPU: no device answers the hooks, so every row sum and the batch's one weighted sum run on the host cores —
the closing equations' product-form runs are expanded there by bt_run_expand.  Proofs made by the CPU oracle at 2^6 and 2^10; every field of
proof_fields.snark replaced once by the existing substitutes (proof_fields.one_per_field), the mutants sent through verify_batch in batches of
eight, ordered by proof_fields_cases.interleaved so that a batch's mutants come from different stretches of the wire form, a good proof in every
batch, with a fixed seed.  The results are held against the ORACLE's codes by the rule of test_proof_fields_host.py (proof_fields.failures), and
against the single verifier's code for code."""
import os
import re
import subprocess
import time

import pytest

import otti_amd as oa
import proof_fields as pf
import proof_fields_cases as pc
import snark_verify_many_cases as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes([0x5e]) * 32


class _Case:
    def __init__(self, n):
        self.case = pc.SnarkCase(oa.synth_r1cs(n, 3, 7))
        self.proofs = [self.case.oracle_proof(bytes([s]) * 32) for s in range(1, 4)]
        self.inputs = oa.InputsAssignment.new(self.case.inputs)
        proof = self.proofs[0]
        self.corpus = pf.one_per_field(proof, pf.snark(proof))
        self.corpus.check_skips()
        self.oracle = pc.codes(self.case.oracle, self.corpus, pc.ORACLE_THREADS)
        self.single = pc.codes(self.case.product, self.corpus)

    def batch(self, blobs, threads=0, details=False):
        return oa.SNARK.verify_batch(self.case.comm, blobs, self.inputs, self.case.gens, pc.LABEL, threads, SEED, details)


@pytest.fixture(scope="module", params=[1 << 6, 1 << 10])
def run(request):
    return _Case(request.param)


def test_six_good_proofs_on_the_host(run):
    got, info = run.batch(run.proofs * 2, details=True)
    print(info)
    assert got == [0] * 6 and info["on_device"] == 0 and info["accepted_first_pass"] == 1 and info["localise_passes"] == 0 and info["singles_rerun"] == 0
    rounds = (run.case.N.bit_length() - 1) + (2 * run.case.V).bit_length() - 1
    assert info["live"] == 6 and info["equations"] == 6 * (2 * rounds + 6 + 4)


@pytest.mark.parametrize("threads", [1, 0])
def test_every_field_replaced_once_in_batches_of_eight(run, threads):
    corpus = run.corpus
    order = pc.interleaved(len(corpus), 7)
    got = [None] * len(corpus)
    t0 = time.time(); passes = reruns = 0
    for b in range(0, len(order), 7):
        part = order[b:b + 7]
        blobs = [corpus.mutants[i][2] for i in part]
        blobs.insert(len(part) // 2, run.proofs[(b // 7) % 3])                              # eight with the good one, which must be accepted
        codes, info = run.batch(blobs, threads, details=True)
        assert codes.pop(len(part) // 2) == 0, [corpus.mutants[i][:2] for i in part]
        passes += info["localise_passes"]; reruns += info["singles_rerun"]
        for i, c in zip(part, codes):
            got[i] = c
    print("%d mutants in batches of eight, threads=%d: %.1f s, %d localisation passes, %d single reruns" % (len(corpus), threads, time.time() - t0, passes, reruns))
    bad = pf.failures(corpus, run.oracle, got)
    assert not bad, "%d of %d mutants:\n%s" % (len(bad), len(corpus), "\n".join(bad[:40]))
    bad = pf.differences(corpus, run.single, got)                                            # and the single verifier's, code for code
    assert not bad, "\n".join(bad[:40])
    assert passes >= 1


@pytest.mark.parametrize("member", ["pe_mem.z2", "pe_ops.z1", "pe_derefs.L[0]", "polyeval.z1", "pok.z2"])
def test_a_culprit_no_hash_sees_is_localised(run, member):
    proof = run.proofs[1]
    fields = pf.snark(proof)
    field = next(f for f in fields if f[0] == member)
    m = pf.substitute(proof, fields, field, pf.ONE_PER_FIELD[field[2]])
    blobs = [run.proofs[0], m, run.proofs[2], run.proofs[1]]
    got, info = run.batch(blobs, details=True)
    assert got == [0, run.case.product(m), 0, 0] and got[1] != 0
    # L[0] is hashed: its proof's other equations change with the challenge, and still nothing fails before the sum
    assert info["localise_passes"] == 1 and info["singles_rerun"] == 1 and info["accepted_first_pass"] == 0


def test_the_tamper_list_refusals_and_chunks(run, monkeypatch):
    six = [run.case.oracle_proof(bytes([s]) * 32) for s in range(1, 7)]
    items = sm.tamper_list(six, run.case.inputs)
    want = [sm.single_code(run.case.comm, run.case.gens, pc.LABEL, p, i) for p, i in items]
    call = lambda it, threads=0: oa.SNARK.verify_batch(run.case.comm, [p for p, _ in it], [oa.InputsAssignment.new(i) for _, i in it], run.case.gens, pc.LABEL, threads, SEED)
    assert call(items) == want and call(items[::-1], 2) == want[::-1]
    assert call([]) == []
    for k in (0, 3, 6):
        assert call([items[k]]) == [want[k]]
    monkeypatch.setenv("OTTI_SNARK_VERIFY_CHUNK", "4")
    assert call((items[:2] * 6)[:11], 4) == [0] * 11
    with pytest.raises(oa.SpartanError):
        call(items, 17)


def test_new_entries_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path]).decode()
    exported = set(re.findall(r" T (otti_[a-z0-9_]+)", out))
    hdr = open(os.path.join(ROOT, "include", "otti_spartan.h")).read()
    for name in ("otti_snark_verify_batch", "otti_k_gen_runs"):
        assert name in exported and re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(oa.lib, name).argtypes is not None, name
    assert callable(oa.SNARK.verify_batch) and callable(oa.kernels.gen_runs)
