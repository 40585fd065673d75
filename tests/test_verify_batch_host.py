"""otti_nizk_verify_batch without a GPU: the randomised batch verifier with its sum on the host cores, on proofs made by the CPU oracle.  Every
verdict is held against otti_nizk_verify on the item alone (verify_many_cases.py's list, its refusals) and, for the one-mutant-per-field corpus of
test_proof_fields_host.py, against the oracle's verifier too; the info counters say which route a batch took: one sum for good proofs, one
localisation pass and one single verification per culprit otherwise."""
import os
import re
import subprocess
import threading

import pytest

import host_build

import otti_amd as oa
import orc
import proof_fields as pf
import proof_fields_cases as pc
import verify_many_cases as vm
from verify_batch_cases import SEED, batch, corpus_in_batches, raw_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = b"many"


def _oracle_case(n, ni=3):
    r = oa.synth_r1cs(n, ni, 1)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    oi, og = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"]), orc.OGens(r["num_cons"], r["num_vars"], r["num_inputs"])
    proofs = [orc.nizk_prove(oi, r["vars"], r["inputs"], og, LABEL, bytes([seed]) * 32)[0] for seed in range(1, 7)]
    assert len(set(proofs)) == 6
    nc, nv, _ = inst.dims
    return inst, gens, proofs, r["inputs"], vm.tamper_list(proofs, r["inputs"], nc, nv)


@pytest.fixture(scope="module", params=[1 << 6, 1 << 10])
def case(request):
    return _oracle_case(request.param)


def test_results_are_the_single_verifier_codes(case):
    inst, gens, _, _, items = case
    singles = [vm.single_code(inst, gens, LABEL, p, i) for p, i in items]
    got = batch(inst, gens, LABEL, items)
    print("single codes", singles, "verify_batch", got)
    assert got == singles
    for kind, code in zip(vm.KINDS, got):
        assert (code == 0) == (kind == "good"), (kind, code)
    assert batch(inst, gens, LABEL, items[::-1]) == singles[::-1]
    for threads in (1, 3):
        assert batch(inst, gens, LABEL, items, threads) == singles, threads
    for k in range(len(items)):                                                          # lists of one
        assert batch(inst, gens, LABEL, [items[k]]) == [singles[k]], vm.KINDS[k]


def test_count_zero_and_argument_refusals(case, monkeypatch):
    """vm.check_refusals, word for word, with the batch entry in verify_many's place"""
    inst, gens, _, _, items = case
    monkeypatch.setattr(vm, "raw_many", raw_batch)
    monkeypatch.setattr(oa.NIZK, "verify_many", staticmethod(lambda *a, **k: oa.NIZK.verify_batch(*a, **k)))
    vm.check_refusals(inst, gens, LABEL, items)
    singles = [vm.single_code(inst, gens, LABEL, p, i) for p, i in items]
    rc, raw, rejected = raw_batch(inst._h, gens._h, LABEL, items)
    assert rc == 0 and raw == singles and rejected == 5
    assert "5 of 8" in oa.api._last_error()


def test_good_proofs_are_accepted_by_one_sum(case):
    """the guard against a term form that rejects valid proofs: six good proofs, one sum, no single verification"""
    inst, gens, proofs, inputs, _ = case
    codes, info = batch(inst, gens, LABEL, [(p, inputs) for p in proofs], details=True)
    print(info)
    assert codes == [0] * 6
    assert info["accepted_first_pass"] == 1 and info["singles_rerun"] == 0 and info["localise_passes"] == 0
    assert info["live"] == 6 and info["on_device"] == 0 and info["equations"] > 0 and info["points"] > 0 and info["gen_slots"] > 0
    nc, nv, _ = inst.dims
    rounds = (nc.bit_length() - 1) + ((2 * nv).bit_length() - 1)
    assert info["equations"] == 6 * (2 * rounds + 7)                                     # two per round, six sigma equations, the closing equation


def _deferred_only_mutant(proof, nc):
    """a scalar of the last round's dot-product proof of the first sum-check replaced: only a deferred group equation sees it"""
    name = "sc1.proofs[%d].z[0]" % (nc.bit_length() - 2)
    off, kind = next((o, k) for f, o, k in pf.nizk(proof) if f == name)
    assert kind != "len"
    out = bytearray(proof); out[off:off + 32] = (5).to_bytes(32, "little")
    return bytes(out)


def test_one_mutant_between_good_proofs_is_the_only_rerun(case):
    inst, gens, proofs, inputs, _ = case
    mutant = _deferred_only_mutant(proofs[1], inst.dims[0])
    items = [(proofs[0], inputs), (mutant, inputs), (proofs[2], inputs)]
    singles = [vm.single_code(inst, gens, LABEL, p, i) for p, i in items]
    assert singles[0] == 0 and singles[1] != 0 and singles[2] == 0
    codes, info = batch(inst, gens, LABEL, items, details=True)
    print(singles, codes, info)
    assert codes == singles
    assert info["accepted_first_pass"] == 0 and info["localise_passes"] == 1 and info["singles_rerun"] == 1


def test_a_seed_repeats_the_counters_and_entropy_the_verdicts(case):
    inst, gens, _, _, items = case
    a = batch(inst, gens, LABEL, items, details=True)
    b = batch(inst, gens, LABEL, items, details=True)
    ints = lambda d: {k: v for k, v in d.items() if k != "sum_ms"}
    assert a[0] == b[0] and ints(a[1]) == ints(b[1])
    assert batch(inst, gens, LABEL, items, seed=None) == a[0]


def test_two_caller_threads_on_the_same_handles(case):
    inst, gens, _, _, items = case
    want = [vm.single_code(inst, gens, LABEL, p, i) for p, i in items]
    got = [None, None]

    def call(k):
        got[k] = batch(inst, gens, LABEL, items if k == 0 else items[::-1], threads=2, seed=None)

    th = [threading.Thread(target=call, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == want and got[1] == want[::-1]


# ------------------------------------------------------------------------------------------------ one mutant per field
@pytest.fixture(scope="module")
def nizk_run():
    case = pc.NizkCase(oa.synth_r1cs(64, 3, 7))                                          # test_proof_fields_host.py's corpus, at its size
    proof = case.oracle_proof()
    return pc.Run(case, proof, pf.full(proof, pf.nizk(proof)), "NIZK n = 64, ni = 3")


def test_field_corpus_in_batches_of_eight(nizk_run):
    case = nizk_run.case
    got, infos = corpus_in_batches(nizk_run, lambda blobs: batch(case.inst, case.gens, pc.LABEL, [(b, case.inputs) for b in blobs], seed=None, details=True))
    bad = nizk_run.many_differences(got)
    assert not bad, "%d:\n%s" % (len(bad), "\n".join(bad[:40]))
    assert len(nizk_run.corpus) >= 500
    mid = len(nizk_run.corpus) // 2
    mutants = got[1:1 + mid] + got[2 + mid:-1]
    assert len(mutants) == len(nizk_run.corpus)
    accepted = [(m[:2], o) for m, o, g in zip(nizk_run.corpus.mutants, nizk_run.oracle, mutants) if g == 0 and o != 0]
    assert not accepted, accepted[:20]
    print("batches %d, localised %d, singles rerun %d of %d mutants" % (len(infos), sum(i["localise_passes"] for i in infos), sum(i["singles_rerun"] for i in infos), len(mutants)))


def test_small_instances_are_not_routed_to_verify_many(case):
    """two live proofs: below 2^16 constraints the batch itself runs (the routing of larger instances: test_gpu_verify_batch.py)"""
    inst, gens, proofs, inputs, items = case
    two = [(proofs[0], inputs), (proofs[3][:-7], inputs), (proofs[1], inputs)]             # the truncated one is not live
    codes, info = batch(inst, gens, LABEL, two, details=True)
    assert codes == [0, vm.MALFORMED, 0] and info["live"] == 2 and info["routed_to_many"] == 0 and info["accepted_first_pass"] == 1 and info["equations"] > 0


# ------------------------------------------------------------------------------------------------ the exported entries; the stand-alone program
def test_new_entries_are_exported_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path]).decode()
    exported = set(re.findall(r" T (otti_[a-z0-9_]+)", out))
    hdr = open(os.path.join(ROOT, "include", "otti_spartan.h")).read()
    for name in ("otti_nizk_verify_batch", "otti_k_batch_sum"):
        assert name in exported and re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(oa.lib, name).argtypes is not None, name
    assert callable(oa.NIZK.verify_batch) and callable(oa.kernels.batch_sum)


def _check_files(tmp_path, n):
    """zkif files of a small instance, six oracle proofs of it, three tampered ones and one only a deferred equation rejects"""
    s = oa.synth_r1cs(n, 3, 4)
    paths = [str(tmp_path / x) for x in ("s.zkif", "s.inp.zkif", "s.wit.zkif")]
    oa.zkif_write(s, *paths)
    oi, og = orc.OInstance(s["num_cons"], s["num_vars"], s["num_inputs"], s["A"], s["B"], s["C"]), orc.OGens(s["num_cons"], s["num_vars"], s["num_inputs"])
    proofs = [orc.nizk_prove(oi, s["vars"], s["inputs"], og, LABEL, bytes([seed]) * 32)[0] for seed in range(1, 7)]
    inst = oa.Instance.new(s["num_cons"], s["num_vars"], s["num_inputs"], s["A"], s["B"], s["C"])
    nc, nv, _ = inst.dims
    items = vm.tamper_list(proofs, s["inputs"], nc, nv)
    files = []
    for k, blob in enumerate(proofs + [items[2][0], items[3][0], items[6][0], _deferred_only_mutant(proofs[4], nc)]):
        p = tmp_path / ("proof%d.bin" % k)
        p.write_bytes(blob)
        files.append(str(p))
    return [*paths, LABEL.decode(), *files]


WANT = "verify_batch_host_check: 13 items (6 accepted), workers 1 2 4, both orders, 0 mismatches"


def test_batch_verifier_under_address_and_ub_sanitizers(tmp_path):
    exe = host_build.build_check(tmp_path, "verify_batch_host_check.cpp", "verify_batch_asan", host_build.ASAN_UBSAN, extra=["verify_many.cpp", "verify_batch.cpp"])
    r = subprocess.run([str(exe), *_check_files(tmp_path, 200)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    tail = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0, tail
    assert WANT in r.stdout, tail


def test_batch_verifier_under_thread_sanitizer(tmp_path):
    """workers with their spinning helpers, the decode threads of the host sum and the single verifier's background threads: no data race.  (The
    helper pool's sleeping helpers are reported as "double lock of a mutex" by this libtsan, the known false positive test_verify_many_host.py names.)"""
    exe = host_build.build_check(tmp_path, "verify_batch_host_check.cpp", "verify_batch_tsan", host_build.TSAN, extra=["verify_many.cpp", "verify_batch.cpp"])
    r = subprocess.run([str(exe), *_check_files(tmp_path, 200)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, OTTI_HOST_THREADS="3", TSAN_OPTIONS="halt_on_error=0"))
    tail = r.stdout[-2000:] + r.stderr[-4000:]
    assert WANT in r.stdout, tail
    reports = re.findall(r"WARNING: ThreadSanitizer: ([^(\n]+)", r.stderr)
    assert all(w.strip() == "double lock of a mutex" for w in reports), (sorted(set(reports)), tail)
