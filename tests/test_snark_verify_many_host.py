"""otti_snark_verify_many without a GPU: the staged verifier's host path (every row sum is summed on the host, as otti_snark_verify does without a
device) on proofs made by the CPU oracle, element by element against otti_snark_verify on each item alone; the exported symbols; and
snark_verify_many with the four-step evaluation-proof walk as a stand-alone program (tests/snark_verify_many_check.cpp: own main, host sources
only, nothing preloaded) under the address + undefined-behaviour sanitizers and under the thread sanitizer."""
import os
import re
import subprocess
import threading

import pytest

import host_build
import otti_amd as oa
import orc
import snark_verify_many_cases as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = b"many"


def _oracle_case(n, ni=3, seed=1):
    """(oracle commitment bytes, num_nz_entries, six oracle proofs, the synthetic instance)"""
    r = oa.synth_r1cs(n, ni, seed)
    nz = max(r["A"].size, r["B"].size, r["C"].size)
    oi = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    og = orc.OSnarkGens(r["num_cons"], r["num_vars"], r["num_inputs"], nz)
    oc = orc.OSnarkComm.encode(oi, og)
    proofs = [orc.snark_prove(oi, oc, r["vars"], r["inputs"], og, LABEL, bytes([s]) * 32)[0] for s in range(1, 7)]
    assert len(set(proofs)) == 6                                                        # six seeds: six different blinds
    return oc.bytes, nz, proofs, r


def _oracle_items(n):
    cb, nz, proofs, r = _oracle_case(n)
    comm = oa.ComputationCommitment.from_bytes(cb)                                      # the verifier holds the commitment only
    gens = oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nz)
    return comm, gens, sm.tamper_list(proofs, r["inputs"])


@pytest.fixture(scope="module", params=[1 << 6, 1 << 10])
def case(request):
    return _oracle_items(request.param)


def test_results_are_the_single_verifier_codes(case, monkeypatch):
    comm, gens, items = case
    sm.check_list(comm, gens, LABEL, items, monkeypatch)


def test_count_zero_and_argument_refusals(case):
    comm, gens, items = case
    sm.check_refusals(comm, gens, LABEL, items)


def test_two_caller_threads_on_the_same_handles(case):
    comm, gens, items = case
    want = [sm.single_code(comm, gens, LABEL, p, i) for p, i in items]
    got = [None, None]

    def call(k):
        got[k] = sm.many(comm, gens, LABEL, items if k == 0 else items[::-1], threads=2)

    th = [threading.Thread(target=call, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == want and got[1] == want[::-1]


def test_more_proofs_than_the_chunk(case, monkeypatch):
    """eleven good proofs with a chunk of four: chunks of 4, 4 and 3"""
    comm, gens, items = case
    good = [items[k] for k in (0, 1)]
    monkeypatch.setenv("OTTI_SNARK_VERIFY_CHUNK", "4")
    assert sm.many(comm, gens, LABEL, (good * 6)[:11], threads=4) == [0] * 11


def test_new_entries_are_exported_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path]).decode()
    exported = set(re.findall(r" T (otti_[a-z0-9_]+)", out))
    hdr = open(os.path.join(ROOT, "include", "otti_spartan.h")).read()
    for name in ("otti_snark_verify_many", "otti_k_row_sum_many"):
        assert name in exported and re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(oa.lib, name).argtypes is not None, name                         # has its _sig entry
    assert callable(oa.SNARK.verify_many) and callable(oa.kernels.row_sum_many)


def _build_check(tmp_path, name, sanitize):
    return host_build.build_check(tmp_path, "snark_verify_many_check.cpp", name, sanitize, extra=["verify_many.cpp", "snark_verify_many.cpp"])


def _check_files(tmp_path, n):
    """commitment and inputs of a small instance, six oracle proofs of it and five tampered ones"""
    cb, nz, proofs, r = _oracle_case(n, 3, 4)
    (tmp_path / "comm.bin").write_bytes(cb)
    (tmp_path / "inputs.bin").write_bytes(r["inputs"].tobytes())
    items = sm.tamper_list(proofs, r["inputs"])
    files = []
    for k, blob in enumerate(proofs + [items[j][0] for j in (2, 3, 6, 7, 8)]):
        p = tmp_path / ("proof%d.bin" % k)
        p.write_bytes(blob)
        files.append(str(p))
    return [str(tmp_path / "comm.bin"), str(tmp_path / "inputs.bin"), str(nz), LABEL.decode(), *files]


WANT_LINE = re.compile(r"14 items \(6 accepted\), steps, workers 1 2 4, both orders, peak threads (\d+) / \1, 0 mismatches")


def test_staged_verifier_under_address_and_ub_sanitizers(tmp_path):
    exe = _build_check(tmp_path, "snark_verify_many_asan", host_build.ASAN_UBSAN)
    r = subprocess.run([str(exe), *_check_files(tmp_path, 200)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    tail = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0, tail
    assert WANT_LINE.search(r.stdout), tail


def test_staged_verifier_under_thread_sanitizer(tmp_path):
    """workers parked between the passes, their spinning helpers and the deferred group equations of several proofs at once: no data race.  (gcc 11's
    libtsan does not intercept pthread_cond_clockwait, which the helper pool's wait_for uses: its sleeping helpers are reported as "double lock of a
    mutex", the known false positive tests/test_host.py names; the run goes on past it and everything else must be clean.)"""
    exe = _build_check(tmp_path, "snark_verify_many_tsan", host_build.TSAN)
    r = subprocess.run([str(exe), *_check_files(tmp_path, 200)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, OTTI_HOST_THREADS="3", TSAN_OPTIONS="halt_on_error=0"))
    tail = r.stdout[-2000:] + r.stderr[-4000:]
    assert WANT_LINE.search(r.stdout), tail
    reports = re.findall(r"WARNING: ThreadSanitizer: ([^(\n]+)", r.stderr)
    assert all(w.strip() == "double lock of a mutex" for w in reports), (sorted(set(reports)), tail)
