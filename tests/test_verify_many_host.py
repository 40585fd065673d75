"""otti_nizk_verify_many without a GPU: the batch verifier's host path (every worker evaluates A, B, C on the host, as otti_nizk_verify does below
4096 constraints or without a device) on proofs made by the CPU oracle, element by element against otti_nizk_verify on each item alone; the exported
symbols; and nizk_verify_many as a stand-alone program (tests/verify_many_check.cpp: own main, host sources only, nothing preloaded) under the
address + undefined-behaviour sanitizers and under the thread sanitizer."""
import os
import re
import subprocess
import threading

import pytest

import host_build
import otti_amd as oa
import orc
import verify_many_cases as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = b"many"


def _oracle_items(n, ni=3):
    r = oa.synth_r1cs(n, ni, 1)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    oi, og = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"]), orc.OGens(r["num_cons"], r["num_vars"], r["num_inputs"])
    proofs = [orc.nizk_prove(oi, r["vars"], r["inputs"], og, LABEL, bytes([seed]) * 32)[0] for seed in range(1, 7)]
    assert len(set(proofs)) == 6                                                        # six seeds: six different blinds, six different points
    nc, nv, _ = inst.dims
    return inst, gens, vm.tamper_list(proofs, r["inputs"], nc, nv)


@pytest.fixture(scope="module", params=[1 << 6, 1 << 10])
def case(request):
    return _oracle_items(request.param)


def test_results_are_the_single_verifier_codes(case):
    inst, gens, items = case
    vm.check_list(inst, gens, LABEL, items)


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


def test_new_entries_are_exported_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path]).decode()
    exported = set(re.findall(r" T (otti_[a-z0-9_]+)", out))
    hdr = open(os.path.join(ROOT, "include", "otti_spartan.h")).read()
    for name in ("otti_nizk_verify_many", "otti_k_instance_evaluate"):
        assert name in exported and re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(oa.lib, name).argtypes is not None, name                         # has its _sig entry


def _build_check(tmp_path, name, sanitize):
    return host_build.build_check(tmp_path, "verify_many_check.cpp", name, sanitize, extra=["verify_many.cpp"])


def _check_files(tmp_path, n):
    """zkif files of a small instance, six oracle proofs of it and three tampered ones"""
    s = oa.synth_r1cs(n, 3, 4)
    paths = [str(tmp_path / x) for x in ("s.zkif", "s.inp.zkif", "s.wit.zkif")]
    oa.zkif_write(s, *paths)
    oi, og = orc.OInstance(s["num_cons"], s["num_vars"], s["num_inputs"], s["A"], s["B"], s["C"]), orc.OGens(s["num_cons"], s["num_vars"], s["num_inputs"])
    proofs = [orc.nizk_prove(oi, s["vars"], s["inputs"], og, LABEL, bytes([seed]) * 32)[0] for seed in range(1, 7)]
    inst = oa.Instance.new(s["num_cons"], s["num_vars"], s["num_inputs"], s["A"], s["B"], s["C"])
    nc, nv, _ = inst.dims
    items = vm.tamper_list(proofs, s["inputs"], nc, nv)
    files = []
    for k, blob in enumerate(proofs + [items[2][0], items[3][0], items[6][0]]):
        p = tmp_path / ("proof%d.bin" % k)
        p.write_bytes(blob)
        files.append(str(p))
    return [*paths, LABEL.decode(), *files]


def test_batch_verifier_under_address_and_ub_sanitizers(tmp_path):
    exe = _build_check(tmp_path, "verify_many_asan", host_build.ASAN_UBSAN)
    r = subprocess.run([str(exe), *_check_files(tmp_path, 200)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    tail = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0, tail
    assert "12 items (6 accepted), workers 1 2 4, both orders, 0 mismatches" in r.stdout, tail


def test_batch_verifier_under_thread_sanitizer(tmp_path):
    """workers, their spinning helpers and the deferred group equations of several proofs at once: no data race.  (gcc 11's libtsan does not
    intercept pthread_cond_clockwait, which the helper pool's wait_for uses: its sleeping helpers are reported as "double lock of a mutex", the known
    false positive tests/test_host.py names; the run goes on past it and everything else must be clean.)"""
    exe = _build_check(tmp_path, "verify_many_tsan", host_build.TSAN)
    r = subprocess.run([str(exe), *_check_files(tmp_path, 200)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, OTTI_HOST_THREADS="3", TSAN_OPTIONS="halt_on_error=0"))
    tail = r.stdout[-2000:] + r.stderr[-4000:]
    assert "12 items (6 accepted), workers 1 2 4, both orders, 0 mismatches" in r.stdout, tail
    reports = re.findall(r"WARNING: ThreadSanitizer: ([^(\n]+)", r.stderr)
    assert all(w.strip() == "double lock of a mutex" for w in reports), (sorted(set(reports)), tail)
