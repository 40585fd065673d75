"""term_sum (verify.h) — the one evaluator behind every deferred group equation of the verifiers — and the five sites that state their equations
as term lists, as a stand-alone program (tests/term_sum_check.cpp: own main, host sources only), built plain and under the address +
undefined-behaviour sanitizers and run directly."""
import os
import subprocess

import pytest

import host_build


@pytest.mark.parametrize("sanitize", [(), host_build.ASAN_UBSAN], ids=["plain", "asan_ubsan"])
def test_term_sums_and_the_sites_that_state_them(tmp_path, sanitize):
    exe = host_build.build_check(tmp_path, "term_sum_check.cpp", "term_sum_check", sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    tail = r.stdout[-2000:] + r.stderr[-3000:]
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, tail
    # 16 of the evaluator; 5 proofs accepted, the log proof once more inline; 4 + 4 + 11 + 11 + 10 fields replaced
    assert "term_sum_check: 62 cases, 0 failures" in r.stdout, tail
