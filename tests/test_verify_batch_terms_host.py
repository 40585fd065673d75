"""batch_terms.h — the scalar side of the randomised batch verifier: weights multiplied in, terms on one point merged, generator terms folded — as a
stand-alone program (tests/verify_batch_check.cpp: own main, the field type and the standard library only), built plain and under the address +
undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import host_build


@pytest.mark.parametrize("sanitize", [(), host_build.ASAN_UBSAN], ids=["plain", "asan_ubsan"])
def test_weighing_merging_and_folding(tmp_path, sanitize):
    exe = host_build.build_check(tmp_path, "verify_batch_check.cpp", "verify_batch_check", sanitize, host=False)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    tail = r.stdout[-2000:] + r.stderr[-3000:]
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, tail
    assert "verify_batch_check: 33 cases, 0 failures" in r.stdout, tail
