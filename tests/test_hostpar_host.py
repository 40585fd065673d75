"""fan_out (otti_amd/csrc/hostpar.h), the one fork-join helper of the host code: tests/hostpar_check.cpp — own main, nothing else linked, the
sanitizer's runtime linked in, nothing preloaded — under the address + undefined-behaviour sanitizers and under the thread sanitizer.  Every share
of nt = 1, 2, 16 and 64 is called exactly once; and in the variant where the start of the third thread throws std::system_error (what a refused
pthread_create does to std::thread), still exactly once, on the caller's thread from that share on, and the call returns normally instead of
unwinding through joinable threads into std::terminate."""
import os
import subprocess

import pytest

import host_build


@pytest.mark.parametrize("sanitize", [host_build.ASAN_UBSAN, host_build.TSAN], ids=["asan_ubsan", "tsan"])
@pytest.mark.parametrize("fail_at", [None, 3])
def test_every_share_runs_exactly_once(tmp_path, sanitize, fail_at):
    defines = [] if fail_at is None else ["OTTI_HOSTPAR_TEST_FAIL_AT=%d" % fail_at]
    exe = host_build.build_check(tmp_path, "hostpar_check.cpp", "hostpar_check", sanitize, defines=defines, host=False)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    tail = r.stdout[-2000:] + r.stderr[-3000:]
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, tail
    want = "hostpar_check: nt 1 2 16 64, 0 failures" if fail_at is None else "hostpar_check: thread start 3 fails, nt 1 2 16 64, 0 failures"
    assert want in r.stdout, tail
