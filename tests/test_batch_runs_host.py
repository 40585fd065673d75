"""Product-form runs in the verifiers' term lists (batch_terms.h BtRun, bt_run_expand, bt_weigh; spartan_host.cpp dotproductlog_verify with a
collector that takes runs, and the closed form of a_hat) as a stand-alone program (tests/batch_runs_check.cpp: own main, the host sources beside
it, nothing preloaded), built plain and under the address + undefined-behaviour sanitizers.  The program holds bt_run_expand against the doubling
recurrence for lg = 0 .. 13, bt_weigh with runs against bt_weigh over the written-out terms, the closed-form a_hat against the direct sum on random
points and on coordinates 0, 1 and l - 1, and a sink without accept_runs against today's term count."""
import os
import subprocess

import pytest

import host_build


@pytest.mark.parametrize("sanitize", [(), host_build.ASAN_UBSAN], ids=["plain", "asan_ubsan"])
def test_runs_expand_weigh_and_close(tmp_path, sanitize):
    exe = host_build.build_check(tmp_path, "batch_runs_check.cpp", "batch_runs_check", sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    tail = r.stdout[-2000:] + r.stderr[-3000:]
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, tail
    assert "batch_runs_check: 85 cases, 0 failures" in r.stdout, tail                   # 14 + 12 + 1 + 12 * 4 + 10
