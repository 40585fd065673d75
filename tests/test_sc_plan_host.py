"""The sum-check round kernels' launch plan (otti_amd/csrc/sc_plan.h: grid width and items per thread of every launch) as a
host program: the header is standard library only, so the grids of a 2^20 proof's rounds and the edges of the rule are pinned
without a GPU.  The launches themselves are covered on the GPU by tests/test_gpu_kernels.py and test_gpu_sumcheck_reduce.py."""
import os, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_of_the_proofs_rounds_and_the_edges_of_the_rule(tmp_path):
    exe = tmp_path / "sc_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "otti_amd", "csrc"), os.path.join(ROOT, "tests", "sc_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "23 plans checked" in r.stdout and "0 failures" in r.stdout
