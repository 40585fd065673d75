"""The fixed-base MSM's launch plan (otti_amd/csrc/msm_plan.h: kernel, chunking, fuse and result route of every launch) as a host program:
the header is standard library only, so the arithmetic that sets the dominant kernel's grid is pinned without a GPU.  The launches
themselves are covered on the GPU by tests/test_gpu_msm_small_mail.py, test_gpu_witness_rows.py and test_gpu_kernels.py.
tests/test_gpu_msm_edges.py runs the kernels at these plans, and at the seam's (bulk_workgroups = 1), and asserts the plan each launch took."""
import os, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_of_the_proofs_launches_and_the_edges_between_kernels_and_routes(tmp_path):
    exe = tmp_path / "msm_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "otti_amd", "csrc"), os.path.join(ROOT, "tests", "msm_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "23 plans checked, 0 failures" in r.stdout
