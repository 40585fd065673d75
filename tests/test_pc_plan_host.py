"""The layer plan of the batched product-circuit sum-check (otti_amd/csrc/pc_plan.h: device, tail and host rounds of a layer, the
armed launches, the host-only layers' export slots) as a host program: the header is standard library only, so which path each
shape takes under each switch is pinned without a GPU.  That every such path yields the oracle's proof is covered on the GPU by
tests/test_gpu_snark.py."""
import os, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layer_plans_of_the_proofs_and_what_the_tail_kernel_relies_on(tmp_path):
    exe = tmp_path / "pc_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "otti_amd", "csrc"), os.path.join(ROOT, "tests", "pc_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "19 plans checked, 3 pre-exports, 21 grids" in r.stdout and "0 failures" in r.stdout
