"""What one item adds to a thread's sums in the batched sum-check round kernel (otti_amd/csrc/pc_accum9.h: abe_accum9, abc_accum9, the sweep and
fold step pc_acc_step), host build, beside exact integers: the stated bounds of every term, the walk bound kPcWalkMax, the canonical sums after
kPcWalkMax and after thousands of items, and where limb 8 of a sum that is only swept would wrap (tests/pc_accum_check.cpp; the device runs the same
text in tests/test_gpu_pc_round_walks.py).  The program is stand-alone and is built with the address and undefined-behaviour sanitizers linked in."""
import re
import subprocess

import host_build


def test_accumulation_against_exact_integers(tmp_path):
    exe = host_build.build_check(tmp_path, "pc_accum_check.cpp", "pc_accum_check", host_build.ASAN_UBSAN, defines=(), host=False)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "54432 assignments" in r.stdout and " 0 failures" in r.stdout
    wraps = re.findall(r"limb 8 first wraps after (\d+) items \(sum (\d) of a (triple|product circuit), (.*)\)", r.stdout)
    assert len(wraps) == 2 and wraps[0][2] == "triple" and wraps[1][2] == "product circuit", r.stdout
    # the corner tests/test_gpu_pc_round_walks.py walks (WORST_TRIPLE there) and the count its docstring and pc_accum9.h quote
    assert (int(wraps[0][0]), wraps[0][1]) == (WRAP_ITEMS, "2") and wraps[0][3] == WORST_TRIPLE, wraps[0]
    assert int(wraps[1][0]) == 3736, wraps[1]                    # product circuits: beyond any walk the library's own grid gives (at most 1286 items)


WRAP_ITEMS = 596
WORST_TRIPLE = "(lower, upper) stored words A (0, l - 1) B (0, l - 1) C (2^232, l - 1)"
