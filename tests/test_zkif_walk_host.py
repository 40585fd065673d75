"""The device ingest's reader (otti_amd/csrc/zkif_walk.h) on the host, before any of it runs on a GPU: tests/zkif_walk_check.cpp — own main, host
sources only, built with the address and undefined-behaviour sanitizers (their runtime linked into the program: nothing is added to LD_PRELOAD and
the environment is passed on as it is), no Python in the process — runs the walker's count and emit
over the files of tests/zkif_ingest_cases.py and compares verdict, error code and entry lists with zkif_load + instance_new."""
import os
import re
import subprocess

import host_build
import zkif_ingest_cases as zc

N_MUTANTS = 1500


def test_walker_agrees_with_the_host_loader_under_sanitizers(tmp_path):
    exe = host_build.build_check(tmp_path, "zkif_walk_check.cpp", "zkif_walk_check", host_build.ASAN_UBSAN)
    d = str(tmp_path)
    lines = []
    for name, n, ni, compiler in (("uniform48", 48, 3, False), ("uniform1000", 1000, 10, False), ("compiler200", 200, 3, True)):
        paths, _ = zc.product_triple(d, name, n, ni, compiler)
        lines.append(("case",) + paths)
    base = lines[0][1:]
    for name, circuit in zc.shaped_cases() + zc.defect_cases():
        lines.append(("case",) + zc.write_case(d, name, circuit))
    lines.append(("case", lines[0][1], lines[0][2], "-"))                        # a verifier's load: no witness file
    with open(base[0], "rb") as f:
        circuit = f.read()
    for i, m in enumerate(zc.mutants(circuit, N_MUTANTS)):
        p = os.path.join(d, f"mutant{i:04d}.zkif")
        with open(p, "wb") as f:
            f.write(m)
        lines.append(("mutant", p, base[1], base[2]))
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("".join(" ".join(l) + "\n" for l in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(manifest)], capture_output=True, text=True, timeout=600, env=env)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert f"{len(lines)} files, 0 mismatches" in r.stdout, tail
    codes = dict(re.findall(r"^case \S*/(\w+)\.zkif (-?\d+)$", r.stdout, re.M))
    for name, _ in zc.shaped_cases():
        assert codes[name] == "0", (name, codes[name])
    want = dict(truncated=-22, prefix_beyond_file=-22, missing_identifier=-22, trailing_bytes=-22, constraint_offset_beyond=-22, vtable_before_start=-22,
                ids_count_beyond=-22, values_not_multiple=-22, ids_without_values=-22, width33_nonzero_tail=-5, undeclared_id=-6, coefficient_l=-5)
    for name, _ in zc.defect_cases():
        assert int(codes[name]) == want[name], (name, codes[name])
    m = re.search(r"^mutants: (\d+) refused, (\d+) accepted$", r.stdout, re.M)
    refused, accepted = int(m.group(1)), int(m.group(2))
    assert refused + accepted == N_MUTANTS and refused > 0 and accepted > 0, (refused, accepted)
