"""The witness ingest's reader (otti_amd/csrc/zkif_wit_walk.h) and the device loader's frame (zkif.cpp zkif_witness_with) on the host, before any of
it runs on a GPU: tests/zkif_wit_walk_check.cpp — own main, host sources only, built with the address and undefined-behaviour sanitizers (their
runtime linked into the program: nothing is added to LD_PRELOAD and the environment is passed on as it is), no Python in the process — reads the
files of tests/zkif_witness_cases.py element by element as the kernel does and compares verdict, error code and assignment with zkif_load on the
three files followed by the upload's checks.  The two-file host loader of OTTI_INGEST_HOST is held against the same reference."""
import os
import re
import subprocess

import host_build
import zkif_ingest_cases as zc
import zkif_witness_cases as wc

N_MUTANTS = 1500


def test_reader_agrees_with_the_host_pair_under_sanitizers(tmp_path):
    exe = host_build.build_check(tmp_path, "zkif_wit_walk_check.cpp", "zkif_wit_walk_check", host_build.ASAN_UBSAN)
    d = str(tmp_path)
    lines = []
    for name, n, ni, compiler in (("uniform48", 48, 3, False), ("uniform1000", 1000, 10, False), ("compiler200", 200, 3, True)):
        paths, r = zc.product_triple(d, name, n, ni, compiler)
        lines.append(("case",) + paths + (str(r["num_vars"]), str(r["num_inputs"])))
    for name, a in wc.accepted_cases():
        lines.append(("case",) + wc.write_case(d, name, a) + (str(a["vars"].shape[0]), str(len(a["inst_ids"]))))
    base_dims = (str(len(wc.BASE_IDS)), str(len(wc.BASE_INST)))
    for name, case, code in wc.defect_cases() + wc.two_defect_cases():
        lines.append(("dims" if code == wc.BAD_ARG else "case",) + wc.write_case(d, name, case) + base_dims)
    lines.append(("case",) + wc.write_case(d, "no_dimensions_given", wc.accepted_cases()[3][1]) + ("-", "-"))
    base = wc.mutant_base()
    base_paths = wc.write_case(d, "mutant_base", base)
    dims = (str(base["vars"].shape[0]), str(len(base["inst_ids"])))
    lines.append(("case",) + base_paths + dims)
    for i, m in enumerate(wc.mutants(base["witness"], N_MUTANTS)):
        p = os.path.join(d, f"mutant{i:04d}.wit.zkif")
        with open(p, "wb") as f:
            f.write(m)
        lines.append(("mutant", base_paths[0], base_paths[1], p) + dims)
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("".join(" ".join(l) + "\n" for l in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(manifest)], capture_output=True, text=True, timeout=600, env=env)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert f"{len(lines)} files, 0 mismatches" in r.stdout, tail
    codes = dict(re.findall(r"^(?:case|dims) \S*/(\w+)\.wit\.zkif (-?\d+)$", r.stdout, re.M))
    for name, _ in wc.accepted_cases():
        assert codes[name] == "0", (name, codes[name])
    for name, _, code in wc.defect_cases() + wc.two_defect_cases():
        assert int(codes[name]) == code, (name, codes[name], code)
    m = re.search(r"^mutants: (\d+) refused, (\d+) accepted$", r.stdout, re.M)
    refused, accepted = int(m.group(1)), int(m.group(2))
    assert refused + accepted == N_MUTANTS and refused > 0 and accepted > 0, (refused, accepted)
