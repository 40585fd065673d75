"""The wire format of `spzk serve` (otti_amd/csrc/serve_proto.h) as a host program: tests/serve_proto_check.cpp holds the cases — round trips,
every bound at its edge and one past it, truncation at every byte, 10,000 seeded mutations.  It is built and run twice, plain and under the
address and undefined-behaviour sanitizers; it has its own main, is never loaded into Python and never runs on a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan-ubsan"])
def test_wire_format_round_trips_bounds_truncations_and_mutations(tmp_path, flags):
    exe = tmp_path / "serve_proto_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "otti_amd", "csrc"),
                    os.path.join(ROOT, "tests", "serve_proto_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " checks, 0 failures" in r.stdout and "mutations:" in r.stdout


def test_header_is_valid_c99():
    """spzk-client is plain C and includes the same header"""
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-x", "c", "-fsyntax-only", os.path.join(ROOT, "otti_amd", "csrc", "serve_proto.h")], check=True)
