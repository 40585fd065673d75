"""The stand-alone check programs' one build line.  A plain helper module (imported by the tests that need it): the list of sources that compile
without HIP is read from otti_amd/csrc/hostonly.mk, where the library's Makefile and tests/san/Makefile take it from too, and a check program
(its own main, under tests/) is compiled beside them by g++ with the sanitizer flags the test names.  A sanitizer's runtime is linked into the
program; nothing here touches the environment of the program's run."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "otti_amd", "csrc")
ASAN_UBSAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan")
TSAN = ("-fsanitize=thread",)


def _mk(name):
    with open(os.path.join(SRC, "hostonly.mk")) as f:
        m = re.search(r"^%s\s*=\s*(.*)$" % name, f.read(), re.M)
    assert m, name
    return m.group(1).split()


def host_sources(extra=()):
    """paths of the host-only sources, and of `extra` (names in otti_amd/csrc) behind them"""
    return [os.path.join(SRC, s) for s in [*_mk("HOSTONLY_SRC"), *extra]]


def build_check(tmp_path, program_cpp, name, sanitize_flags, extra=(), defines=(), host=True):
    """tests/<program_cpp> + the host-only sources (+ extra) -> tmp_path/name; `defines` are -D macros of the program's own; host=False: a
    program over headers alone, nothing linked beside it"""
    exe = tmp_path / name
    sources = host_sources(extra) if host else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", *sanitize_flags, *_mk("HOSTONLY_ARCH"), *_mk("HOSTONLY_WARN"), "-Wno-unknown-pragmas",
                    *["-D" + d for d in defines], os.path.join(ROOT, "tests", program_cpp), *sources, "-o", str(exe), "-lpthread"], check=True)
    return exe
