"""otti_nizk_prove_many without a GPU: the three new entries are exported, declared and bound; every refusal the header lists is made before a handle
is looked into (fake non-null handles serve) and leaves the outputs as they were; and the front half's plan (prove_many_plan.h) is swept as a
stand-alone program (tests/prove_many_plan_check.cpp: own main, the header alone, nothing preloaded), plain and under the address +
undefined-behaviour sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import otti_amd as oa
from otti_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "otti_amd", "csrc")
BAD_ARG, NO_DEVICE = -21, -20
vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32


def test_error_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "otti_spartan.h")).read()
    assert re.search(r"OTTI_ERR_BAD_ARG\s*=\s*-21\b", hdr) and re.search(r"OTTI_ERR_NO_DEVICE\s*=\s*-20\b", hdr)


def test_new_entries_are_exported_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path]).decode()
    exported = set(re.findall(r" T (otti_[a-z0-9_]+)", out))
    hdr = open(os.path.join(ROOT, "include", "otti_spartan.h")).read()
    for name in ("otti_nizk_prove_many", "otti_k_multiply_vec_many", "otti_k_prove_front"):
        assert name in exported and re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(oa.lib, name).argtypes is not None, name                         # has its _sig entry
    assert "otti_prove_many_info" in hdr
    assert callable(oa.NIZK.prove_many) and callable(oa.kernels.multiply_vec_many) and callable(oa.kernels.prove_front)
    assert ctypes.sizeof(api._ProveManyInfo) == 7 * 4 + 4 * 4 + 4 + 3 * 8               # seven counters, four kernels, padding to the doubles


SENTINEL_PTR, SENTINEL_LEN, SENTINEL_RC = 0x5A5A5A5A, 777, 4242


class Call:
    """one otti_nizk_prove_many call over n items with sentinel-filled outputs"""

    def __init__(self, n):
        self.n = n
        m = max(1, n)
        self.fake = ctypes.create_string_buffer(64)                                     # a non-null "handle" nobody may look into
        self.h = ctypes.cast(self.fake, vp).value
        self.wits = (vp * m)(*([self.h] * m))
        self.proofs, self.lens, self.res = (vp * m)(*([SENTINEL_PTR] * m)), (sz * m)(*([SENTINEL_LEN] * m)), (i32 * m)(*([SENTINEL_RC] * m))
        self.failed = sz(SENTINEL_LEN)

    def run(self, inst="fake", gens="fake", wits="own", proofs="own", lens="own", res="own", threads=0):
        pick = lambda v, own: own if isinstance(v, str) and v in ("own", "fake") else v  # noqa: E731
        return oa.lib.otti_nizk_prove_many(pick(inst, self.h), pick(wits, self.wits), self.n, pick(gens, self.h), b"x", 1, None, threads,
                                           pick(proofs, self.proofs), pick(lens, self.lens), pick(res, self.res), ctypes.byref(self.failed), None, None)

    def untouched(self):
        m = max(1, self.n)
        return (all(self.proofs[k] == SENTINEL_PTR and self.lens[k] == SENTINEL_LEN and self.res[k] == SENTINEL_RC for k in range(m))
                and self.failed.value == SENTINEL_LEN)


@pytest.mark.parametrize("what", ["inst", "gens", "proofs", "lens", "res", "wits", "wits[1]", "threads"])
def test_refusals_before_any_handle_is_looked_into(what):
    c = Call(3)
    if what == "wits[1]":
        c.wits[1] = None
        rc = c.run()
    elif what == "threads":
        rc = c.run(threads=17)
    else:
        rc = c.run(**{what: None})
    assert rc == BAD_ARG and c.untouched(), what
    assert api._last_error()


def test_count_zero_with_null_arrays_is_ok():
    c = Call(0)
    assert c.run(wits=None) == 0
    assert c.failed.value == 0 and c.proofs[0] == SENTINEL_PTR and c.res[0] == SENTINEL_RC
    assert c.run(wits=None, threads=17) == BAD_ARG                                      # the argument check comes first


def _real_handles(n=64, other=256):
    r = oa.synth_r1cs(n, 3, 5)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    return inst, oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"]), oa.NIZKGens.new(other, other, 3)


def test_generators_of_another_size_then_no_device():
    """with real instance and generator handles: generators made for another size are refused before a device is asked for; sixteen threads pass
    the argument check, seventeen do not; valid arguments without a device are OTTI_ERR_NO_DEVICE — all with the outputs as they were"""
    inst, gens, wrong = _real_handles()
    c = Call(2)
    assert c.run(inst=inst._h, gens=wrong._h) == BAD_ARG and c.untouched()
    assert "generators" in api._last_error()
    assert c.run(inst=inst._h, gens=gens._h, threads=17) == BAD_ARG and c.untouched()
    if oa.device_count() > 0:
        return                                                                          # with a device the fake witness handles cannot go further
    assert c.run(inst=inst._h, gens=gens._h, threads=16) == NO_DEVICE and c.untouched()
    assert c.run(inst=inst._h, gens=gens._h) == NO_DEVICE and c.untouched()


def test_kernel_entries_refuse_null_arguments():
    inst, gens, wrong = _real_handles()
    z = np.zeros((128, 32), dtype=np.uint8)
    ptrs = (vp * 1)(z.ctypes.data_as(vp))
    o = np.zeros((64, 32), dtype=np.uint8)
    p = o.ctypes.data_as(vp)
    lib = oa.lib
    assert lib.otti_k_multiply_vec_many(None, ptrs, 1, p, p, p, None) == BAD_ARG
    assert lib.otti_k_multiply_vec_many(inst._h, ptrs, 0, p, p, p, None) == BAD_ARG
    assert lib.otti_k_multiply_vec_many(inst._h, None, 1, p, p, p, None) == BAD_ARG
    flags = np.zeros(1, dtype=np.int32)
    f = flags.ctypes.data_as(vp)
    assert lib.otti_k_prove_front(inst._h, None, ptrs, f, 1, p, p, p, p, None, None) == BAD_ARG
    assert lib.otti_k_prove_front(inst._h, gens._h, ptrs, f, 0, p, p, p, p, None, None) == BAD_ARG
    assert lib.otti_k_prove_front(inst._h, wrong._h, ptrs, f, 1, p, p, p, p, None, None) == BAD_ARG


def _plan_check(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", SRC, os.path.join(ROOT, "tests", "prove_many_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert re.search(r"^\d{6,} plans checked, 0 failures$", r.stdout, re.M), r.stdout[-2000:]


def test_plan_sweep(tmp_path):
    _plan_check(tmp_path, "prove_many_plan_check", ["-O2"])


def test_plan_sweep_under_address_and_ub_sanitizers(tmp_path):
    _plan_check(tmp_path, "prove_many_plan_asan", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"])
