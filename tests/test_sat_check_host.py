"""The satisfiability check's surface that needs no GPU: exported symbols and their declarations, argument errors that must be answered
before any device is touched, and the `spzk check` / `--check` command line."""
import ctypes
import os
import re
import subprocess

import pytest

import otti_amd as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPZK = os.path.join(ROOT, "otti_amd", "spzk")
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
BAD_ARG, NO_DEVICE = -21, -20


def test_symbols_exported_and_declared():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = open(HEADER).read()
    for name in ("otti_witness_check_sat", "otti_kd_check_sat", "otti_instance_device_info"):
        assert re.search(r"\bT %s\b" % name, syms), name
        assert re.search(r"int32_t\s+%s\s*\(" % name, header), name
        assert hasattr(oa.lib, name)
    # the corrected comment of the host form
    assert "used by spzk before proving" not in header
    assert "sat_check" in oa.KERNEL_CLASSES and oa.KERNEL_CLASSES.index("sat_check") == len(oa.KERNEL_CLASSES) - 1
    assert oa.KERNEL_CLASSES[:18] == ("msm_rows", "msm_small", "msm_finish", "sc_cubic", "sc_quad", "spmv", "eq", "reduce", "poly_bound", "bullet", "other",
                                      "pc_round", "prod_layer", "hash_layer", "gather", "dot_many", "decode", "msm_var")


def test_null_arguments_are_bad_arg_without_a_device():
    r = oa.synth_r1cs(8, 2, 1)
    inst = oa.Instance.new(8, 8, 2, r["A"], r["B"], r["C"])
    n = ctypes.c_uint64(7)
    rows = (ctypes.c_uint64 * 4)()
    fake_wit = ctypes.c_void_p(1)                              # never dereferenced: every case below is refused on its arguments alone
    f = oa.lib.otti_witness_check_sat
    assert f(None, fake_wit, ctypes.byref(n), rows, 4, None, None) == BAD_ARG
    assert f(inst._h, None, ctypes.byref(n), rows, 4, None, None) == BAD_ARG
    assert f(inst._h, fake_wit, None, rows, 4, None, None) == BAD_ARG
    assert f(inst._h, fake_wit, ctypes.byref(n), None, 4, None, None) == BAD_ARG          # rows_cap > 0 with rows == NULL
    assert n.value == 7
    g = oa.lib.otti_kd_check_sat
    assert g(None, fake_wit, fake_wit, ctypes.byref(n), None) == BAD_ARG
    assert g(inst._h, None, fake_wit, ctypes.byref(n), None) == BAD_ARG
    assert g(inst._h, fake_wit, None, ctypes.byref(n), None) == BAD_ARG
    info = oa.api._DeviceInfo()
    assert oa.lib.otti_instance_device_info(None, 0, ctypes.byref(info)) == BAD_ARG
    assert oa.lib.otti_instance_device_info(inst._h, 0, None) == BAD_ARG
    assert ctypes.sizeof(info) == 56                           # otti_device_info: six uint64_t and two int32_t


def test_spzk_usage_lists_check():
    res = subprocess.run([SPZK], capture_output=True, text=True)
    assert res.returncode == 2
    assert "spzk check" in res.stderr and "--check" in res.stderr


def test_spzk_check_wants_three_files(tmp_path):
    pre = str(tmp_path / "t")
    assert subprocess.run([SPZK, "synth", "16", pre, "2", "5"], capture_output=True).returncode == 0
    assert subprocess.run([SPZK, "check"], capture_output=True).returncode == 2
    assert subprocess.run([SPZK, "check", pre + ".zkif"], capture_output=True).returncode == 2
    assert subprocess.run([SPZK, "check", "--nizk", pre + ".zkif", pre + ".inp.zkif"], capture_output=True).returncode == 2
    assert subprocess.run([SPZK, "check", pre + ".zkif", pre + ".inp.zkif", pre + ".wit.zkif", pre + ".zkif"], capture_output=True).returncode == 2
    # a separate verifier has no witness to check
    assert subprocess.run([SPZK, "verify", "--nizk", "--check", pre + ".zkif", pre + ".inp.zkif", "--proof-in", pre + ".zkif"], capture_output=True).returncode == 2


@pytest.mark.skipif(oa.device_count() > 0, reason="only meaningful without a GPU")
def test_spzk_check_fails_loudly_without_device(tmp_path):
    pre = str(tmp_path / "t")
    assert subprocess.run([SPZK, "synth", "16", pre, "2", "5"], capture_output=True).returncode == 0
    files = [pre + ".zkif", pre + ".inp.zkif", pre + ".wit.zkif"]
    for argv in ([SPZK, "check"] + files, [SPZK, "verify", "--nizk", "--check"] + files):
        res = subprocess.run(argv, capture_output=True, text=True)
        assert res.returncode > 0, res.returncode                                          # an exit status, not a signal
        assert "no HIP device" in res.stderr and "(%d)" % NO_DEVICE in res.stderr
        assert "Satisfied" not in res.stdout and "Verification successful" not in res.stdout


@pytest.mark.skipif(oa.device_count() > 0, reason="only meaningful without a GPU")
def test_check_sat_has_no_cpu_fallback():
    r = oa.synth_r1cs(8, 2, 1)
    inst = oa.Instance.new(8, 8, 2, r["A"], r["B"], r["C"])
    with pytest.raises(oa.NoDeviceError):
        oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"]))
    n = ctypes.c_uint64()
    z = ctypes.c_void_p(64)                                    # the device is asked for before any pointer is used
    assert oa.lib.otti_kd_check_sat(inst._h, z, z, ctypes.byref(n), None) == NO_DEVICE
    with pytest.raises(oa.NoDeviceError):
        inst.device_info()
