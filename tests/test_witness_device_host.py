"""What the device-side witness entry points (otti_witness_from_device, otti_witness_upload_ints, otti_witness_update, otti_witness_info) promise
without a GPU: exported and declared symbols, the OTTI_WIT_* values, argument errors answered before any device is touched (the pointers below
are never dereferenced), OTTI_ERR_NO_DEVICE without a device, and an `import otti_amd` that does not pull torch in."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import otti_amd as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
NAMES = ("otti_witness_from_device", "otti_witness_upload_ints", "otti_witness_update", "otti_witness_info")
BAD_ARG, NO_DEVICE, NUM_VARS, NUM_INPUTS = -21, -20, -4, -3
C32, M32, I64, U64 = 0, 1, 2, 3
SENTINEL = 0x5e5e5e5e


def _inst(n=8, ni=2):
    r = oa.synth_r1cs(n, ni, 1)
    return oa.Instance.new(n, n, ni, r["A"], r["B"], r["C"]), np.ascontiguousarray(r["inputs"])


def test_symbols_exported_declared_and_bound():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, syms), name
        assert re.search(r"int32_t\s+%s\s*\(" % name, header), name
        assert hasattr(oa.lib, name)
    for name in ("from_device", "from_ints", "from_tensor", "update", "info"):
        assert hasattr(oa.Witness, name), name


def test_format_values_in_the_header():
    header = open(HEADER).read()
    for name, value in (("OTTI_WIT_CANONICAL32", 0), ("OTTI_WIT_MONTGOMERY32", 1), ("OTTI_WIT_I64", 2), ("OTTI_WIT_U64", 3)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == value, name
    assert (oa.WIT_CANONICAL32, oa.WIT_MONTGOMERY32, oa.WIT_I64, oa.WIT_U64) == (0, 1, 2, 3)


def test_argument_errors_come_before_any_device():
    inst, inputs = _inst()
    ip, fake = inputs.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(4096)
    out = ctypes.c_void_p(SENTINEL)
    o = ctypes.byref(out)
    fd, ui, up, info = (getattr(oa.lib, n) for n in NAMES)
    # null handles and sources
    assert fd(None, fake, 8, I64, 0, ip, 2, None, o) == BAD_ARG
    assert fd(inst._h, fake, 8, I64, 0, ip, 2, None, None) == BAD_ARG
    assert fd(inst._h, None, 8, I64, 0, ip, 2, None, o) == BAD_ARG
    assert ui(None, fake, 8, I64, ip, 2, o) == BAD_ARG
    assert ui(inst._h, fake, 8, I64, ip, 2, None) == BAD_ARG
    assert ui(inst._h, None, 8, I64, ip, 2, o) == BAD_ARG
    assert up(None, fake, 0, fake, 1, I64, 0, 0, None) == BAD_ARG
    assert up(inst._h, None, 0, fake, 1, I64, 0, 0, None) == BAD_ARG
    assert up(inst._h, fake, 0, None, 1, I64, 0, 0, None) == BAD_ARG
    assert up(inst._h, fake, 0, None, 1, C32, 0, 1, None) == BAD_ARG
    assert info(None, None, None, None) == BAD_ARG
    # unknown formats; the integer upload takes integers only
    for fmt in (-1, 4, 99):
        assert fd(inst._h, fake, 8, fmt, 0, ip, 2, None, o) == BAD_ARG
        assert ui(inst._h, fake, 8, fmt, ip, 2, o) == BAD_ARG
        assert up(inst._h, fake, 0, fake, 1, fmt, 0, 1, None) == BAD_ARG
    for fmt in (C32, M32):
        assert ui(inst._h, fake, 8, fmt, ip, 2, o) == BAD_ARG
    # strides: non-zero and below the element size, or no multiple of 8
    for fmt, stride in ((I64, 4), (U64, 7), (I64, 12), (C32, 8), (C32, 24), (M32, 31), (C32, 36), (M32, 33)):
        assert fd(inst._h, fake, 8, fmt, stride, ip, 2, None, o) == BAD_ARG, (fmt, stride)
        assert up(inst._h, fake, 0, fake, 1, fmt, stride, 1, None) == BAD_ARG, (fmt, stride)
        assert up(inst._h, fake, 0, fake, 1, fmt, stride, 0, None) == BAD_ARG, (fmt, stride)
    # a device source off the 8-byte grid (a host source is staged and may sit anywhere)
    odd = ctypes.c_void_p(4100)
    for fmt in (C32, M32, I64, U64):
        assert fd(inst._h, odd, 8, fmt, 0, ip, 2, None, o) == BAD_ARG
        assert up(inst._h, fake, 0, odd, 1, fmt, 0, 1, None) == BAD_ARG
    # sizes
    assert fd(inst._h, fake, 9, I64, 0, ip, 2, None, o) == NUM_VARS
    assert ui(inst._h, fake, 9, U64, ip, 2, o) == NUM_VARS
    assert up(inst._h, fake, 8, fake, 1, I64, 0, 0, None) == NUM_VARS
    assert up(inst._h, fake, 1, fake, 8, C32, 0, 1, None) == NUM_VARS
    assert up(inst._h, fake, 2 ** 64 - 1, fake, 2, I64, 0, 0, None) == NUM_VARS          # first + count wraps round
    assert fd(inst._h, fake, 8, I64, 0, ip, 1, None, o) == NUM_INPUTS
    assert ui(inst._h, fake, 8, I64, ip, 3, o) == NUM_INPUTS
    assert out.value == SENTINEL


@pytest.mark.skipif(oa.device_count() > 0, reason="only meaningful without a GPU")
def test_valid_arguments_without_a_device_are_no_device():
    inst, inputs = _inst()
    ip, fake = inputs.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(4096)
    out = ctypes.c_void_p(SENTINEL)
    ints = np.arange(8, dtype=np.int64)
    for fmt, stride in ((C32, 0), (M32, 64), (I64, 0), (U64, 24)):
        assert oa.lib.otti_witness_from_device(inst._h, fake, 8, fmt, stride, ip, 2, None, ctypes.byref(out)) == NO_DEVICE
    assert oa.lib.otti_witness_upload_ints(inst._h, ints.ctypes.data_as(ctypes.c_void_p), 8, I64, ip, 2, ctypes.byref(out)) == NO_DEVICE
    assert oa.lib.otti_witness_update(inst._h, fake, 2, ints.ctypes.data_as(ctypes.c_void_p), 6, I64, 0, 0, None) == NO_DEVICE
    assert oa.lib.otti_witness_update(inst._h, fake, 0, fake, 8, C32, 0, 1, None) == NO_DEVICE
    assert out.value == SENTINEL
    with pytest.raises(oa.NoDeviceError):
        oa.Witness.from_ints(inst, ints, oa.InputsAssignment.new(inputs))


def test_update_names_the_types_it_takes():
    w = oa.Witness._adopt(None)                                # no handle: the values are looked at before the library is called
    inst, _ = _inst()
    for bad in ([1, 2, 3], "abc", 7, np.zeros(3, dtype=np.float64)):
        with pytest.raises(ValueError):
            w.update(inst, 0, bad)


def test_tensor_on_the_null_stream_is_synchronised_on_the_host():
    """handle 0 (torch's default stream = HIP's null stream) cannot be named to the library: it is synchronised and NULL is passed; any other
    current stream is passed on as it is; a stream the caller gives is never second-guessed.  Stand-ins: no torch, no GPU."""
    import types

    class Stream:
        def __init__(self, handle):
            self.cuda_stream, self.synced = handle, False

        def synchronize(self):
            self.synced = True

    tensor = types.SimpleNamespace(device="cuda:0")
    for handle, want in ((0, None), (0x7f00, 0x7f00)):
        st = Stream(handle)
        fake_torch = types.SimpleNamespace(cuda=types.SimpleNamespace(current_stream=lambda dev, st=st: st))
        assert oa.api._torch_stream(fake_torch, tensor, None) == want
        assert st.synced == (handle == 0)
        assert oa.api._torch_stream(fake_torch, tensor, 77) == 77


def test_import_does_not_pull_torch_in():
    code = "import sys; sys.path.insert(0, %r); import otti_amd; assert hasattr(otti_amd.Witness, 'from_tensor'); print('torch' in sys.modules)" % ROOT
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.strip() == "False"


def test_generated_multiplication_keeps_its_accumulators_apart_from_its_inputs(tmp_path):
    """The integer formats give fr_mul compile-time zero limbs; an accumulator operand that is not early-clobber may then share a register with one
    (wrong products after a carry).  The committed body is what the generator writes, and every statement declares both accumulators `+&v`."""
    import shutil
    csrc = os.path.join(ROOT, "otti_amd", "csrc")
    body = open(os.path.join(csrc, "fr_mul_gfx950.inc")).read()
    statements = [ln for ln in body.split("\n") if ln.startswith("asm(")]
    assert len(statements) >= 16
    assert all('" : "+&v"(acc), "+&v"(ex) : ' in ln for ln in statements)
    assert '"+v"(' not in body
    shutil.copy(os.path.join(csrc, "gen_fr_mul.py"), tmp_path / "gen_fr_mul.py")
    subprocess.run([sys.executable, str(tmp_path / "gen_fr_mul.py")], check=True, capture_output=True, timeout=60)
    assert open(tmp_path / "fr_mul_gfx950.inc").read() == body
