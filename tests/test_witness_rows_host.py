"""What the kept-rows entry points (otti_witness_keep_rows, otti_witness_keep_rows_snark, otti_witness_drop_rows, otti_witness_rows_info) promise
without a GPU: exported, declared and bound symbols, argument errors answered before any device is touched (the witness pointers below are
never dereferenced), and OTTI_ERR_NO_DEVICE for valid arguments without a device."""
import ctypes
import os
import re
import subprocess

import pytest

import otti_amd as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
NAMES = ("otti_witness_keep_rows", "otti_witness_keep_rows_snark", "otti_witness_drop_rows", "otti_witness_rows_info")
BAD_ARG, NO_DEVICE = -21, -20
SENTINEL = 0x5e5e5e5e


def _inst(n=8, ni=2):
    r = oa.synth_r1cs(n, ni, 1)
    return oa.Instance.new(n, n, ni, r["A"], r["B"], r["C"])


def test_symbols_exported_declared_and_bound():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, syms), name
        assert re.search(r"int32_t\s+%s\s*\(" % name, header), name
        assert hasattr(oa.lib, name)
    for name in ("keep_rows", "drop_rows", "rows_info"):
        assert hasattr(oa.Witness, name), name


def test_header_states_the_contract():
    text = " ".join(open(HEADER).read().split())
    i = text.index("kept rows: a resident witness")
    block = text[i:text.index("int32_t otti_witness_keep_rows(", i)]
    for phrase in ("128 * L bytes", "Both provers use them", "sharded proofs ignore them", "byte-identical with and without kept rows"):
        assert phrase in block, phrase


def test_argument_errors_come_before_any_device():
    inst = _inst()
    gens, other = oa.NIZKGens.new(8, 8, 2), oa.NIZKGens.new(64, 64, 2)
    sg, sother = oa.SNARKGens.new(8, 8, 2, 8), oa.SNARKGens.new(64, 64, 2, 64)
    fake_wit = ctypes.c_void_p(1)                              # never dereferenced: every case below is refused on its arguments alone
    keep, keep_snark, drop, info = (getattr(oa.lib, n) for n in NAMES)
    for f, g, g_other in ((keep, gens, other), (keep_snark, sg, sother)):
        assert f(None, fake_wit, g._h) == BAD_ARG
        assert f(inst._h, None, g._h) == BAD_ARG
        assert f(inst._h, fake_wit, None) == BAD_ARG
        assert f(inst._h, fake_wit, g_other._h) == BAD_ARG      # generators made for another size
        assert b"different instance size" in _last_error()
    assert drop(None) == BAD_ARG
    kept, L, R, n = ctypes.c_int32(SENTINEL), ctypes.c_size_t(SENTINEL), ctypes.c_size_t(SENTINEL), ctypes.c_uint64(SENTINEL)
    assert info(None, ctypes.byref(kept), ctypes.byref(L), ctypes.byref(R), ctypes.byref(n)) == BAD_ARG
    assert info(None, None, None, None, None) == BAD_ARG
    assert (kept.value, L.value, R.value, n.value) == (SENTINEL,) * 4


def _last_error():
    buf = ctypes.create_string_buffer(256)
    oa.lib.otti_last_error(buf, 256)
    return buf.value


@pytest.mark.skipif(oa.device_count() > 0, reason="only meaningful without a GPU")
def test_valid_arguments_without_a_device_are_no_device():
    inst = _inst()
    gens, sg = oa.NIZKGens.new(8, 8, 2), oa.SNARKGens.new(8, 8, 2, 8)
    fake_wit = ctypes.c_void_p(1)
    assert oa.lib.otti_witness_keep_rows(inst._h, fake_wit, gens._h) == NO_DEVICE
    assert oa.lib.otti_witness_keep_rows_snark(inst._h, fake_wit, sg._h) == NO_DEVICE
    # without a device no witness handle can exist: such a pointer is rejected, not read
    kept = ctypes.c_int32(SENTINEL)
    assert oa.lib.otti_witness_rows_info(fake_wit, ctypes.byref(kept), None, None, None) == NO_DEVICE
    assert kept.value == SENTINEL
    assert oa.lib.otti_witness_drop_rows(fake_wit) == NO_DEVICE
    w = oa.Witness._adopt(fake_wit)
    try:
        with pytest.raises(oa.NoDeviceError):
            w.keep_rows(inst, gens)
        with pytest.raises(oa.NoDeviceError):
            w.rows_info()
    finally:
        w._h = None                                            # not a handle: nothing to free
