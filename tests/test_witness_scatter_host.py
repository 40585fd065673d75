"""What the scatter-update entry points (otti_witness_scatter, otti_witness_scatter_info, otti_witness_set_inputs, otti_k_msm_scatter_rows) promise
without a GPU: exported, declared and bound symbols, a header that states the contract, argument and host-index errors answered before any
device is touched (the witness pointers below are never dereferenced), and OTTI_ERR_NO_DEVICE for valid arguments without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import otti_amd as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
NAMES = ("otti_witness_scatter", "otti_witness_scatter_info", "otti_witness_set_inputs", "otti_k_msm_scatter_rows")
BAD_ARG, NO_DEVICE, INVALID_INDEX, INVALID_SCALAR, INVALID_NUM_INPUTS = -21, -20, -6, -5, -3
SENTINEL = 0x5e5e5e5e
V, NI = 8, 2
Q = oa.L_ORDER
_vp = ctypes.c_void_p


def _inst():
    r = oa.synth_r1cs(V, NI, 1)
    return oa.Instance.new(V, V, NI, r["A"], r["B"], r["C"])


def _u64(xs):
    return np.array(xs, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(_vp)


def test_symbols_exported_declared_and_bound():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, syms), name
        assert re.search(r"int32_t\s+%s\s*\(" % name, header), name
        assert hasattr(oa.lib, name)
    for name in ("scatter", "scatter_info", "set_inputs"):
        assert hasattr(oa.Witness, name), name
    assert hasattr(oa.kernels, "msm_scatter_rows")


def test_header_states_the_contract():
    text = " ".join(open(HEADER).read().split())
    i = text.index("scatter update: variables idx[0 .. count)")
    block = text[i:text.index("int32_t otti_witness_scatter(", i)]
    for phrase in ("STRICTLY ASCENDING", "bit for bit", "changes nothing", "OTTI_ERR_INVALID_INDEX", "count == 0"):
        assert phrase in block, phrase
    assert "strictly ascending" in block.lower()


def test_argument_errors_come_before_any_device():
    inst = _inst()
    fake = _vp(1)                                              # never dereferenced: every case below is refused on its arguments alone
    scatter = oa.lib.otti_witness_scatter
    idx, src = _u64([1, 2]), np.array([5, 6], dtype=np.int64)
    I64, C32 = oa.WIT_I64, oa.WIT_CANONICAL32
    assert scatter(None, fake, _p(idx), _p(src), 2, I64, 0, 0, None) == BAD_ARG
    assert scatter(inst._h, None, _p(idx), _p(src), 2, I64, 0, 0, None) == BAD_ARG
    assert scatter(inst._h, fake, None, _p(src), 2, I64, 0, 0, None) == BAD_ARG          # null idx with a count
    assert scatter(inst._h, fake, _p(idx), None, 2, I64, 0, 0, None) == BAD_ARG          # null src with a count
    assert scatter(inst._h, fake, _p(idx), _p(src), 2, 4, 0, 0, None) == BAD_ARG         # unknown format
    assert scatter(inst._h, fake, _p(idx), _p(src), 2, -1, 0, 0, None) == BAD_ARG
    assert scatter(inst._h, fake, _p(idx), _p(src), 2, I64, 4, 0, None) == BAD_ARG       # stride below the element size
    assert scatter(inst._h, fake, _p(idx), _p(src), 2, I64, 12, 0, None) == BAD_ARG      # not a multiple of 8
    assert scatter(inst._h, fake, _p(idx), _p(src), 2, C32, 24, 0, None) == BAD_ARG
    assert scatter(inst._h, fake, _vp(0x1000), _vp(0x2004), 2, I64, 0, 1, None) == BAD_ARG   # misaligned device source
    assert scatter(inst._h, fake, _vp(0x1004), _vp(0x2000), 2, I64, 0, 1, None) == BAD_ARG   # misaligned device index list
    # a bad argument is named before a bad index list
    assert scatter(inst._h, fake, _p(_u64([3, 3])), _p(src), 2, 4, 0, 0, None) == BAD_ARG
    for bad in ([3, 3], [5, 4], [V], [0, V], [2, 1, 3]):
        ix, sv = _u64(bad), np.arange(len(bad), dtype=np.int64)
        assert scatter(inst._h, fake, _p(ix), _p(sv), len(bad), I64, 0, 0, None) == INVALID_INDEX, bad
    many, sv = _u64(range(V + 1)), np.zeros(V + 1, dtype=np.int64)
    assert scatter(inst._h, fake, _p(many), _p(sv), V + 1, I64, 0, 0, None) == INVALID_INDEX
    assert scatter(inst._h, fake, _vp(0x1000), _vp(0x2000), V + 1, I64, 0, 1, None) == INVALID_INDEX   # the count alone, device pointers never read

    info = oa.lib.otti_witness_scatter_info
    a, b, c = ctypes.c_uint64(SENTINEL), ctypes.c_uint64(SENTINEL), ctypes.c_uint64(SENTINEL)
    assert info(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == BAD_ARG
    assert info(None, None, None, None) == BAD_ARG
    assert (a.value, b.value, c.value) == (SENTINEL,) * 3

    set_inputs = oa.lib.otti_witness_set_inputs
    ok = np.zeros((NI, 32), dtype=np.uint8)
    assert set_inputs(None, fake, _p(ok), NI) == BAD_ARG
    assert set_inputs(inst._h, None, _p(ok), NI) == BAD_ARG
    assert set_inputs(inst._h, fake, None, NI) == BAD_ARG
    assert set_inputs(inst._h, fake, _p(ok), NI + 1) == INVALID_NUM_INPUTS
    assert set_inputs(inst._h, fake, _p(ok), NI - 1) == INVALID_NUM_INPUTS
    bad = ok.copy(); bad[1] = np.frombuffer(Q.to_bytes(32, "little"), dtype=np.uint8)
    assert set_inputs(inst._h, fake, _p(bad), NI) == INVALID_SCALAR

    out = np.zeros((1, 32), dtype=np.uint8)
    gens = oa.NIZKGens.new(V, V, NI)
    k = oa.lib.otti_k_msm_scatter_rows
    s2 = np.zeros((2, 32), dtype=np.uint8)
    assert k(None, 1, _p(idx), _p(s2), 2, _p(out), None) == BAD_ARG
    assert k(gens._h, 0, _p(idx), _p(s2), 2, _p(out), None) == BAD_ARG
    assert k(gens._h, 1, None, _p(s2), 2, _p(out), None) == BAD_ARG
    assert k(gens._h, 1, _p(_u64([3, 3])), _p(s2), 2, _p(out), None) == INVALID_INDEX
    assert k(gens._h, 1, _p(_u64([0, 1 << 40])), _p(s2), 2, _p(out), None) == INVALID_INDEX


@pytest.mark.skipif(oa.device_count() > 0, reason="only meaningful without a GPU")
def test_valid_arguments_without_a_device_are_no_device():
    inst = _inst()
    fake = _vp(1)
    idx, src = _u64([1, 7]), np.array([5, -6], dtype=np.int64)
    assert oa.lib.otti_witness_scatter(inst._h, fake, _p(idx), _p(src), 2, oa.WIT_I64, 0, 0, None) == NO_DEVICE
    assert oa.lib.otti_witness_scatter(inst._h, fake, None, None, 0, oa.WIT_I64, 0, 0, None) == NO_DEVICE     # count == 0 as well
    assert oa.lib.otti_witness_scatter(inst._h, fake, _vp(0x1000), _vp(0x2000), 2, oa.WIT_I64, 16, 1, None) == NO_DEVICE
    a = ctypes.c_uint64(SENTINEL)
    assert oa.lib.otti_witness_scatter_info(fake, ctypes.byref(a), None, None) == NO_DEVICE
    assert a.value == SENTINEL
    ok = np.zeros((NI, 32), dtype=np.uint8)
    assert oa.lib.otti_witness_set_inputs(inst._h, fake, _p(ok), NI) == NO_DEVICE
    w = oa.Witness._adopt(fake)
    try:
        with pytest.raises(oa.NoDeviceError):
            w.scatter(inst, np.array([4, 1], dtype=np.int64), np.array([1, 2], dtype=np.int64))   # sorted for the caller, then no device
        with pytest.raises(oa.NoDeviceError):
            w.scatter_info()
        with pytest.raises(oa.NoDeviceError):
            w.set_inputs(inst, ok)
    finally:
        w._h = None                                            # not a handle: nothing to free


def test_python_scatter_refuses_duplicate_and_negative_indices_itself(monkeypatch):
    inst = _inst()
    calls = []
    monkeypatch.setattr(oa.lib, "otti_witness_scatter", lambda *a: calls.append(a) or 0)
    w = oa.Witness._adopt(_vp(1))
    try:
        vals = np.array([1, 2, 3], dtype=np.int64)
        for bad in (np.array([2, 5, 2], dtype=np.int64), np.array([4, 4, 4], dtype=np.uint64), np.array([1, -1, 3], dtype=np.int64)):
            with pytest.raises(ValueError):
                w.scatter(inst, bad, vals)
        with pytest.raises(ValueError):
            w.scatter(inst, np.array([1, 2], dtype=np.int64), vals)                        # lengths differ
        with pytest.raises(ValueError):
            w.scatter(inst, np.array([1.0, 2.0, 3.0]), vals)
        assert not calls
        w.scatter(inst, np.array([6, 0, 3], dtype=np.int64), vals)                         # unsorted: sorted here, values alongside
        assert len(calls) == 1
    finally:
        w._h = None
