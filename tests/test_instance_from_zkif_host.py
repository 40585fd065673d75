"""otti_instance_from_zkif / otti_instance_entries / otti_instance_ingest_info where no GPU is needed: the symbols and their declarations, the
argument errors that are answered before any device is touched, the host mode end to end, and the entries of an instance made the usual way."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import otti_amd as oa
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
BAD_ARG, NO_DEVICE, IO = -21, -20, -22
AUTO, HOST, DEVICE = 0, 1, 2


def _triple(tmp_path, n=256, ni=3, compiler=False):
    r = (oa.synth_r1cs_compiler_like if compiler else oa.synth_r1cs)(n, ni, 1)
    paths = [str(tmp_path / ("t" + ext)) for ext in (".zkif", ".inp.zkif", ".wit.zkif")]
    oa.zkif_write(r, *paths)
    return paths, r


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_symbols_exported_declared_and_bound_with_the_headers_signatures():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    header = re.sub(r"\s+", " ", header)
    want = {
        "otti_instance_from_zkif": "int32_t otti_instance_from_zkif(const char *circuit_path, const char *inputs_path, const char *witness_path , "
                                   "int32_t mode, otti_instance **inst, otti_r1cs **assignment);",
        "otti_instance_entries": "int32_t otti_instance_entries(otti_instance *inst, int32_t which , otti_entry *out, size_t cap, size_t *count);",
        "otti_instance_ingest_info": "int32_t otti_instance_ingest_info(const otti_instance *inst, int32_t *on_device, uint64_t *circuit_bytes, "
                                     "uint64_t *hbm_entry_bytes, double ms[4] );",
    }
    for name, decl in want.items():
        assert re.search(r"\bT %s\b" % name, syms), name
        assert decl in header, name
        assert getattr(oa.lib, name).restype is ctypes.c_int32
    assert "enum { OTTI_INGEST_AUTO = 0, OTTI_INGEST_HOST = 1, OTTI_INGEST_DEVICE = 2 };" in header
    assert len(oa.lib.otti_instance_from_zkif.argtypes) == 6 and len(oa.lib.otti_instance_entries.argtypes) == 5
    assert len(oa.lib.otti_instance_ingest_info.argtypes) == 5
    assert oa.api.INGEST_MODES == {"auto": AUTO, "host": HOST, "device": DEVICE}


def test_argument_errors_come_before_any_device(tmp_path):
    (c, i, w), _ = _triple(tmp_path, 16, 2)
    c, i, w = (os.fsencode(p) for p in (c, i, w))
    f = oa.lib.otti_instance_from_zkif
    # fake non-null outputs: never dereferenced, every call below is refused on its arguments or the files alone
    inst, asg = ctypes.cast(ctypes.c_void_p(8), ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(ctypes.c_void_p(8), ctypes.POINTER(ctypes.POINTER(oa.api._R1CS)))
    for mode in (AUTO, HOST, DEVICE):
        assert f(None, i, w, mode, inst, asg) == BAD_ARG
        assert f(c, None, w, mode, inst, asg) == BAD_ARG
        assert f(c, i, w, mode, None, asg) == BAD_ARG
        assert f(c, i, w, mode, inst, None) == BAD_ARG
        assert f(os.fsencode(str(tmp_path / "missing.zkif")), i, w, mode, inst, asg) == IO
        assert f(c, os.fsencode(str(tmp_path / "missing.inp.zkif")), w, mode, inst, asg) == IO
        assert f(c, i, os.fsencode(str(tmp_path)), mode, inst, asg) == IO               # a directory is no file
    for mode in (-1, 3, 77):
        assert f(c, i, w, mode, inst, asg) == BAD_ARG
    e = oa.lib.otti_instance_entries
    n = ctypes.c_size_t(7)
    assert e(None, 0, None, 0, ctypes.byref(n)) == BAD_ARG and n.value == 7
    assert oa.lib.otti_instance_ingest_info(None, None, None, None, None) == BAD_ARG


def test_errors_leave_the_outputs_untouched(tmp_path):
    (c, i, w), _ = _triple(tmp_path, 16, 2)
    bad = str(tmp_path / "bad.zkif")
    with open(c, "rb") as f:
        data = f.read()
    with open(bad, "wb") as f:
        f.write(data[:-9])
    h, rp = ctypes.c_void_p(0x1234), ctypes.POINTER(oa.api._R1CS)()
    assert oa.lib.otti_instance_from_zkif(os.fsencode(bad), os.fsencode(i), os.fsencode(w), HOST, ctypes.byref(h), ctypes.byref(rp)) == IO
    assert h.value == 0x1234 and not rp


@pytest.mark.skipif(oa.device_count() > 0, reason="only meaningful without a GPU")
def test_device_mode_without_a_device_is_no_device(tmp_path):
    (c, i, w), _ = _triple(tmp_path, 16, 2)
    with pytest.raises(oa.NoDeviceError):
        oa.Instance.from_zkif(c, i, w, mode="device")
    inst, _ = oa.Instance.from_zkif(c, i, w, mode="auto")                                # no runtime up: the host, silently
    assert not inst.ingest_info()["on_device"]


@pytest.mark.parametrize("compiler", [False, True], ids=["uniform", "compiler_like"])
def test_host_mode_is_zkif_load_plus_instance_new(tmp_path, compiler):
    (c, i, w), r = _triple(tmp_path, 256, 3, compiler)
    want = oa.zkif_load(c, i, w)
    inst, asg = oa.Instance.from_zkif(c, i, w, mode="host")
    for k, name in enumerate("ABC"):
        assert _same(inst.entries(k), want[name]), name
        assert asg[name] is None and asg["n" + name] == want[name].size
    assert (asg["num_cons"], asg["num_vars"], asg["num_inputs"]) == (want["num_cons"], want["num_vars"], want["num_inputs"])
    assert _same(asg["vars"], want["vars"]) and _same(asg["inputs"], want["inputs"])
    assert inst.dims == oa.Instance.new(want["num_cons"], want["num_vars"], want["num_inputs"], want["A"], want["B"], want["C"]).dims
    assert inst.is_sat(oa.VarsAssignment.new(asg["vars"]), oa.InputsAssignment.new(asg["inputs"]))
    info = inst.ingest_info()
    assert not info["on_device"] and info["circuit_bytes"] == os.path.getsize(c) and info["hbm_entry_bytes"] == 0 and info["ms"] == (0.0,) * 4
    # the oracle's proof of that circuit, through the new instance
    n, nv, ni = want["num_cons"], want["num_vars"], want["num_inputs"]
    oi, og = orc.OInstance(n, nv, ni, want["A"], want["B"], want["C"]), orc.OGens(n, nv, ni)
    pf, _ = orc.nizk_prove(oi, want["vars"], want["inputs"], og, b"lbl", b"\x11" * 32)
    oa.NIZK(pf).verify(inst, oa.InputsAssignment.new(asg["inputs"]), oa.NIZKGens.new(n, nv, ni), b"lbl")
    with pytest.raises(oa.ProofVerifyError):
        oa.NIZK(pf).verify(inst, oa.InputsAssignment.new(asg["inputs"]), oa.NIZKGens.new(n, nv, ni), b"lbx")


def test_assignment_with_null_lists_is_freed_by_r1cs_free(tmp_path):
    (c, i, w), r = _triple(tmp_path, 16, 2)
    h, rp = ctypes.c_void_p(), ctypes.POINTER(oa.api._R1CS)()
    assert oa.lib.otti_instance_from_zkif(os.fsencode(c), os.fsencode(i), None, HOST, ctypes.byref(h), ctypes.byref(rp)) == 0
    a = rp.contents
    assert not a.A and not a.B and not a.C and (a.nA, a.nB, a.nC) == (r["A"].size, r["B"].size, r["C"].size)
    assert a.nvars == 0 and a.ninputs == 2 and a.num_cons == 16                          # a verifier's load: no witness file, no assignment
    oa.lib.otti_r1cs_free(rp)
    oa.lib.otti_instance_free(h)


def test_entries_of_an_instance_made_the_usual_way_are_the_callers():
    r = oa.synth_r1cs_compiler_like(100, 3, 4)                                           # 100 variables: padded to 128, so the columns behind them were shifted
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    assert any(int(r[name]["col"].max()) >= r["num_vars"] for name in "ABC")
    for k, name in enumerate("ABC"):
        assert _same(inst.entries(k), np.ascontiguousarray(r[name], dtype=oa.api.ENTRY_DTYPE)), name
    n = ctypes.c_size_t()
    small = np.zeros(1, dtype=oa.api.ENTRY_DTYPE)
    assert oa.lib.otti_instance_entries(inst._h, 0, small.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(n)) == BAD_ARG and n.value == r["A"].size
    assert oa.lib.otti_instance_entries(inst._h, 3, None, 0, ctypes.byref(n)) == BAD_ARG
