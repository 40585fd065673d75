"""otti_witness_from_zkif / otti_witness_ingest_info / otti_witness_ingest_min_mb where no GPU is needed: the symbols and their declarations, the
argument and file errors that are answered before any device is touched, the missing device said in every mode, and the parsing of the AUTO
cut-over."""
import ctypes
import os
import re
import subprocess

import pytest

import otti_amd as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
BAD_ARG, NO_DEVICE, IO = -21, -20, -22
AUTO, HOST, DEVICE = 0, 1, 2


def _triple(tmp_path, n=16, ni=2):
    r = oa.synth_r1cs(n, ni, 1)
    paths = [str(tmp_path / ("t" + ext)) for ext in (".zkif", ".inp.zkif", ".wit.zkif")]
    oa.zkif_write(r, *paths)
    return paths, r


def test_symbols_exported_declared_and_bound_with_the_headers_signatures():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    header = re.sub(r"\s+", " ", header)
    want = {
        "otti_witness_from_zkif": "int32_t otti_witness_from_zkif(otti_instance *inst, const char *inputs_path, const char *witness_path, int32_t mode, "
                                  "otti_witness **out, otti_r1cs **inputs_out);",
        "otti_witness_ingest_info": "int32_t otti_witness_ingest_info(const otti_witness *wit, int32_t *on_device, uint64_t *witness_bytes, double ms[3] );",
        "otti_witness_ingest_min_mb": "double otti_witness_ingest_min_mb(void);",
    }
    for name, decl in want.items():
        assert re.search(r"\bT %s\b" % name, syms), name
        assert decl in header, name
    assert oa.lib.otti_witness_from_zkif.restype is ctypes.c_int32 and len(oa.lib.otti_witness_from_zkif.argtypes) == 6
    assert oa.lib.otti_witness_ingest_info.restype is ctypes.c_int32 and len(oa.lib.otti_witness_ingest_info.argtypes) == 4
    assert oa.lib.otti_witness_ingest_min_mb.restype is ctypes.c_double and len(oa.lib.otti_witness_ingest_min_mb.argtypes) == 0
    assert callable(oa.Witness.from_zkif) and callable(oa.Witness.ingest_info)
    full = open(HEADER).read()
    for word in ("OTTI_INGEST_WIT_MIN_MB", "OTTI_ERR_NO_DEVICE in every mode", "*out and *inputs_out are untouched"):
        assert word in full, word


def test_argument_and_file_errors_come_before_any_device(tmp_path):
    (c, i, w), r = _triple(tmp_path)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    i, w = os.fsencode(i), os.fsencode(w)
    f = oa.lib.otti_witness_from_zkif
    # fake non-null outputs: never dereferenced, every call below is refused on its arguments or the files alone
    out = ctypes.cast(ctypes.c_void_p(8), ctypes.POINTER(ctypes.c_void_p))
    for mode in (AUTO, HOST, DEVICE):
        assert f(None, i, w, mode, out, None) == BAD_ARG
        assert f(inst._h, None, w, mode, out, None) == BAD_ARG
        assert f(inst._h, i, None, mode, out, None) == BAD_ARG
        assert f(inst._h, i, w, mode, None, None) == BAD_ARG
        assert f(inst._h, os.fsencode(str(tmp_path / "missing.inp.zkif")), w, mode, out, None) == IO
        assert f(inst._h, i, os.fsencode(str(tmp_path)), mode, out, None) == IO         # a directory is no file
    for mode in (-1, 3, 77):
        assert f(inst._h, i, w, mode, out, None) == BAD_ARG
    assert oa.lib.otti_witness_ingest_info(None, None, None, None) == BAD_ARG


@pytest.mark.skipif(oa.device_count() > 0, reason="only meaningful without a GPU")
def test_without_a_device_every_mode_is_no_device_and_the_outputs_stay(tmp_path):
    (c, i, w), r = _triple(tmp_path)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    for mode in ("auto", "host", "device"):
        with pytest.raises(oa.NoDeviceError):
            oa.Witness.from_zkif(inst, i, w, mode=mode)
    h, rp = ctypes.c_void_p(0x1234), ctypes.POINTER(oa.api._R1CS)()
    assert oa.lib.otti_witness_from_zkif(inst._h, os.fsencode(i), os.fsencode(w), HOST, ctypes.byref(h), ctypes.byref(rp)) == NO_DEVICE
    assert h.value == 0x1234 and not rp


def test_the_auto_cut_over_is_read_per_call_and_bad_values_fall_back_to_the_default(monkeypatch):
    f = oa.lib.otti_witness_ingest_min_mb
    monkeypatch.delenv("OTTI_INGEST_WIT_MIN_MB", raising=False)
    default = f()
    m = re.search(r"OTTI_INGEST_WIT_MIN_MB MiB \(read per call; default ([0-9.]+)", open(HEADER).read())
    assert m and float(m.group(1)) == default and default >= 0
    for text, want in (("7.5", 7.5), ("0", 0.0), ("1e3", 1000.0), ("12 ", 12.0), ("abc", default), ("", default), ("-3", default)):
        monkeypatch.setenv("OTTI_INGEST_WIT_MIN_MB", text)
        assert f() == want, text
