"""otti_instance_host_lists_info, otti_k_decomm_entries and otti_k_shard_filter where no GPU is needed: the symbols and their declarations, the
argument errors that are answered before any device is touched, and what an instance made the usual way reports about its host lists."""
import ctypes
import os
import re
import subprocess

import numpy as np

import otti_amd as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
BAD_ARG = -21


def test_symbols_exported_declared_and_bound_with_the_headers_signatures():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    header = re.sub(r"\s+", " ", header)
    want = {
        "otti_instance_host_lists_info": ("int32_t otti_instance_host_lists_info(const otti_instance *inst, int32_t *materialised, uint64_t *host_bytes);", 3),
        "otti_k_decomm_entries": ("int32_t otti_k_decomm_entries(const uint32_t *h_row, const uint32_t *h_col, const uint8_t *h_val_mont32, size_t n, size_t N, size_t pad_to, "
                                  "uint32_t pad_col, uint32_t *out_row_u32, uint32_t *out_col_u32, uint8_t *out_row_fr, uint8_t *out_col_fr, uint8_t *out_val_fr, "
                                  "float *kernel_ms);", 13),
        "otti_k_shard_filter": ("int32_t otti_k_shard_filter(const uint32_t *h_row, const uint32_t *h_col, const uint8_t *h_val_mont32, size_t n, uint32_t world, uint32_t rank, "
                                "int32_t by_col, uint32_t *out_row, uint32_t *out_col, uint8_t *out_val, size_t *out_n, float *kernel_ms);", 12),
    }
    for name, (decl, nargs) in want.items():
        assert re.search(r"\bT %s\b" % name, syms), name
        assert decl in header, name
        f = getattr(oa.lib, name)
        assert f.restype is ctypes.c_int32 and len(f.argtypes) == nargs, name
    assert callable(oa.Instance.host_lists_info) and callable(oa.kernels.decomm_entries) and callable(oa.kernels.shard_filter)
    # the ingest call the tests pin keeps its five arguments
    assert len(oa.lib.otti_instance_ingest_info.argtypes) == 5


def _fake(n=8):
    """a non-null pointer that is never dereferenced: every call below is refused on its arguments alone"""
    return ctypes.c_void_p(n)


def test_argument_errors_come_before_any_device():
    """(without a device every call that reached the device layer would come back as OTTI_ERR_NO_DEVICE, -20, instead)"""
    p, ms = _fake(), ctypes.c_float(0)
    d = oa.lib.otti_k_decomm_entries
    ok = dict(row=p, col=p, val=p, n=4, N=8, pad_to=4, pad_col=0, o0=p, o1=p, o2=p, o3=p, o4=p)
    def decomm(**kw):
        a = dict(ok, **kw)
        return d(a["row"], a["col"], a["val"], a["n"], a["N"], a["pad_to"], a["pad_col"], a["o0"], a["o1"], a["o2"], a["o3"], a["o4"], ctypes.byref(ms))
    for name in ("row", "col", "val", "o0", "o1", "o2", "o3", "o4"):
        assert decomm(**{name: None}) == BAD_ARG, name
    assert decomm(n=9) == BAD_ARG                                             # n > N
    assert decomm(pad_to=9) == BAD_ARG                                        # pad_to > N
    assert decomm(n=0, N=0, pad_to=0) == BAD_ARG                              # nothing to launch over
    f = oa.lib.otti_k_shard_filter
    cnt = ctypes.c_size_t(77)
    okf = dict(row=p, col=p, val=p, n=4, world=2, rank=1, by_col=0, o0=p, o1=p, o2=p, cnt=ctypes.byref(cnt))
    def filt(**kw):
        a = dict(okf, **kw)
        return f(a["row"], a["col"], a["val"], a["n"], a["world"], a["rank"], a["by_col"], a["o0"], a["o1"], a["o2"], a["cnt"], ctypes.byref(ms))
    for name in ("row", "col", "val", "o0", "o1", "o2", "cnt"):
        assert filt(**{name: None}) == BAD_ARG, name
    for world, rank in ((0, 0), (3, 0), (6, 1), (2, 2), (8, 8), (1, 1)):
        assert filt(world=world, rank=rank) == BAD_ARG, (world, rank)
    assert cnt.value == 77                                                    # untouched by every refusal
    assert oa.lib.otti_instance_host_lists_info(None, None, None) == BAD_ARG
    m, hb = ctypes.c_int32(5), ctypes.c_uint64(5)
    assert oa.lib.otti_instance_host_lists_info(None, ctypes.byref(m), ctypes.byref(hb)) == BAD_ARG and (m.value, hb.value) == (5, 5)


def test_an_instance_made_the_usual_way_has_its_host_lists():
    r = oa.synth_r1cs_compiler_like(100, 3, 4)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    total = int(r["A"].size + r["B"].size + r["C"].size)
    assert inst.host_lists_info() == {"materialised": True, "host_bytes": 40 * total}
    # any out pointer may be NULL
    m, hb = ctypes.c_int32(-1), ctypes.c_uint64(0)
    assert oa.lib.otti_instance_host_lists_info(inst._h, ctypes.byref(m), None) == 0 and m.value == 1
    assert oa.lib.otti_instance_host_lists_info(inst._h, None, ctypes.byref(hb)) == 0 and hb.value == 40 * total
    assert oa.lib.otti_instance_host_lists_info(inst._h, None, None) == 0
    empty = oa.Instance.new(4, 4, 1, np.zeros(0, dtype=oa.api.ENTRY_DTYPE), np.zeros(0, dtype=oa.api.ENTRY_DTYPE), np.zeros(0, dtype=oa.api.ENTRY_DTYPE))
    assert empty.host_lists_info() == {"materialised": True, "host_bytes": 0}
