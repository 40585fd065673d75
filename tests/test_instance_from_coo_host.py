"""otti_instance_from_coo / otti_instance_device_entries where no GPU is needed: the symbols, their declarations and bindings, the argument errors
that are answered before any device is touched (the pointers below are never dereferenced), the rule of otti_amd/csrc/coo_walk.h under the
sanitizers as a stand-alone program (tests/coo_walk_check.cpp: its runtime linked into the program, nothing added to the environment), and the
cases of tests/coo_cases.py against Instance.new, which runs on the host."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import otti_amd as oa
import coo_cases as cc
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
BAD_ARG, NO_DEVICE = -21, -20
SENTINEL = 0x5e5e5e5e
Coo = oa.api._Coo


def test_symbols_exported_declared_and_bound_with_the_headers_signatures():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    header = re.sub(r"\s+", " ", header)
    want = {
        "otti_instance_from_coo": "int32_t otti_instance_from_coo(uint64_t num_cons, uint64_t num_vars, uint64_t num_inputs, const otti_coo mats[3] , "
                                  "int32_t src_on_device, void *stream, otti_instance **out);",
        "otti_instance_device_entries": "int32_t otti_instance_device_entries(const otti_instance *inst, int32_t which, const void **d_row, const void **d_col, "
                                        "const void **d_val, size_t *n);",
    }
    for name, decl in want.items():
        assert re.search(r"\bT %s\b" % name, syms), name
        assert decl in header, name
        assert getattr(oa.lib, name).restype is ctypes.c_int32
    assert "enum { OTTI_IDX_U32 = 0, OTTI_IDX_I32 = 1, OTTI_IDX_U64 = 2, OTTI_IDX_I64 = 3 };" in header
    assert "typedef struct { const void *row, *col; const void *val; size_t n; int32_t index_format, val_format; size_t val_stride_bytes; } otti_coo;" in header
    assert (oa.IDX_U32, oa.IDX_I32, oa.IDX_U64, oa.IDX_I64) == (0, 1, 2, 3) == (cc.IDX_U32, cc.IDX_I32, cc.IDX_U64, cc.IDX_I64)
    assert len(oa.lib.otti_instance_from_coo.argtypes) == 7 and len(oa.lib.otti_instance_device_entries.argtypes) == 6
    assert [f[0] for f in Coo._fields_] == ["row", "col", "val", "n", "index_format", "val_format", "val_stride_bytes"]
    assert ctypes.sizeof(Coo) == 3 * ctypes.sizeof(ctypes.c_void_p) + ctypes.sizeof(ctypes.c_size_t) + 8 + ctypes.sizeof(ctypes.c_size_t)
    for name in ("from_coo", "device_entries"):
        assert hasattr(oa.Instance, name), name


def _mats(**changes):
    """three valid descriptions over a fake address (never dereferenced), matrix 1 changed"""
    m = (Coo * 3)()
    for k in range(3):
        m[k] = Coo(4096, 8192, 16384, 5, cc.IDX_I64, cc.I64, 0)
    for key, value in changes.items():
        setattr(m[1], key, value)
    return m


def _call(mats, dims=(8, 8, 2), on_device=1, out=None):
    out = ctypes.c_void_p(SENTINEL) if out is None else out
    rc = oa.lib.otti_instance_from_coo(*dims, mats, on_device, None, ctypes.byref(out))
    assert out.value == SENTINEL
    return rc


def test_argument_errors_come_before_any_device():
    """every one of them is BAD_ARG with or without a GPU: said before NO_DEVICE, for a device and for a host source alike"""
    f = oa.lib.otti_instance_from_coo
    out = ctypes.c_void_p(SENTINEL)
    assert f(8, 8, 2, None, 1, None, ctypes.byref(out)) == BAD_ARG
    assert f(8, 8, 2, _mats(), 1, None, None) == BAD_ARG
    for on_device in (0, 1):
        for field in ("row", "col", "val"):
            assert _call(_mats(**{field: None}), on_device=on_device) == BAD_ARG, field                 # a null array with a non-zero n
        for fmt in (-1, 4, 99):
            assert _call(_mats(index_format=fmt), on_device=on_device) == BAD_ARG
            assert _call(_mats(val_format=fmt), on_device=on_device) == BAD_ARG
            assert _call(_mats(index_format=fmt, n=0), on_device=on_device) == BAD_ARG                   # judged whatever n is
        for fmt, stride in ((cc.I64, 4), (cc.U64, 7), (cc.I64, 12), (cc.C32, 8), (cc.C32, 24), (cc.M32, 31), (cc.C32, 36), (cc.M32, 33)):
            assert _call(_mats(val_format=fmt, val_stride_bytes=stride), on_device=on_device) == BAD_ARG, (fmt, stride)
        # alignment to the element: 4 or 8 bytes for indices, 8 for every coefficient format
        for fmt, addr in ((cc.IDX_U32, 4098), (cc.IDX_I32, 4097), (cc.IDX_U64, 4100), (cc.IDX_I64, 4100)):
            assert _call(_mats(index_format=fmt, row=addr), on_device=on_device) == BAD_ARG, (fmt, addr)
            assert _call(_mats(index_format=fmt, col=addr), on_device=on_device) == BAD_ARG, (fmt, addr)
        for fmt in (cc.C32, cc.M32, cc.I64, cc.U64):
            assert _call(_mats(val_format=fmt, val=16388), on_device=on_device) == BAD_ARG, fmt
        for n in (2 ** 32, 2 ** 32 + 1, 2 ** 63):
            assert _call(_mats(n=n), on_device=on_device) == BAD_ARG, n
        for dims in ((2 ** 30 + 1, 8, 2), (8, 2 ** 30 + 1, 2), (8, 8, 2 ** 30), (2 ** 64 - 1, 8, 2), (8, 2 ** 64 - 1, 2), (8, 8, 2 ** 64 - 1)):
            assert _call(_mats(), dims=dims, on_device=on_device) == BAD_ARG, dims
            assert "instance too large for 32-bit indices" in oa.api._last_error()
    e = oa.lib.otti_instance_device_entries
    n = ctypes.c_size_t(7)
    assert e(None, 0, None, None, None, ctypes.byref(n)) == BAD_ARG and n.value == 7


@pytest.mark.parametrize("on_device", [0, 1])
def test_valid_arguments_without_a_device_are_no_device(on_device):
    if oa.device_count() > 0:
        return                                                  # with a device the fake addresses would be read: test_gpu_instance_from_coo.py runs the real thing
    assert _call(_mats(), on_device=on_device) == NO_DEVICE
    assert _call(_mats(index_format=cc.IDX_U32, row=4100, col=4100, val_format=cc.M32, val_stride_bytes=40), on_device=on_device) == NO_DEVICE
    assert _call(_mats(n=0, row=None, col=None, val=None), on_device=on_device) == NO_DEVICE
    assert _call(_mats(), dims=(2 ** 30, 2 ** 30, 2 ** 30 - 1), on_device=on_device) == NO_DEVICE      # the largest dimensions Instance.new takes
    case = cc.count_case(5, 6, 7)
    with pytest.raises(oa.NoDeviceError):
        oa.Instance.from_coo(*case.dims(), *case.arrays())


def test_an_instance_made_on_the_host_keeps_no_device_lists():
    case = cc.count_case(5, 6, 7)
    inst = oa.Instance.new(*case.dims(), *case.entry_arrays())
    for k in range(3):
        assert inst.device_entries(k) == (0, 0, 0, 0)
    r, n = ctypes.c_void_p(SENTINEL), ctypes.c_size_t(7)
    assert oa.lib.otti_instance_device_entries(inst._h, 3, ctypes.byref(r), None, None, ctypes.byref(n)) == BAD_ARG and (r.value, n.value) == (SENTINEL, 7)
    assert oa.lib.otti_instance_device_entries(inst._h, -1, None, None, None, None) == BAD_ARG
    assert oa.lib.otti_instance_device_entries(inst._h, 0, None, None, None, None) == 0


def test_the_wrapper_refuses_what_it_can_see():
    case = cc.count_case(5, 6, 7)
    A, B, C = case.arrays()
    with pytest.raises(ValueError):
        oa.Instance.from_coo(*case.dims(), A, B, (C[0], C[1].astype(np.int32), C[2]))                   # two index dtypes in one matrix
    with pytest.raises(ValueError):
        oa.Instance.from_coo(*case.dims(), A, B, (C[0], C[1], C[2].astype(np.float64)))
    with pytest.raises(ValueError):
        oa.Instance.from_coo(*case.dims(), A, B, (C[0], C[1], C[2][:-1]))
    with pytest.raises(ValueError):
        oa.Instance.from_coo(*case.dims(), A, B, C, montgomery=True)                                    # integers are never Montgomery words

    class OnGpu:                                               # a stand-in for a GPU tensor: the mix is refused before anything else is looked at
        is_cuda = True
    import sys
    import types
    fake = types.SimpleNamespace(Tensor=OnGpu)
    had = sys.modules.get("torch")
    sys.modules["torch"] = fake
    try:
        with pytest.raises(oa.SpartanError) as err:
            oa.Instance.from_coo(*case.dims(), A, B, (C[0], C[1], OnGpu()))
        assert err.value.code == BAD_ARG and type(err.value) is oa.SpartanError
    finally:
        if had is None:
            del sys.modules["torch"]
        else:
            sys.modules["torch"] = had


def test_rule_agrees_with_a_sequential_walk_under_sanitizers(tmp_path):
    exe = host_build.build_check(tmp_path, "coo_walk_check.cpp", "coo_walk_check", host_build.ASAN_UBSAN, host=False)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"^(\d+) placements, (\d+) runs, 0 mismatches$", r.stdout, re.M)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) >= 4000, tail


def _all_valid_cases():
    out = [cc.count_case(*p) for p in cc.count_params()] + [cc.format_case(*p) for p in cc.format_params()]
    return out + [cc.padding_case(*p) for p in cc.PADDINGS] + [cc.order_case()]


def test_expected_lists_agree_with_instance_new():
    """the (row, padded column, canonical value) lists a from_coo instance has to keep, against the entries Instance.new keeps for the same triples
    (otti_instance_entries gives the caller's columns back: the padding is undone by the case's own rule, and checked to be the instance's)"""
    for case in _all_valid_cases():
        inst = oa.Instance.new(*case.dims(), *case.entry_arrays())
        assert inst.dims == (case.ncp, case.nvp, case.ni), case.name
        arrays = case.arrays()
        for k in range(3):
            got, want = inst.entries(k), case.expected(k)
            assert got.shape[0] == len(want) == len(arrays[k][0]), case.name
            assert got["row"].tolist() == [r for r, _, _ in want], case.name
            assert got["col"].tolist() == [case.col_unshifted(c) for _, c, _ in want], case.name
            assert all(c < case.nv or case.nvp <= c < case.nvp + 1 + case.ni for _, c, _ in want), case.name
            assert got["val"].tobytes() == b"".join(v.to_bytes(32, "little") for _, _, v in want), case.name
            # the arrays themselves hold what the triples say, in the format's own encoding and at the stride asked for
            rows, cols, vals = arrays[k]
            assert rows.dtype == cols.dtype == cc.INDEX_DTYPE[case.index_format]
            assert [int(x) for x in rows] == [r for r, _, _ in case.triples[k]] and [int(x) for x in cols] == [c for _, c, _ in case.triples[k]]
            if len(want) > 1:
                assert vals.strides[0] == (case.stride or (8 if case.val_format in (cc.I64, cc.U64) else 32))
            if case.val_format in (cc.I64, cc.U64):
                assert [int(x) % cc.L for x in vals] == [v for _, _, v in want]
            elif case.val_format == cc.C32:
                assert vals.tobytes() == got["val"].tobytes()
            else:
                assert [int.from_bytes(vals[i].tobytes(), "little") * sc_rinv() % cc.L for i in range(len(want))] == [v for _, _, v in want]


def sc_rinv():
    return pow(cc.R, -1, cc.L)


def test_error_cases_are_refused_by_instance_new_where_it_can_take_them():
    """each refusal case names the first defect of a sequential walk (in Python integers here); where the triples fit otti_entry — no negative index —
    Instance.new refuses them with the same code and message"""
    for name, build, code, msg in cc.error_cases():
        dims, arrays = build()
        fmts = [cc.C32 if a[2].ndim == 2 else cc.I64 for a in arrays]
        assert cc.sequential_first_error(dims, arrays, fmts) == (code, msg), name
        if any(int(x) < 0 for a in arrays for x in np.concatenate([a[0], a[1]])) or name.startswith("montgomery"):
            continue
        ents = []
        for rows, cols, vals in arrays:
            e = np.zeros(len(rows), dtype=oa.ENTRY_DTYPE)
            e["row"], e["col"] = rows.astype(np.uint64), cols.astype(np.uint64)
            e["val"] = vals if vals.ndim == 2 else np.frombuffer(b"".join((int(x) % cc.L).to_bytes(32, "little") for x in vals), dtype=np.uint8).reshape(-1, 32)
            ents.append(e)
        with pytest.raises(oa.R1CSError) as err:
            oa.Instance.new(*dims, *ents)
        assert err.value.code == code and msg in str(err.value), name
