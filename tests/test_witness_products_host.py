"""What kept products (otti_witness_keep_products, otti_witness_drop_products, otti_witness_products_info, otti_k_products_patch) promise without a
GPU: exported, declared and bound symbols, argument errors answered before any device is touched (the witness pointers below are never
dereferenced), OTTI_ERR_NO_DEVICE for valid arguments without a device — and the model the GPU tests judge the patch by (products_cases.py: touched
rows = rows with an entry of A, B or C in a changed column) held against SparseCase.multiply_vec on every case those tests use: outside the touched
set no sum moves."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import otti_amd as oa
import products_cases as pc
import sparse_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
NAMES = ("otti_witness_keep_products", "otti_witness_drop_products", "otti_witness_products_info", "otti_k_products_patch")
BAD_ARG, NO_DEVICE, INVALID_INDEX = -21, -20, -6
SENTINEL = 0x5e5e5e5e
_vp = ctypes.c_void_p


def _inst(n=8, ni=2):
    r = oa.synth_r1cs(n, ni, 1)
    return oa.Instance.new(n, n, ni, r["A"], r["B"], r["C"])


def _last_error():
    buf = ctypes.create_string_buffer(256)
    oa.lib.otti_last_error(buf, 256)
    return buf.value


def test_symbols_exported_declared_and_bound():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, syms), name
        assert re.search(r"int32_t\s+%s\s*\(" % name, header), name
        assert hasattr(oa.lib, name)
    for name in ("keep_products", "drop_products", "products_info"):
        assert hasattr(oa.Witness, name), name
    assert hasattr(oa.kernels, "products_patch")


def test_header_states_the_contract():
    text = " ".join(open(HEADER).read().split())
    i = text.index("kept products: a resident witness")
    block = text[i:text.index("int32_t otti_witness_keep_products(", i)]
    for phrase in ("96 * N + N / 8 bytes", "OTTI_PRODUCTS_FULL_SHARE", "byte-identical with and without kept products", "Sharded provers ignore them",
                   "must outlive the kept products", "another instance"):
        assert phrase in block, phrase


def _patch_args(inst, n=8, cols=None, ncols=0, first=0, count=0, z=True):
    """arguments of otti_k_products_patch for an instance of n constraints = variables; the buffers are kept alive by the returned list"""
    zb = np.zeros((2 * n, 32), dtype=np.uint8)
    abc = [np.zeros((n, 32), dtype=np.uint8) for _ in range(3)]
    bits, unsat = np.zeros((n + 63) // 64, dtype=np.uint64), ctypes.c_uint64(SENTINEL)
    rows, nt, full = np.zeros(n, dtype=np.uint32), ctypes.c_uint64(SENTINEL), ctypes.c_int32(SENTINEL)
    p = lambda a: a.ctypes.data_as(_vp)
    args = [inst, p(zb) if z else None, p(cols) if cols is not None else None, ncols, first, count, p(abc[0]), p(abc[1]), p(abc[2]), p(bits), ctypes.byref(unsat),
            p(rows), n, ctypes.byref(nt), ctypes.byref(full), None]
    return args, (zb, abc, bits, unsat, rows, nt, full, cols)


def test_argument_errors_come_before_any_device():
    inst = _inst()
    fake_wit = ctypes.c_void_p(1)                              # never dereferenced: every case below is refused on its arguments alone
    keep, drop, info, patch = (getattr(oa.lib, n) for n in NAMES)
    assert keep(None, fake_wit) == BAD_ARG
    assert keep(inst._h, None) == BAD_ARG
    assert drop(None) == BAD_ARG
    kept, n = ctypes.c_int32(SENTINEL), ctypes.c_size_t(SENTINEL)
    u = ctypes.c_uint64(SENTINEL)
    assert info(None, ctypes.byref(kept), ctypes.byref(n), None, None, None, ctypes.byref(u), None, None, None) == BAD_ARG
    assert info(None, None, None, None, None, None, None, None, None, None) == BAD_ARG
    assert (kept.value, n.value, u.value) == (SENTINEL,) * 3
    # the kernel-level entry: null arguments, then the column list judged on the host — strictly ascending and below 2 * num_vars
    args, keepalive = _patch_args(None, cols=np.array([1], dtype=np.uint64), ncols=1)
    assert patch(*args) == BAD_ARG
    args, keepalive = _patch_args(inst._h, z=False)
    assert patch(*args) == BAD_ARG
    args, keepalive = _patch_args(inst._h, cols=None, ncols=3)           # a count without a list
    assert patch(*args) == BAD_ARG
    for bad in ([3, 3], [4, 2], [1, 16], [0, 2 ** 63]):
        args, keepalive = _patch_args(inst._h, cols=np.array(bad, dtype=np.uint64), ncols=len(bad))
        assert patch(*args) == INVALID_INDEX, bad
        assert b"strictly ascending" in _last_error()
        assert keepalive[3].value == SENTINEL and keepalive[5].value == SENTINEL
    for first, count in ((17, 0), (10, 7), (0, 2 ** 63)):
        args, keepalive = _patch_args(inst._h, first=first, count=count)
        assert patch(*args) == INVALID_INDEX, (first, count)


@pytest.mark.skipif(oa.device_count() > 0, reason="only meaningful without a GPU")
def test_valid_arguments_without_a_device_are_no_device():
    inst = _inst()
    fake_wit = ctypes.c_void_p(1)
    assert oa.lib.otti_witness_keep_products(inst._h, fake_wit) == NO_DEVICE
    # without a device no witness handle can exist: such a pointer is rejected, not read
    kept = ctypes.c_int32(SENTINEL)
    assert oa.lib.otti_witness_products_info(fake_wit, ctypes.byref(kept), None, None, None, None, None, None, None, None) == NO_DEVICE
    assert kept.value == SENTINEL
    assert oa.lib.otti_witness_drop_products(fake_wit) == NO_DEVICE
    args, keepalive = _patch_args(inst._h, cols=np.array([1, 5], dtype=np.uint64), ncols=2)
    assert oa.lib.otti_k_products_patch(*args) == NO_DEVICE
    args, keepalive = _patch_args(inst._h, first=3, count=4)
    assert oa.lib.otti_k_products_patch(*args) == NO_DEVICE
    w = oa.Witness._adopt(fake_wit)
    try:
        with pytest.raises(oa.NoDeviceError):
            w.keep_products(inst)
        with pytest.raises(oa.NoDeviceError):
            w.products_info()
        with pytest.raises(oa.NoDeviceError):
            w.drop_products()
    finally:
        w._h = None                                            # not a handle: nothing to free


# ------------------------------------------------------------------------------------------------ the model
def test_marker_is_no_field_element():
    assert pc.MARKER_WORD >= sc.L and pc.marker_rows(3).tobytes() == bytes([0xa5]) * 96


def test_edge_case_touches_what_it_is_built_to_touch():
    case = pc.edges_case()
    assert (case.ncp, case.nvp) == (256, 64)
    for name, (cols, rows) in pc.EDGE_CHANGES.items():
        assert pc.touched_rows(case, cols) == rows, name
    ln = case.lengths(by_col=True)
    assert not ln[:, 2].any()                                  # three empty lists


def test_ladder_changes_meet_every_cut_over():
    case = sc.ladder_case("lane", 1, "codes", transposed=True)
    assert [n for n, _ in pc.columns_by_length(case, 1)] == list(sc.LADDER)
    for layout in ("lane", "quad"):
        case = sc.ladder_case(layout, 2, "nocodes")
        ln = case.lengths()[2]
        for n, col in pc.columns_by_row_length(case, 2):
            rows = pc.touched_rows(case, [col])
            assert any(ln[r] == n for r in rows), (layout, n, col)


def test_model_agrees_with_multiply_vec_on_every_case():
    """rows outside the touched set have equal sums before and after the change; with values that differ, the change shows somewhere inside it unless
    every list of the column is empty"""
    n_cases = n_changes = 0
    for case, changes in pc.kernel_cases():
        before = case.multiply_vec()
        n_cases += 1
        for cols in changes:
            assert all(0 <= c < 2 * case.nvp for c in cols) and sorted(set(cols)) == list(cols), (case.name, cols)
            rows = pc.touched_rows(case, cols)
            z_new = pc.changed_z(case, case.z, cols)
            assert all((z_new[i] != case.z[i]) == (i in cols) for i in range(2 * case.nvp))
            after = case.multiply_vec(z_new)
            inside = set(rows)
            moved = {r for k in range(3) for r in range(case.ncp) if before[k][r] != after[k][r]}
            assert moved <= inside, (case.name, cols, sorted(moved - inside)[:8])
            assert bool(moved) == bool(rows), (case.name, cols)
            n_changes += 1
    assert n_cases >= 24 and n_changes >= 13 * 18
