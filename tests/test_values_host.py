"""Instance.set_values (otti_instance_set_values) where it needs no GPU: the plain route on an Instance.new instance — host lists converted and
replaced, the device copy dropped — against Instance.new on the new triples, the library's host is_sat and the oracle; the symbols; the refusals;
and the row rule of otti_comp_comm_revalue (otti_amd/csrc/value_rows.h) under the address and undefined-behaviour sanitizers as a stand-alone
program (tests/value_rows_check.cpp: its runtime linked into the program, nothing added to the environment).  Everything is exact."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import otti_amd as oa
import orc
import coo_cases as cc
import values_cases as vc
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
BAD_ARG, NO_DEVICE, INVALID_SCALAR = -21, -20, -5
L = vc.L
Vals = oa.api._CooValues


def test_symbols_exported_declared_and_bound():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", oa.lib_path], text=True)
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    header = re.sub(r"\s+", " ", header)
    want = {
        "otti_instance_set_values": "int32_t otti_instance_set_values(otti_instance *inst, const otti_coo_values vals[3] , int32_t src_on_device, void *stream);",
        "otti_instance_values_info": "int32_t otti_instance_values_info(const otti_instance *inst, uint64_t *generation, int32_t *slots_resident, uint64_t *slot_bytes, double ms[3] );",
        "otti_comp_comm_revalue": "int32_t otti_comp_comm_revalue(otti_comp_comm *comm, otti_instance *inst, otti_snark_gens *gens);",
    }
    for name, decl in want.items():
        assert re.search(r"\bT %s\b" % name, syms), name
        assert decl in header, name
        assert getattr(oa.lib, name).restype is ctypes.c_int32
    assert "typedef struct { const void *val; size_t n; int32_t val_format; size_t val_stride_bytes; } otti_coo_values;" in header
    assert [f[0] for f in Vals._fields_] == ["val", "n", "val_format", "val_stride_bytes"]
    for cls, name in ((oa.Instance, "set_values"), (oa.Instance, "values_info"), (oa.ComputationCommitment, "revalue")):
        assert hasattr(cls, name), name


def _new(s, vals):
    return oa.Instance.new(*s.dims(), *s.entry_arrays(vals))


def _same_entries(got, want):
    for k in range(3):
        a, b = got.entries(k), want.entries(k)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), k


def _assignment(s):
    return oa.VarsAssignment.new(s.vars32()), oa.InputsAssignment.new(s.inputs32())


@pytest.mark.parametrize("name", sorted(vc.STRUCTURES))
def test_plain_route_gives_the_instance_of_the_new_triples(name):
    s = vc.STRUCTURES[name]
    assert s.satisfied(s.V0) == []
    inst = _new(s, s.V0)
    assert inst.values_info() == dict(generation=0, slots_resident=False, slot_bytes=0, ms=(0.0, 0.0, 0.0))
    vars_, inputs = _assignment(s)
    assert inst.is_sat(vars_, inputs)
    gen = 0
    for scale in vc.scales(name):
        V1 = s.V1(scale)
        assert s.satisfied(V1) == [] and V1[0] != s.V0[0]
        inst.set_values(*[vc.value_list(cc.C32, 32, xs)[0] for xs in V1])
        gen += 1
        _same_entries(inst, _new(s, V1))
        assert inst.is_sat(vars_, inputs)
        assert orc.OInstance(*s.dims(), *[inst.entries(k) for k in range(3)]).is_sat(s.vars32(), s.inputs32())
        assert inst.values_info()["generation"] == gen
    if s.broken:
        V2 = s.V2()
        assert s.satisfied(V2) == s.broken and len(s.broken) == min(3, s.nc)
        inst.set_values(C=vc.value_list(cc.C32, 32, V2[2])[0], A=vc.value_list(cc.C32, 32, V2[0])[0])      # B keeps V1's, which are V0's
        gen += 1
        _same_entries(inst, _new(s, V2))
        assert not inst.is_sat(vars_, inputs)
        assert not orc.OInstance(*s.dims(), *[inst.entries(k) for k in range(3)]).is_sat(s.vars32(), s.inputs32())
    info = inst.values_info()
    assert info["generation"] == gen and not info["slots_resident"] and info["slot_bytes"] == 0


@pytest.mark.parametrize("val_format,stride", vc.format_params())
def test_plain_route_in_every_format_and_stride(val_format, stride):
    """V0 -> V1 (small) -> V0 on the structure whose A holds the ends of the int64 range; a list the format cannot hold travels as canonical bytes"""
    s = vc.STRUCTURES["quad1280"]
    inst = _new(s, s.V0)
    used = set()
    for vals in (s.V1("small"), s.V0):
        arrays = [vc.value_list(val_format, stride, xs) for xs in vals]
        assert [f for _, f in arrays] == vc.plan(val_format, vals)
        used |= {f for _, f in arrays}
        assert all(a.strides[0] == stride for a, f in arrays if f == val_format)
        inst.set_values(*[a for a, _ in arrays], montgomery=val_format == cc.M32 and all(f == cc.M32 for _, f in arrays))
        _same_entries(inst, _new(s, vals))
    assert val_format in used
    assert inst.values_info()["generation"] == 2


def test_a_matrix_not_named_is_left_alone():
    s = vc.STRUCTURES["padded40"]
    inst = _new(s, s.V0)
    V1 = s.V1("field")
    inst.set_values(B=vc.value_list(cc.I64, 16, V1[1])[0])
    _same_entries(inst, _new(s, [s.V0[0], V1[1], s.V0[2]]))
    inst.set_values()                                              # nothing named: nothing changes but the generation
    _same_entries(inst, _new(s, [s.V0[0], V1[1], s.V0[2]]))
    assert inst.values_info()["generation"] == 2


def test_refusals_leave_the_instance_as_it_was():
    s = vc.STRUCTURES["padded40"]
    inst = _new(s, s.V0)
    before = [inst.entries(k).tobytes() for k in range(3)]
    V1 = s.V1("field")
    good = [vc.value_list(cc.C32, 32, xs)[0] for xs in V1]
    # a wrong count, in each matrix
    for k in range(3):
        arrays = list(good)
        arrays[k] = arrays[k][:-1]
        with pytest.raises(oa.SpartanError) as err:
            inst.set_values(*arrays)
        assert err.value.code == BAD_ARG and type(err.value) is oa.SpartanError, k
    # a coefficient = l at B[7] and another at C[0]: Instance.new's code and wording, for canonical bytes and for Montgomery words
    for montgomery in (False, True):
        arrays = [vc.value_list(cc.M32 if montgomery else cc.C32, 40, xs)[0] for xs in V1]
        arrays[1][7] = np.frombuffer(int(L).to_bytes(32, "little"), dtype=np.uint8)
        arrays[2][0] = np.frombuffer(int(L).to_bytes(32, "little"), dtype=np.uint8)
        with pytest.raises(oa.R1CSError) as err:
            inst.set_values(*arrays, montgomery=montgomery)
        assert err.value.code == INVALID_SCALAR and str(err.value).endswith(cc.MSG_SCALAR), str(err.value)
    bad_entries = s.entry_arrays(V1)
    bad_entries[1]["val"][7] = np.frombuffer(int(L).to_bytes(32, "little"), dtype=np.uint8)
    with pytest.raises(oa.R1CSError) as new_err:
        oa.Instance.new(*s.dims(), *bad_entries)
    assert (new_err.value.code, str(new_err.value)) == (err.value.code, str(err.value))
    assert [inst.entries(k).tobytes() for k in range(3)] == before
    assert inst.values_info()["generation"] == 0
    # raw argument errors come as BAD_ARG with or without a device; a device source without a device is NO_DEVICE behind them
    f = oa.lib.otti_instance_set_values
    ok = (Vals * 3)()
    assert f(None, ok, 0, None) == BAD_ARG and f(inst._h, None, 0, None) == BAD_ARG
    n = s.nnz()
    for bad in (Vals(None, n[0], cc.C32, 0), Vals(4096, n[0], 7, 0), Vals(4096, n[0], cc.C32, 24), Vals(4096, n[0], cc.I64, 12), Vals(4100, n[0], cc.I64, 0),
                Vals(4096, n[0] + 1, cc.I64, 0)):
        for on_device in (0, 1):
            m = (Vals * 3)()
            m[0] = bad
            assert f(inst._h, m, on_device, None) == BAD_ARG, (bad.val, bad.n, bad.val_format, bad.val_stride_bytes)
    if oa.device_count() < 1:
        m = (Vals * 3)()
        m[0] = Vals(4096, n[0], cc.I64, 0)
        assert f(inst._h, m, 1, None) == NO_DEVICE
    assert [inst.entries(k).tobytes() for k in range(3)] == before and inst.values_info()["generation"] == 0
    inst.set_values(*good)
    _same_entries(inst, _new(s, V1))


def test_value_rows_rule_under_sanitizers(tmp_path):
    exe = host_build.build_check(tmp_path, "value_rows_check.cpp", "value_rows_check", host_build.ASAN_UBSAN, host=False)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"^(\d+) layouts, (\d+) with R > N, (\d+) generator splits, 0 mismatches$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 100 and int(m.group(2)) >= 12 and int(m.group(3)) == 12, tail
