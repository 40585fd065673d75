"""What otti_gens_adopt_table and otti_gens_table_users promise without a GPU: exported, declared and bound symbols, the sharing rules in the
header, refusals answered before any device is touched, and OTTI_ERR_NO_DEVICE after them."""
import ctypes
import os
import re
import subprocess

import pytest

import otti_amd as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "otti_spartan.h")
NAMES = ("otti_gens_adopt_table", "otti_gens_table_users")
BAD_ARG, NO_DEVICE = -21, -20


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
    assert hasattr(oa.NIZKGens, "adopt_table") and hasattr(oa.NIZKGens, "table_users")


def test_header_states_the_sharing_rules():
    text = " ".join(open(HEADER).read().replace(" * ", " ").split())
    i = text.index("one device table for several generator handles")
    block = text[i:text.index("int32_t otti_gens_table_users(", i)]
    for phrase in ("shared ownership", "freed with its last reference", "before any device is touched", "gens == donor", "fewer points than gens needs",
                   "another stream label", "then OTTI_ERR_NO_DEVICE", "same donor: OTTI_OK, nothing done", "kept rows belong to the points and stay valid",
                   "never while a proof with either handle is running", "builds a table of its own", "SNARK generators (otti_snark_gens) share nothing"):
        assert phrase in block, phrase


def test_refusals_come_before_any_device():
    small, big = oa.NIZKGens.new(1 << 10, 1 << 10, 2), oa.NIZKGens.new(1 << 14, 1 << 14, 2)
    adopt = oa.lib.otti_gens_adopt_table
    assert adopt(None, big._h) == BAD_ARG and adopt(small._h, None) == BAD_ARG and adopt(None, None) == BAD_ARG
    assert adopt(small._h, small._h) == BAD_ARG and b"own table" in _last_error()
    assert adopt(big._h, small._h) == BAD_ARG and b"fewer points" in _last_error()      # the donor is the smaller one
    with pytest.raises(oa.SpartanError):
        big.adopt_table(small)
    # nothing was built, nothing is shared
    for g in (small, big):
        assert g.table_users() == (0, None) and g.table_info == (0, 0)
    assert oa.lib.otti_gens_table_users(None, None, None) == BAD_ARG
    assert oa.lib.otti_gens_table_users(small._h, None, None) == 0


@pytest.mark.skipif(oa.device_count() > 0, reason="only meaningful without a GPU")
def test_valid_arguments_without_a_device_are_no_device():
    small, big, same = oa.NIZKGens.new(1 << 10, 1 << 10, 2), oa.NIZKGens.new(1 << 14, 1 << 14, 2), oa.NIZKGens.new(1 << 10, 1 << 10, 2)
    assert oa.lib.otti_gens_adopt_table(small._h, big._h) == NO_DEVICE
    assert oa.lib.otti_gens_adopt_table(small._h, same._h) == NO_DEVICE                   # as many points as the adopter has: enough
    with pytest.raises(oa.NoDeviceError):
        small.adopt_table(big)
    assert small.table_users() == (0, None) and big.table_users() == (0, None)
