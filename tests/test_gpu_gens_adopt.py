"""otti_gens_adopt_table: kernels running from a window table that was built for ANOTHER generator handle, with another number of bases.

Every NIZKGens takes its points from one stream and the table is laid out base by base, so a handle may hold the table of a longer one.  What
is pinned here: after adoption both handles report one device address and two users; the proof at a fixed seed, otti_k_msm_rows,
otti_k_bullet_round and kept rows patched by a scatter give the bytes they gave before adoption, which are the CPU oracle's; releasing or
freeing the donor leaves the adopter proving; a donor that released builds its own table again; a handle that never adopted is unchanged.

Sizes cross the `nbases < 256` rule of device_window_bits (prover.cpp): adopters 2^10 (R = 32) and 2^13 (R = 128), donors 2^14 (R = 128: as
many points as the second adopter has) and 2^16 (R = 256).  The window is pinned to 10 bits, so the largest table here is 258 bases."""
import gc

import numpy as np
import pytest

import otti_amd as oa
import orc
from witness_cases import Q, SEED, bytes32, case, values

pytestmark = pytest.mark.gpu
K = oa.kernels
PAIRS = [(10, 14), (10, 16), (13, 14), (13, 16)]


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(autouse=True)
def _small_tables(monkeypatch):
    monkeypatch.setenv("OTTI_MSM_WINDOW", "10")
    monkeypatch.setenv("OTTI_MSM_TABLE_GB", "1")


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


_want = {}


def oracle(ell, rng):
    """per adopter size, computed once and left alone: an assignment, the oracle's proof of it, a commitment and two bullet rounds"""
    if ell not in _want:
        c = case(ell)
        cur = values(rng, c.V)
        Z, bl = orc.rand_fr(rng, 3 * c.R), orc.rand_fr(rng, 3)
        a, b, blinds, us = orc.rand_fr(rng, c.R), orc.rand_fr(rng, c.R), orc.rand_fr(rng, 4), orc.rand_fr(rng, 2)
        idx = sorted(int(j) for j in rng.choice(c.V, size=5, replace=False)); new = values(rng, 5, "large")
        moved = list(cur)
        for j, x in zip(idx, new):
            moved[j] = x
        _want[ell] = dict(cur=cur, proof=c.want(cur, b"adopt"), Z=Z, bl=bl, rows=orc.commit_rows(c.ogens, Z, 3, c.R, bl), a=a, b=b, blinds=blinds, us=us,
                          LR=orc.bullet_reduce(c.ogens, a, b, blinds, us)[0][:2], idx=idx, new=new, moved=moved, proof_moved=c.want(moved, b"scattered"))
    return _want[ell]


def fr_inv(x):
    return orc.fr_from_ints([pow(v, Q - 2, Q) for v in orc.fr_to_ints(x)])


def everything(c, gens, w):
    """what is compared before and after adoption, each against the oracle: (proof, msm rows, bullet L/R of two rounds, proof from kept and patched rows)"""
    R = c.R
    wit = c.host_witness(w["cur"])
    proof = oa.NIZK.prove(c.inst, wit, None, gens, b"adopt", SEED).bytes
    rows, _ = K.msm_rows(gens, w["Z"], 3, R, w["bl"])
    one = np.repeat(orc.fr_from_ints([1]), R, axis=0)
    LR0, a1, b1, s1, _ = K.bullet_round(gens, R, w["a"], w["b"], one, w["blinds"][0:2])
    LR1 = K.bullet_round(gens, R // 2, a1, b1, s1, w["blinds"][2:4], w["us"][0:1], fr_inv(w["us"][0:1]))[0]
    wit.keep_rows(c.inst, gens)
    wit.scatter(c.inst, np.array(w["idx"], dtype=np.int64), bytes32(w["new"]))
    assert wit.rows_info()[:3] == (True, c.L, R)
    moved = oa.NIZK.prove(c.inst, wit, None, gens, b"scattered", SEED).bytes
    assert proof == w["proof"] and eq(rows, w["rows"]) and eq(LR0, w["LR"][0]) and eq(LR1, w["LR"][1]) and moved == w["proof_moved"]
    return proof, rows.tobytes(), LR0.tobytes(), LR1.tobytes(), moved


@pytest.mark.parametrize("a_ell,d_ell", PAIRS)
def test_adoption_changes_no_byte_and_shares_one_table(rng, a_ell, d_ell):
    c, w = case(a_ell), oracle(a_ell, rng)
    gens, donor = oa.NIZKGens.new(c.V, c.V, 2), oa.NIZKGens.new(1 << d_ell, 1 << d_ell, 2)
    assert gens.table_users() == (0, None) and donor.table_users() == (0, None)
    before = everything(c, gens, w)
    own_info, (own_users, own_addr) = gens.table_info, gens.table_users()
    assert own_users == 1 and own_addr and own_info[0] == 10
    gens.adopt_table(donor)                                       # the donor had no table: built as prepare_device builds it
    users, addr = gens.table_users()
    assert (users, addr) == donor.table_users() and users == 2 and addr
    assert gens.table_info == donor.table_info and donor.table_info[0] == 10
    d_R = 1 << (d_ell - d_ell // 2)
    assert donor.table_info[1] * (c.R + 2) == own_info[1] * (d_R + 2)                           # same entry size, the donor's number of bases
    assert everything(c, gens, w) == before
    gens.adopt_table(donor)                                       # again: nothing
    assert gens.table_users() == (2, addr)
    # the donor lets go: the adopter holds the table alone and still proves
    donor.release_device()
    assert donor.table_users() == (0, None) and gens.table_users() == (1, addr)
    assert everything(c, gens, w) == before
    # a donor that released builds its own again, and proves with it (2^14 only: the oracle's proof of a larger circuit takes too long for here)
    if d_ell == 14 and a_ell == 10:
        d = case(14)
        cur = values(rng, d.V)
        assert oa.NIZK.prove(d.inst, d.host_witness(cur), None, donor, b"donor again", SEED).bytes == d.want(cur, b"donor again")
    else:
        oa.lib.otti_prepare_device(None, donor._h)
    (du, da), (gu, ga) = donor.table_users(), gens.table_users()
    assert du == 1 and da and (gu, ga) == (1, addr)
    # the adopter takes the rebuilt one, then the donor handle is freed altogether
    gens.adopt_table(donor)
    assert gens.table_users() == (2, da)
    del donor
    gc.collect()
    assert gens.table_users() == (1, da)
    assert everything(c, gens, w) == before
    # the adopter releases: its next proof builds a table of its own size again
    gens.release_device()
    assert gens.table_users() == (0, None)
    assert everything(c, gens, w) == before
    assert gens.table_info == own_info


def test_a_handle_that_never_adopted_is_unchanged(rng):
    c, w = case(10), oracle(10, rng)
    plain, gens, donor = oa.NIZKGens.new(c.V, c.V, 2), oa.NIZKGens.new(c.V, c.V, 2), oa.NIZKGens.new(1 << 16, 1 << 16, 2)
    before = everything(c, plain, w)
    info, (users, addr) = plain.table_info, plain.table_users()
    gens.adopt_table(donor)
    assert everything(c, gens, w) == before
    assert everything(c, plain, w) == before
    assert plain.table_info == info and plain.table_users() == (users, addr) and users == 1
    assert gens.table_users()[1] != addr


def test_refusals_leave_both_handles_as_they_were():
    small, big = oa.NIZKGens.new(1 << 10, 1 << 10, 2), oa.NIZKGens.new(1 << 16, 1 << 16, 2)
    oa.lib.otti_prepare_device(None, small._h)
    was = small.table_users()
    for args in ((big._h, small._h), (small._h, small._h), (small._h, None), (None, small._h)):
        assert oa.lib.otti_gens_adopt_table(*args) == -21
    assert small.table_users() == was and big.table_users() == (0, None)
