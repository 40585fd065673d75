"""The one ending every mutator of the resident witness shares (witness.cpp DeviceWitness::z_written), on a witness that keeps BOTH rows and products:
update, scatter, assign (patch and re-sum forced) and set_inputs each bring small_fraction, the kept rows, the kept products and exactly their own
counters along, and launch exactly what they launched before they shared that ending.

ell = 5 (V = 32, four rows of R = 8) and ell = 10, as the sibling tests.  Every mutator but set_inputs makes the same change on a fresh witness: the last
element of row 1 and the first of row 2 (a change that straddles a row boundary and leaves rows 0 and 3 alone), values below 2^40; set_inputs changes
the inputs alone.  The judges: a fresh upload of the new values (small_fraction, check_sat, proof) and the CPU oracle (proof), each computed once."""
import ctypes

import numpy as np
import pytest

import otti_amd as oa
from witness_cases import SEED, Case, Dev, bytes32, values

pytestmark = pytest.mark.gpu
C32, I64 = oa.WIT_CANONICAL32, oa.WIT_I64
_vp = ctypes.c_void_p
NEW = [(1 << 39) + 12345, 77]                                      # the two new values, below 2^40
NEW_INPUTS = [5, 1 << 33]

# Non-zero launch counts per kernel class of ONE mutator call, by (ell, mutator); a host and a device source launch the same.  Taken from commit 70c7bf6
# (the parent of the change that gave the mutators their shared ending) by running these same calls there: the ending may neither add nor drop a launch.
_RESUM = {5: dict(msm_small=1), 10: dict(msm_small=1, msm_finish=1)}       # rows 1 and 2 summed again: two rows, the latency-bound kernel
LAUNCHES = {}
for _ell in (5, 10):
    LAUNCHES[(_ell, "update")] = dict(_RESUM[_ell], spmv=2, other=1)
    LAUNCHES[(_ell, "scatter")] = dict(spmv=2, other=3)
    LAUNCHES[(_ell, "assign_patch")] = dict(spmv=2, other=4)
    LAUNCHES[(_ell, "assign_resum")] = dict(_RESUM[_ell], spmv=2, other=2)
    LAUNCHES[(_ell, "set_inputs")] = dict(spmv=1)


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


class State:
    """one size: the start values, the two changed assignments with their oracle proofs and fresh uploads"""

    def __init__(self, ell):
        self.c = c = Case(ell)                                     # its own handles: a table other modules rebuild under another window launches otherwise
        with pytest.MonkeyPatch.context() as mp:                    # LAUNCHES below holds for the window these sizes get by default (c = 12: 22 windows)
            mp.setenv("OTTI_MSM_WINDOW", "12")
            c.inst.prepare_device(c.gens)
        assert c.gens.table_info[0] == 12
        self.start = values(np.random.default_rng(5 + ell), c.V, "mixed")
        self.at = [2 * c.R - 1, 2 * c.R]                           # the last element of row 1, the first of row 2
        assert all(self.start[j] != x for j, x in zip(self.at, NEW))
        self.moved = list(self.start)
        for j, x in zip(self.at, NEW):
            self.moved[j] = x
        self.new_inputs32 = bytes32(NEW_INPUTS)
        self.ref = {}
        for kind, cur, inputs32 in (("vars", self.moved, None), ("inputs", self.start, self.new_inputs32)):
            label = b"mutators, " + kind.encode()
            fresh = oa.Witness(c.inst, oa.VarsAssignment.new(bytes32(cur)), oa.InputsAssignment.new(c.inputs32 if inputs32 is None else inputs32))
            want = c.want(cur, label, inputs32=inputs32)
            assert oa.NIZK.prove(c.inst, fresh, None, c.gens, label, SEED).bytes == want, f"2^{ell} {kind}: a fresh upload's proof differs from the oracle's"
            rep = fresh.check_sat(c.inst)
            self.ref[kind] = (label, want, fresh.info[2], (rep.n_unsat, rep.rows.tolist()))


_states = {}


def state_of(ell):
    if ell not in _states:
        _states[ell] = State(ell)
    return _states[ell]


def counters(wit):
    p = wit.products_info()
    return dict(rows_resummed=wit.rows_info()[3], scatter=wit.scatter_info(), assign=wit.assign_info(),
                products=(p["patches"], p["rows_recomputed"], p["full_passes"]))


def add(before, **moves):
    """`before` with the named counters moved by the given amounts, every other one as it was"""
    out = dict(before)
    for k, d in moves.items():
        out[k] = before[k] + d if isinstance(d, int) else tuple(a + b for a, b in zip(before[k], d))
    return out


def mutate(S, wit, name, where):
    c, at = S.c, S.at
    if name == "update":                                          # the range of the two: 32-byte words through the staging buffer, integers straight in
        if where == "host":
            wit.update(c.inst, at[0], bytes32(NEW))
        else:
            d = Dev(np.array(NEW, dtype=np.int64))
            wit.update(c.inst, at[0], (d.addr, 2), fmt=I64)
    elif name == "scatter":
        if where == "host":
            wit.scatter(c.inst, np.array(at, dtype=np.int64), bytes32(NEW))
        else:
            di, ds = Dev(np.array(at, dtype=np.uint64)), Dev(np.array(NEW, dtype=np.int64))
            assert oa.lib.otti_witness_scatter(c.inst._h, wit._h, _vp(di.addr), _vp(ds.addr), 2, I64, 0, 1, None) == 0
    elif name.startswith("assign"):                               # the whole vector, of which the two moved
        if where == "host":
            assert wit.assign(c.inst, bytes32(S.moved)) == 2
        else:
            d = Dev(bytes32(S.moved))
            assert wit.assign(c.inst, (d.addr, c.V), fmt=C32) == 2
    else:
        wit.set_inputs(c.inst, S.new_inputs32)


# what the header documents for each mutator, for two changed variables in two rows whose columns reach two constraints (row j of A and C reads variable j)
PATCHED = dict(products=(1, 2, 0))
MOVES = {
    "update": dict(rows_resummed=2, **PATCHED),
    "scatter": dict(scatter=(1, 2, 2), **PATCHED),
    "assign_patch": dict(assign=(1, 2, 0), scatter=(0, 2, 2), **PATCHED),
    "assign_resum": dict(assign=(1, 2, 1), rows_resummed=2, **PATCHED),
    "set_inputs": dict(),                                          # no constraint reads an input column here: nothing to recompute
}
CALLS = [(n, w) for n in ("update", "scatter", "assign_patch", "assign_resum") for w in ("host", "device")] + [("set_inputs", "host")]


@pytest.mark.parametrize("name,where", CALLS)
@pytest.mark.parametrize("ell", [5, 10])
def test_every_mutator_brings_the_derived_state_along(monkeypatch, ell, name, where):
    monkeypatch.delenv("OTTI_PRODUCTS_FULL_SHARE", raising=False)
    monkeypatch.delenv("OTTI_ASSIGN_RESUM_SHARE", raising=False)
    if name.startswith("assign"):
        monkeypatch.setenv("OTTI_ASSIGN_RESUM_SHARE", "2" if name == "assign_patch" else "0")
    S = state_of(ell)
    c = S.c
    wit = c.host_witness(S.start)
    wit.keep_rows(c.inst, c.gens)
    wit.keep_products(c.inst)
    assert wit.rows_info()[:3] == (True, c.L, c.R) and wit.products_info()["kept"]
    before = counters(wit)
    oa.stats_enable(True)
    try:
        mutate(S, wit, name, where)
        launches = {k: v[0] for k, v in oa.stats_read().items() if v[0]}
    finally:
        oa.stats_enable(False)
    after = counters(wit)
    print("launches", (ell, name, where), launches)
    assert after == add(before, **MOVES[name]), (before, after)
    label, want, small_fraction, sat = S.ref["inputs" if name == "set_inputs" else "vars"]
    assert wit.info[2] == small_fraction
    rep = wit.check_sat(c.inst)
    assert (rep.n_unsat, rep.rows.tolist()) == sat
    assert oa.NIZK.prove(c.inst, wit, None, c.gens, label, SEED).bytes == want
    assert counters(wit) == after                                 # proofs and checks only read
    assert launches == LAUNCHES[(ell, name)]
