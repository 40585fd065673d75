"""Instance.set_values (otti_instance_set_values, k_revalue.hip) and ComputationCommitment.revalue (otti_comp_comm_revalue) against a FRESH instance
built from the same rows and columns with the new coefficients: the same entries, the same variants on both CSR copies, the same products and
evaluations (also against Python integers), the same NIZK proof bytes (also the oracle's), the same SNARK commitment and proof bytes.  Everything is
exact: bytes and integers, no tolerance.  Structures and coefficient sets: tests/values_cases.py (test_values_host.py runs the plain route on them
without a GPU).  Nothing here is expected to fault: the convert pass reads and writes position i < n of lists of n elements, the place pass writes
at slots that a cursor starting at the copy's own row pointers handed out (all below n), and a refused call writes staging lists alone."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import otti_amd as oa
import orc
import coo_cases as cc
import sparse_cases as sc
import values_cases as vc
import values_tensor_worker as W

pytestmark = pytest.mark.gpu
K = oa.kernels
L, R = vc.L, vc.R
LABEL, SEED = W.LABEL, W.SEED
HERE = os.path.dirname(os.path.abspath(__file__))
BAD_ARG, INVALID_SCALAR = -21, -5
NAMES = sorted(vc.STRUCTURES)


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def _montgomery_words(xs):
    if not xs:
        return []
    words = [int.from_bytes(w.tobytes(), "little") for w in K.from_canonical(sc.bytes32(xs))]
    assert words == [x * R % L for x in xs]
    return words


def _download(ptr, n, dtype, width=None):
    out = np.zeros(n if width is None else (n, width), dtype=dtype)
    if n:
        assert ptr
        assert oa.lib.otti_dev_download(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), out.nbytes) == 0
    return out


def _assignment(s):
    return oa.VarsAssignment.new(s.vars32()), oa.InputsAssignment.new(s.inputs32())


@functools.lru_cache(maxsize=None)
def _gens(name):
    return oa.NIZKGens.new(*vc.STRUCTURES[name].dims())


def _vals(s, which):
    return s.V0 if which == "V0" else s.V2() if which == "V2" else s.V1(which)


_points = W.points


def _evaluate(inst, pts):
    nrx, nry = len(pts[0][0]), len(pts[0][1])
    rx = orc.fr_from_ints([x for p in pts for x in p[0]]).reshape(len(pts), nrx, 32)
    ry = orc.fr_from_ints([x for p in pts for x in p[1]]).reshape(len(pts), nry, 32)
    out, _ = K.instance_evaluate(inst, rx, ry)
    return out.tobytes()


def _observe(inst, s, prove=True):
    """everything the tests compare, short of the entry lists: variants, products, table, evaluations, proof bytes"""
    sp = s.sparse(s.V0)                                           # (the vectors alone: they do not depend on the coefficients)
    obs = dict(info=[inst.device_info(by_col=b) for b in (False, True)],
               mv=[a.tobytes() for a in K.multiply_vec(inst, orc.fr_from_ints(sp.z))[:3]],
               tab=K.eval_table_sparse(inst, orc.fr_from_ints(sp.eq), orc.fr_from_ints(sp.coef))[0].tobytes(),
               ev=_evaluate(inst, _points(s)))
    if prove:
        obs["proof"] = oa.NIZK.prove(inst, *_assignment(s), _gens(s.name), LABEL, SEED).bytes
    return obs


@functools.lru_cache(maxsize=None)
def _fresh(name, which):
    """the reference of one (structure, coefficient set), made once and only read: a fresh from_coo instance's observations and entries, held to
    Python integers, to the variant rules and to the oracle's proof"""
    s = vc.STRUCTURES[name]
    vals = _vals(s, which)
    inst = oa.Instance.from_coo(*s.dims(), *s.coo(vals))
    obs = _observe(inst, s)
    sp = s.sparse(vals)
    assert obs["info"] == [sp.variant(False), sp.variant(True)], (name, which, obs["info"])
    assert obs["mv"] == [orc.fr_from_ints(ints).tobytes() for ints in sp.multiply_vec()], (name, which)
    assert obs["tab"] == orc.fr_from_ints(sp.eval_table()).tobytes(), (name, which)
    shifted = [[(r, sp.col_shifted(c), v) for r, c, v in m] for m in sp.ents]
    want_ev = []
    for rx, ry in _points(s):
        ex, ey = (orc.fr_to_ints(orc.eq_evals(orc.fr_from_ints(r))) for r in (rx, ry))
        want_ev += [sum(v * ex[r] * ey[c] for r, c, v in m) % L for m in shifted]
    assert obs["ev"] == orc.fr_from_ints(want_ev).tobytes(), (name, which)
    ents = s.entry_arrays(vals)
    oinst, ogens = orc.OInstance(*s.dims(), *ents), orc.OGens(*s.dims())
    oproof, _ = orc.nizk_prove(oinst, s.vars32(), s.inputs32(), ogens, LABEL, SEED)
    assert obs["proof"] == oproof, (name, which, "the fresh instance's proof is not the oracle's")
    obs["entries"] = [e.tobytes() for e in ents]
    obs["mont"] = [b"".join((v * R % L).to_bytes(32, "little") for v in xs) for xs in vals]
    return obs


def _assert_is_fresh(inst, s, which, entries=True, verify=False):
    want = _fresh(s.name, which)
    got = _observe(inst, s)
    for key in ("info", "mv", "tab", "ev", "proof"):
        assert got[key] == want[key], (s.name, which, key, got[key] if key == "info" else "")
    if verify:
        oa.NIZK(got["proof"]).verify(inst, oa.InputsAssignment.new(s.inputs32()), _gens(s.name), LABEL)
    if entries:
        assert [inst.entries(k).tobytes() for k in range(3)] == want["entries"], (s.name, which, "entries")


def _arrays(vals, val_format, stride):
    out = [vc.value_list(val_format, stride, xs, raw_of=_montgomery_words) for xs in vals]
    assert [f for _, f in out] == vc.plan(val_format, vals)
    return [a if len(a) else None for a, _ in out]


def test_the_cases_cover_what_they_are_built_for():
    """both directions of the codes flip, the quad layout, both long-list seams by row, the long constant column, every format somewhere"""
    q, h = vc.STRUCTURES["quad1280"], vc.STRUCTURES["heavy"]
    for s in (q, h):
        assert s.sparse(s.V0).variant()["use_small"] and not s.sparse(s.V1("field")).variant()["use_small"] and s.sparse(s.V1("small")).variant()["use_small"]
    assert q.sparse(q.V0).variant()["quad"] and q.sparse(q.V0).variant(True)["n_heavy"] >= 1
    ln = sorted(h.sparse(h.V0).lengths().max(axis=0))[-2:]
    assert ln[0] == 65 and ln[1] > sc.HEAVY_SEG and h.sparse(h.V0).variant()["n_seg"] == 3 and h.sparse(h.V0).variant(True)["n_heavy"] >= 1
    assert vc.plan(cc.I64, q.V0) == [cc.I64, cc.I64, cc.C32] and vc.plan(cc.U64, q.V1("small"))[1] == cc.U64
    assert any(x in q.V0[0] for x in (cc.INT64_MIN % L, cc.INT64_MAX))


# ------------------------------------------------------------------------------------------------ parity: host arrays
@pytest.mark.parametrize("val_format,stride", vc.format_params())
@pytest.mark.parametrize("name", NAMES)
def test_host_arrays_give_the_fresh_instance(name, val_format, stride):
    s = vc.STRUCTURES[name]
    scale = W.scale_for(vc, cc, name, val_format)
    total = sum(s.nnz())
    inst = oa.Instance.from_coo(*s.dims(), *s.coo(s.V0))
    assert inst.values_info() == dict(generation=0, slots_resident=False, slot_bytes=0, ms=(0.0, 0.0, 0.0))
    montgomery = val_format == cc.M32
    inst.set_values(*_arrays(s.V1(scale), val_format, stride), montgomery=montgomery)
    info = inst.values_info()
    assert (info["generation"], info["slots_resident"], info["slot_bytes"]) == (1, True, 8 * total), info
    for k in range(3):                                            # the lists in HBM: the staging list has become the list
        _, _, pv, n = inst.device_entries(k)
        assert n == s.nnz()[k] and _download(pv, n, np.uint8, 32).tobytes() == _fresh(name, scale)["mont"][k], (name, k)
    _assert_is_fresh(inst, s, scale, entries=False)
    assert inst.host_lists_info() == {"materialised": False, "host_bytes": 0}                 # set_values, the kernels and a proof have asked for no host list
    _assert_is_fresh(inst, s, scale, verify=True)                 # ... the host verifier and entries() download them
    assert inst.host_lists_info()["materialised"] is (total > 0)
    # back: the slots are reused, the downloaded host lists refreshed, the original proof bytes restored
    inst.set_values(*_arrays(s.V0, val_format, stride), montgomery=montgomery)
    assert inst.values_info()["generation"] == 2 and inst.values_info()["slot_bytes"] == 8 * total
    _assert_is_fresh(inst, s, "V0")
    inst.set_values(*_arrays(s.V1(scale), val_format, stride), montgomery=montgomery)
    assert inst.values_info()["generation"] == 3
    _assert_is_fresh(inst, s, scale)


@pytest.mark.parametrize("name", ["quad1280", "heavy"])
def test_codes_flip_both_ways_and_stay(name):
    """V0 (codes) -> field scaling (no codes) -> small scaling (codes again, small[] allocated anew) -> V0, with device_info named at every step"""
    s = vc.STRUCTURES[name]
    inst = oa.Instance.from_coo(*s.dims(), *s.coo(s.V0))
    for which, codes in (("field", False), ("small", True), ("V0", True), ("field", False), ("V0", True)):
        inst.set_values(*_arrays(_vals(s, which), cc.C32, 32))
        assert [inst.device_info(by_col=b)["use_small"] for b in (False, True)] == [codes, codes], (name, which)
        _assert_is_fresh(inst, s, which, entries=False)
    # one matrix alone tips the rule: A's wide values against B's and C's that stay
    inst.set_values(A=_arrays(s.V1("field"), cc.C32, 32)[0])
    mixed = s.sparse([s.V1("field")[0], s.V0[1], s.V0[2]])
    assert [inst.device_info(by_col=b) for b in (False, True)] == [mixed.variant(False), mixed.variant(True)]
    assert [a.tobytes() for a in K.multiply_vec(inst, orc.fr_from_ints(mixed.z))[:3]] == [orc.fr_from_ints(x).tobytes() for x in mixed.multiply_vec()]
    inst.set_values(A=_arrays(s.V0, cc.I64, 8)[0])
    _assert_is_fresh(inst, s, "V0")


def test_b_alone_is_replaced():
    s = vc.STRUCTURES["quad1280"]
    inst = oa.Instance.from_coo(*s.dims(), *s.coo(s.V0))
    newB = [(7 * v + 1) % L for v in s.V0[1]]
    inst.set_values(B=vc.value_list(cc.U64, 16, newB)[0])
    want = oa.Instance.from_coo(*s.dims(), *s.coo([s.V0[0], newB, s.V0[2]]))
    assert [inst.entries(k).tobytes() for k in range(3)] == [want.entries(k).tobytes() for k in range(3)]
    a, b = _observe(inst, s), _observe(want, s)
    assert a == b and a["mv"][0] == _fresh(s.name, "V0")["mv"][0] and a["mv"][1] != _fresh(s.name, "V0")["mv"][1]
    assert inst.values_info()["generation"] == 1


# ------------------------------------------------------------------------------------------------ parity: device tensors on a torch stream
_TENSOR_RUN = {}                                                  # "lines" or "failure": the child's one run, whichever way it ended


def _tensor_lines():
    """the child's lines; it is started ONCE per session, and a run that failed — status, fault, time limit — is remembered as a failure: every
    case then fails from what is stored here and none starts another process on the GPU"""
    if not _TENSOR_RUN:
        try:
            res = subprocess.run([sys.executable, os.path.join(HERE, "values_tensor_worker.py")], capture_output=True, text=True, timeout=600)
        except BaseException as e:                                # (a time limit, an interrupt: remembered like a bad status)
            _TENSOR_RUN["failure"] = f"the child did not end: {e!r}"
            raise
        if res.returncode != 0:
            _TENSOR_RUN["failure"] = f"the child ended with status {res.returncode}:\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}"
        else:
            _TENSOR_RUN["lines"] = {tuple(ln.split(" ")[1:4]): ln.split(" ")[4:6] for ln in res.stdout.split("\n") if ln.startswith("case ")}
    assert "failure" not in _TENSOR_RUN, _TENSOR_RUN["failure"] + "\n(the child is not started again)"
    return _TENSOR_RUN["lines"]


@pytest.mark.parametrize("val_format,stride", vc.format_params())
@pytest.mark.parametrize("name", NAMES)
def test_device_tensors_on_a_torch_stream_give_the_fresh_instance(name, val_format, stride):
    """torch has to bring the GPU up before the library is loaded, so the tensors are made and handed over in ONE fresh child process for all cases
    (values_tensor_worker.py); its digests are held against the fresh instances' here"""
    s = vc.STRUCTURES[name]
    got = _tensor_lines().get((name, str(val_format), str(stride)))
    assert got is not None, (name, val_format, stride, "no line from the child")
    want = []
    for which in (W.scale_for(vc, cc, name, val_format), "V0"):
        fresh = oa.Instance.from_coo(*s.dims(), *s.coo(_vals(s, which)))
        assert [fresh.entries(k).tobytes() for k in range(3)] == _fresh(name, which)["entries"]
        want.append(W.digest(oa, fresh, s, _gens(name)))
    assert got == want, (name, val_format, stride)


# ------------------------------------------------------------------------------------------------ refusals
def _upload(a):
    p = ctypes.c_void_p()
    a = np.ascontiguousarray(a)
    assert oa.lib.otti_dev_alloc(max(8, a.nbytes), ctypes.byref(p)) == 0
    assert oa.lib.otti_dev_upload(p, a.ctypes.data_as(ctypes.c_void_p), a.nbytes) == 0
    return p


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("first_call", [True, False])
def test_refusals_leave_the_instance_as_it_was(first_call, on_device):
    """a wrong count, and a coefficient = l at B[7] with another at C[0], on an instance with and without slot maps, from host and device memory"""
    s = vc.STRUCTURES["quad1280"]
    inst = oa.Instance.from_coo(*s.dims(), *s.coo(s.V0))
    if not first_call:
        inst.set_values(*_arrays(s.V1("field"), cc.C32, 32))
        inst.set_values(*_arrays(s.V0, cc.C32, 32))
    gen = inst.values_info()["generation"]
    V1 = s.V1("field")
    for montgomery in (False, True):
        arrays = [vc.value_list(cc.M32 if montgomery else cc.C32, 32, xs, raw_of=_montgomery_words)[0] for xs in V1]
        arrays[1][7] = np.frombuffer(int(L).to_bytes(32, "little"), dtype=np.uint8)
        arrays[2][0] = np.frombuffer(int(L).to_bytes(32, "little"), dtype=np.uint8)
        if on_device:
            ptrs = [_upload(a) for a in arrays]
            m = (oa.api._CooValues * 3)(*[oa.api._CooValues(p, len(a), cc.M32 if montgomery else cc.C32, 0) for p, a in zip(ptrs, arrays)])
            rc = oa.lib.otti_instance_set_values(inst._h, m, 1, None)
            msg = oa.api._last_error()
            for p in ptrs:
                assert oa.lib.otti_dev_free(p) == 0
            assert rc == INVALID_SCALAR and msg.endswith(cc.MSG_SCALAR), (rc, msg)
        else:
            with pytest.raises(oa.R1CSError) as err:
                inst.set_values(*arrays, montgomery=montgomery)
            assert err.value.code == INVALID_SCALAR and str(err.value).endswith(": " + cc.MSG_SCALAR), str(err.value)
    with pytest.raises(oa.SpartanError) as err:
        inst.set_values(A=_arrays(V1, cc.C32, 32)[0][:-1])
    assert err.value.code == BAD_ARG
    info = inst.values_info()
    assert info["generation"] == gen and info["slots_resident"] == (not first_call)
    _assert_is_fresh(inst, s, "V0")                               # multiply_vec, the proof bytes, the variants, the entries: those from before the calls
    inst.set_values(*_arrays(V1, cc.C32, 32))                     # and the context and the instance are as usable as before
    _assert_is_fresh(inst, s, "field")


# ------------------------------------------------------------------------------------------------ other ingest routes
@pytest.mark.parametrize("name", ["padded40", "quad1280"])
def test_device_mode_zkif_instance(name, tmp_path):
    s = vc.STRUCTURES[name]

    def ingest(vals, tag):
        A, B, C = s.entry_arrays(vals)
        paths = [str(tmp_path / (tag + ext)) for ext in (".zkif", ".inp.zkif", ".wit.zkif")]
        oa.zkif_write(dict(num_cons=s.nc, num_vars=s.nv, num_inputs=s.ni, A=A, B=B, C=C, vars=s.vars32(), inputs=s.inputs32()), *paths)
        return oa.Instance.from_zkif(*paths, mode="device")[0]

    inst, want = ingest(s.V0, "v0"), ingest(s.V1("field"), "v1")
    assert inst.dims == want.dims == (s.ncp, s.nvp, s.ni)
    # the instance's own entry order, read from the lists in HBM (asking for entries() would download the host lists)
    new = []
    for k in range(3):
        pr, pc, _, n = inst.device_entries(k)
        rows, cols = _download(pr, n, np.uint32).tolist(), _download(pc, n, np.uint32).tolist()
        value = {(r, c + s.nvp - s.nv if c >= s.nv else c): v for (r, c), v in zip(s.pos[k], s.V1("field")[k])}
        assert len(value) == len(s.pos[k])                        # (no pair twice in these structures)
        new.append([value[rc] for rc in zip(rows, cols)])
    inst.set_values(*[vc.value_list(cc.C32, 32, xs)[0] if xs else None for xs in new])
    for k in range(3):
        (_, _, pv, n), (_, _, wv, wn) = inst.device_entries(k), want.device_entries(k)
        assert n == wn and _download(pv, n, np.uint8, 32).tobytes() == _download(wv, wn, np.uint8, 32).tobytes(), (name, k)
    a, b = _observe(inst, s), _observe(want, s)
    assert a == b and a["proof"] == _fresh(name, "field")["proof"]            # the fresh zkif instance's, the fresh from_coo instance's and the oracle's
    assert inst.values_info()["slots_resident"] and inst.values_info()["generation"] == 1
    assert inst.host_lists_info() == {"materialised": False, "host_bytes": 0}
    oa.NIZK(a["proof"]).verify(inst, oa.InputsAssignment.new(s.inputs32()), _gens(name), LABEL)


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("name", ["dups_zeros", "heavy"])
def test_instance_new_with_a_device_copy_takes_the_plain_route(name, on_device):
    s = vc.STRUCTURES[name]
    inst = oa.Instance.new(*s.dims(), *s.entry_arrays(s.V0))
    inst.prepare_device()
    _assert_is_fresh(inst, s, "V0")
    arrays = _arrays(s.V1("field"), cc.C32, 32)
    if on_device:
        ptrs = [_upload(a) for a in arrays]
        m = (oa.api._CooValues * 3)(*[oa.api._CooValues(p, len(a), cc.C32, 0) for p, a in zip(ptrs, arrays)])
        assert oa.lib.otti_instance_set_values(inst._h, m, 1, None) == 0, oa.api._last_error()
        for p in ptrs:
            assert oa.lib.otti_dev_free(p) == 0
    else:
        inst.set_values(*arrays)
    info = inst.values_info()
    assert info["generation"] == 1 and not info["slots_resident"] and info["slot_bytes"] == 0
    _assert_is_fresh(inst, s, "field", verify=True)
    inst.set_values(*_arrays(s.V0, cc.C32, 32))
    _assert_is_fresh(inst, s, "V0")


# ------------------------------------------------------------------------------------------------ a witness that keeps its products
def test_kept_products_go_stale_and_come_back():
    s = vc.STRUCTURES["quad1280"]
    inst = oa.Instance.from_coo(*s.dims(), *s.coo(s.V0))
    fresh2 = oa.Instance.from_coo(*s.dims(), *s.coo(s.V2()))
    gens = _gens(s.name)
    vars_, inputs = _assignment(s)
    w, wf = oa.Witness(inst, vars_, inputs), oa.Witness(fresh2, vars_, inputs)
    w.keep_products(inst)
    assert w.products_info()["kept"] and w.check_sat(inst).n_unsat == 0
    assert oa.NIZK.prove(inst, w, inputs, gens, LABEL, SEED).bytes == _fresh(s.name, "V0")["proof"]
    inst.set_values(*_arrays(s.V2(), cc.C32, 32))
    assert not w.products_info()["kept"]
    want = wf.check_sat(fresh2)
    assert want.n_unsat == 3 and want.rows.tolist() == s.broken
    got = w.check_sat(inst)
    assert got.n_unsat == 3 and got.rows.tolist() == s.broken and got.values.tobytes() == want.values.tobytes()
    proof2 = oa.NIZK.prove(fresh2, wf, inputs, gens, LABEL, SEED).bytes
    assert oa.NIZK.prove(inst, w, inputs, gens, LABEL, SEED).bytes == proof2          # the proof forms its own products
    # a mutator does not patch the stale products: the same variables written again
    w.update(inst, 0, s.vars32()[:4])
    assert not w.products_info()["kept"]
    w.keep_products(inst)                                          # recomputed over the new coefficients
    info = w.products_info()
    assert info["kept"] and info["n_unsat"] == 3 and info["full_passes"] == 1 and info["patches"] == 0, info
    again = w.check_sat(inst)                                      # answered from the kept count and bitmap
    assert again.n_unsat == 3 and again.rows.tolist() == s.broken and again.values.tobytes() == want.values.tobytes()
    assert w.products_info()["full_passes"] == 1
    assert oa.NIZK.prove(inst, w, inputs, gens, LABEL, SEED).bytes == proof2
    inst.set_values(*_arrays(s.V0, cc.C32, 32))
    assert not w.products_info()["kept"] and w.check_sat(inst).n_unsat == 0
    assert oa.NIZK.prove(inst, w, inputs, gens, LABEL, SEED).bytes == _fresh(s.name, "V0")["proof"]


# ------------------------------------------------------------------------------------------------ SNARK: the commitment revalued
@pytest.mark.parametrize("route", ["from_coo", "new"])
@pytest.mark.parametrize("name", vc.SNARK_STRUCTURES)
def test_snark_commitment_revalued(name, route):
    s = vc.STRUCTURES[name]
    make = (lambda vals: oa.Instance.from_coo(*s.dims(), *s.coo(vals))) if route == "from_coo" else (lambda vals: oa.Instance.new(*s.dims(), *s.entry_arrays(vals)))
    inst, fresh = make(s.V0), make(s.V1("field"))
    gens = oa.SNARKGens.new(*s.dims(), max(s.nnz()))
    vars_, inputs = _assignment(s)
    comm = oa.ComputationCommitment.encode(inst, gens)
    assert comm.dims[3] == s.snark_n()
    old_bytes = comm.bytes
    old_proof = oa.SNARK.prove(inst, comm, vars_, inputs, gens, LABEL, SEED)
    inst.set_values(*_arrays(s.V1("field"), cc.C32, 32))
    with pytest.raises(oa.SpartanError) as err:
        oa.SNARK.prove(inst, comm, vars_, inputs, gens, LABEL, SEED)
    assert err.value.code == BAD_ARG and "predates the instance's coefficients" in str(err.value), str(err.value)
    assert comm.bytes == old_bytes                                # the refusal changed nothing
    comm.revalue(inst, gens)
    fresh_comm = oa.ComputationCommitment.encode(fresh, gens)
    assert comm.bytes == fresh_comm.bytes and comm.bytes != old_bytes
    if route == "from_coo":
        assert inst.host_lists_info() == {"materialised": False, "host_bytes": 0}             # revalue read the lists in HBM
    proof = oa.SNARK.prove(inst, comm, vars_, inputs, gens, LABEL, SEED)
    assert proof.bytes == oa.SNARK.prove(fresh, fresh_comm, vars_, inputs, gens, LABEL, SEED).bytes
    proof.verify(oa.ComputationCommitment.from_bytes(comm.bytes), inputs, gens, LABEL)
    with pytest.raises(oa.ProofVerifyError):
        old_proof.verify(oa.ComputationCommitment.from_bytes(comm.bytes), inputs, gens, LABEL)            # a proof about the old instance
    with pytest.raises(oa.ProofVerifyError):
        proof.verify(oa.ComputationCommitment.from_bytes(old_bytes), inputs, gens, LABEL)                 # and the new one under the old commitment bytes
    # a commitment parsed from bytes has nothing to revalue; attached to the revalued instance it proves at its generation
    parsed = oa.ComputationCommitment.from_bytes(comm.bytes)
    with pytest.raises(oa.SpartanError) as err:
        parsed.revalue(inst, gens)
    assert err.value.code == BAD_ARG
    parsed.attach(inst, gens)
    assert oa.SNARK.prove(inst, parsed, vars_, inputs, gens, LABEL, SEED).bytes == proof.bytes
    # and back: V1 -> V0 restores the first commitment and proof
    inst.set_values(*_arrays(s.V0, cc.C32, 32))
    comm.revalue(inst, gens)
    assert comm.bytes == old_bytes
    assert oa.SNARK.prove(inst, comm, vars_, inputs, gens, LABEL, SEED).bytes == old_proof.bytes
