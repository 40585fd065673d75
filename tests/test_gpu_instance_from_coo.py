"""Instance.from_coo (otti_instance_from_coo, k_coo_ingest.hip) against Instance.new on the same triples: the same instance — dimensions, entries in
caller order, the variants on both CSR copies, products, proof and commitment bytes — and the same refusals.  Everything is exact: bytes and
integers, no tolerance.  The cases and their Python-integer expectations are tests/coo_cases.py's (test_instance_from_coo_host.py holds them
against Instance.new without a GPU).  Nothing here is expected to fault: a thread reads and writes position i < n of arrays of n elements alone,
a refused entry writes nothing, and the strided coefficient load ends at (n - 1) * stride + element size, which is what gets staged."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import otti_amd as oa
import orc
import coo_cases as cc
import sparse_cases as sc

pytestmark = pytest.mark.gpu
K = oa.kernels
L, R = cc.L, cc.R
LABEL, SEED = b"instance_from_coo", b"\x42" * 32
HERE = os.path.dirname(os.path.abspath(__file__))


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def _montgomery_words(xs):
    """canonical integers -> the Montgomery words kernels.from_canonical makes of them, as integers (and they are x * 2^256 mod l)"""
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


def _assert_same_instance(case, got, want, products=True):
    """got (from_coo) is want (Instance.new): dimensions, entries, device_info of both copies, the lists in HBM, multiply_vec"""
    assert got.dims == want.dims == (case.ncp, case.nvp, case.ni), case.name
    info = got.ingest_info()
    per_entry = 2 * np.dtype(cc.INDEX_DTYPE[case.index_format]).itemsize + (8 if case.val_format in (cc.I64, cc.U64) else 32)
    total = sum(len(m) for m in case.triples)
    assert info["on_device"] and info["circuit_bytes"] == per_entry * total and info["hbm_entry_bytes"] == 40 * total and info["ms"][0] == 0, (case.name, info)
    assert got.host_lists_info() == {"materialised": False, "host_bytes": 0}
    for by_col in (False, True):
        assert got.device_info(by_col=by_col) == want.device_info(by_col=by_col), (case.name, by_col)
    for k in range(3):
        exp = case.expected(k)
        pr, pc, pv, n = got.device_entries(k)
        assert n == len(exp), (case.name, k)
        assert want.device_entries(k) == (0, 0, 0, 0)
        if not n:
            assert (pr, pc, pv) == (0, 0, 0)
        assert _download(pr, n, np.uint32).tolist() == [r for r, _, _ in exp], (case.name, k, "rows in HBM")
        assert _download(pc, n, np.uint32).tolist() == [c for _, c, _ in exp], (case.name, k, "padded columns in HBM")
        assert _download(pv, n, np.uint8, 32).tobytes() == b"".join((v * R % L).to_bytes(32, "little") for _, _, v in exp), (case.name, k, "values in HBM")
    assert got.host_lists_info()["materialised"] is False
    for k in range(3):
        a, b = got.entries(k), want.entries(k)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (case.name, "entries", k)
    # (asking for the entries of a matrix without any downloads nothing: an instance without entries never materialises its lists)
    assert got.host_lists_info() == {"materialised": total > 0, "host_bytes": 40 * total}
    if products:
        s = case.sparse()
        z32 = orc.fr_from_ints(s.z)
        ga, gw = K.multiply_vec(got, z32)[:3], K.multiply_vec(want, z32)[:3]
        for k, ints in enumerate(s.multiply_vec()):
            assert ga[k].tobytes() == gw[k].tobytes() == orc.fr_from_ints(ints).tobytes(), (case.name, "multiply_vec", k)


def _both(case, **kw):
    arrays = case.arrays(raw_of=_montgomery_words)
    got = oa.Instance.from_coo(*case.dims(), *arrays, montgomery=case.val_format == cc.M32, **kw)
    return got, oa.Instance.new(*case.dims(), *case.entry_arrays())


# ------------------------------------------------------------------------------------------------ counts: the seams of a 256-thread workgroup
@pytest.mark.parametrize("nA,nB,nC", cc.count_params())
def test_counts_per_matrix(nA, nB, nC):
    case = cc.count_case(nA, nB, nC)
    _assert_same_instance(case, *_both(case))


# ------------------------------------------------------------------------------------------------ every index format x coefficient format x stride
@pytest.mark.parametrize("index_format,val_format,stride", cc.format_params())
def test_formats_and_strides(index_format, val_format, stride):
    case = cc.format_case(index_format, val_format, stride)
    numbers = [x for _, _, x in case.triples[0]]
    assert list(numbers[:len(cc.SPECIALS[val_format])]) == list(cc.SPECIALS[val_format])
    arrays = case.arrays()
    assert all(a[2].strides[0] == stride for a in arrays)
    _assert_same_instance(case, *_both(case))


# ------------------------------------------------------------------------------------------------ padding and the shift of the columns behind the variables
@pytest.mark.parametrize("nv,ni,nc", cc.PADDINGS)
def test_padding_and_shift(nv, ni, nc):
    case = cc.padding_case(nv, ni, nc)
    cols = {c for m in case.triples for _, c, _ in m}
    assert {nv, nv + ni} <= cols and (nv == 0 or nv - 1 in cols)
    assert case.ncp == (2 if nc == 1 else 8)
    _assert_same_instance(case, *_both(case))


# ------------------------------------------------------------------------------------------------ order, duplicates, explicit zeros; the sparse kernels' own cases
def test_order_duplicates_and_zeros_are_kept():
    case = cc.order_case()
    assert sum(1 for t in case.triples[0] if t[:2] == (4, 11)) >= 3 and any(x == 0 for _, _, x in case.triples[0])
    _assert_same_instance(case, *_both(case))


SPARSE = [("ladder", ("lane", 0, "codes")), ("ladder", ("quad", 1, "nocodes")), ("ladder", ("lane", 2, "codes_with_wide", True)),
          ("code_edge", ("lane",)), ("code_edge", ("quad",))] + [("boundary", ("lane",) + b) for b in sc.BOUNDARIES] + [("boundary", ("quad", 1024, 512))]


@pytest.mark.parametrize("kind,args", SPARSE)
def test_sparse_kernel_cases_through_the_new_route(kind, args):
    s = getattr(sc, kind + "_case")(*args)
    case = cc.from_sparse(s)
    got, want = _both(case)
    for by_col, layout in ((False, s.layout), (True, s.layout_col)):
        info = got.device_info(by_col=by_col)
        assert info == want.device_info(by_col=by_col) == s.variant(by_col), (s.name, by_col, info)
        assert info["use_small"] == s.codes and (layout is None or info["quad"] == (layout == "quad")), (s.name, by_col, info)
    z32 = orc.fr_from_ints(s.z)
    out = K.multiply_vec(got, z32)[:3]
    for k, ints in enumerate(s.multiply_vec()):
        assert out[k].tobytes() == orc.fr_from_ints(ints).tobytes(), (s.name, "multiply_vec", k)
    tab, _ = K.eval_table_sparse(got, orc.fr_from_ints(s.eq), orc.fr_from_ints(s.coef))
    assert tab.tobytes() == orc.fr_from_ints(s.eval_table()).tobytes(), (s.name, "eval_table_sparse")
    assert got.host_lists_info()["materialised"] is False
    for k in range(3):
        assert got.entries(k).tobytes() == want.entries(k).tobytes(), (s.name, "entries", k)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name,build,code,msg", cc.error_cases(), ids=[e[0] for e in cc.error_cases()])
def test_refusals_name_what_instance_new_names(name, build, code, msg):
    dims, arrays = build()
    fmts = [cc.C32 if a[2].ndim == 2 else cc.I64 for a in arrays]
    assert cc.sequential_first_error(dims, arrays, fmts) == (code, msg)
    with pytest.raises(oa.R1CSError) as err:
        oa.Instance.from_coo(*dims, *arrays, montgomery=name.startswith("montgomery"))
    assert err.value.code == code and str(err.value).endswith(": " + msg), (name, str(err.value))
    # the context is as usable as before: the next call on this thread gives the whole instance
    case = cc.count_case(257, 1, 256)
    _assert_same_instance(case, *_both(case))


# ------------------------------------------------------------------------------------------------ whole proofs
def _coo_of(r):
    """the entry arrays of oa.synth_r1cs as from_coo takes them: the 32-byte values are read where they are, 48 bytes apart"""
    return [(np.ascontiguousarray(r[m]["row"]), np.ascontiguousarray(r[m]["col"]), r[m]["val"]) for m in "ABC"]


def test_nizk_proof_bytes_and_laziness():
    r = oa.synth_r1cs(64, 3, 1)
    dims = (r["num_cons"], r["num_vars"], r["num_inputs"])
    coo = _coo_of(r)
    assert coo[0][2].strides == (48, 1) and coo[0][0].dtype == np.uint64
    got, want = oa.Instance.from_coo(*dims, *coo), oa.Instance.new(*dims, r["A"], r["B"], r["C"])
    assert got.host_lists_info() == {"materialised": False, "host_bytes": 0}
    gens = oa.NIZKGens.new(*dims)
    vars_, inputs = oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"])
    pg = oa.NIZK.prove(got, vars_, inputs, gens, LABEL, SEED)
    pw = oa.NIZK.prove(want, vars_, inputs, gens, LABEL, SEED)
    assert pg.bytes == pw.bytes
    assert got.host_lists_info() == {"materialised": False, "host_bytes": 0}                 # a proof reads the device copy alone
    assert got.entries(0).tobytes() == r["A"].tobytes()
    assert got.host_lists_info() == {"materialised": True, "host_bytes": 40 * (len(r["A"]) + len(r["B"]) + len(r["C"]))}
    pg.verify(got, inputs, gens, LABEL)
    assert got.is_sat(vars_, inputs)


def test_snark_commitment_bytes_and_a_proof_that_verifies():
    r = oa.synth_r1cs(64, 3, 1)
    dims = (r["num_cons"], r["num_vars"], r["num_inputs"])
    got, want = oa.Instance.from_coo(*dims, *_coo_of(r)), oa.Instance.new(*dims, r["A"], r["B"], r["C"])
    gens = oa.SNARKGens.new(*dims, max(len(r["A"]), len(r["B"]), len(r["C"])))
    cg, cw = oa.ComputationCommitment.encode(got, gens), oa.ComputationCommitment.encode(want, gens)
    assert cg.bytes == cw.bytes
    assert got.host_lists_info() == {"materialised": False, "host_bytes": 0}                 # encode read the lists in HBM
    vars_, inputs = oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"])
    proof = oa.SNARK.prove(got, cg, vars_, inputs, gens, LABEL, SEED)
    assert proof.bytes == oa.SNARK.prove(want, cw, vars_, inputs, gens, LABEL, SEED).bytes
    proof.verify(oa.ComputationCommitment.from_bytes(cw.bytes), inputs, gens, LABEL)


# ------------------------------------------------------------------------------------------------ a device source on a torch stream
def test_device_tensors_on_a_torch_stream_give_the_same_instance():
    """GPU tensors computed on a non-default torch stream and handed over without synchronising — once under `torch.cuda.stream(s)` with no stream
    named, once with the stream's handle passed — give the instance the host arrays give.  A missing ordering between the producer's stream and
    the ingest shows here only by luck: the producer's kernels are short, and nothing forces the ingest to overtake them.  torch has to bring
    the GPU up before the library is loaded, so the work happens in one fresh child process (coo_tensor_worker.py)."""
    import coo_tensor_worker as W
    case = W.tensor_case()
    want_inst = oa.Instance.new(*case.dims(), *case.entry_arrays())
    h = hashlib.sha256()
    for k in range(3):
        h.update(want_inst.entries(k).tobytes())
    want = h.hexdigest() + " " + repr([want_inst.device_info(by_col=b) for b in (False, True)]).replace(" ", "")
    res = subprocess.run([sys.executable, os.path.join(HERE, "coo_tensor_worker.py")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"the child ended with status {res.returncode}:\n{res.stdout}\n{res.stderr}"      # nothing further is started after a fault
    got = dict(ln.split(" ", 2)[1:] for ln in res.stdout.split("\n") if ln.startswith("instance "))
    assert set(got) == {"host_arrays", "current_stream_int64_strided", "named_stream_int32", "default_stream"}, res.stdout + res.stderr
    for name, line in got.items():
        assert line == want, f"{name}: {line} is not {want}"
