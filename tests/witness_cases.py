"""Shared by the GPU tests of the resident witness (test_gpu_witness_device.py, test_gpu_witness_rows.py, test_gpu_witness_scatter.py): the circuit
that every assignment satisfies with its two provers, value generators, raw device memory, the launch counter and the read-back of z.  A plain
module like sparse_cases.py; nothing here is collected.  The worker scripts keep a bytes32 of their own: they run as separate processes."""
import ctypes

import numpy as np

import otti_amd as oa
import orc

Q = orc.L_ORDER
SEED = b"\x2a" * 32
_vp = ctypes.c_void_p


def bytes32(xs):
    return np.array([np.frombuffer((int(x) % Q).to_bytes(32, "little"), dtype=np.uint8) for x in xs], dtype=np.uint8).reshape(-1, 32)


class Case:
    """row i: (k_i * v_i) * 1 = k_i * v_i — satisfied by EVERY assignment, while Az and Cz still depend on every variable"""

    def __init__(self, ell, ni=2):
        nv = self.V = 1 << ell
        self.L, self.R = 1 << (ell // 2), 1 << (ell - ell // 2)
        k = [3 + 2 * i for i in range(nv)]
        A, B = np.zeros(nv, dtype=oa.ENTRY_DTYPE), np.zeros(nv, dtype=oa.ENTRY_DTYPE)
        A["row"] = B["row"] = np.arange(nv)
        A["col"] = np.arange(nv); A["val"] = bytes32(k)
        B["col"] = nv; B["val"] = bytes32([1] * nv)              # column num_vars is the constant 1
        self.args = (nv, nv, ni, A, B, A)
        self.inputs32 = bytes32([11, Q - 3][:ni])
        self.inst, self.gens = oa.Instance.new(*self.args), oa.NIZKGens.new(nv, nv, ni)
        self.oinst, self.ogens = orc.OInstance(*self.args), orc.OGens(nv, nv, ni)
        self.inputs = oa.InputsAssignment.new(self.inputs32)

    def want(self, cur, label, seed=SEED, inputs32=None):
        return orc.nizk_prove(self.oinst, bytes32(cur), self.inputs32 if inputs32 is None else inputs32, self.ogens, label, seed)[0]

    def check(self, wit, cur, label, seed=SEED, inputs32=None):
        got = oa.NIZK.prove(self.inst, wit, None, self.gens, label, seed).bytes
        assert got == self.want(cur, label, seed, inputs32), f"2^{self.V.bit_length() - 1} {label!r}: the proof differs from the oracle's"

    def host_witness(self, cur):
        return oa.Witness(self.inst, oa.VarsAssignment.new(bytes32(cur)), self.inputs)


_cases = {}


def case(ell):
    if ell not in _cases:
        _cases[ell] = Case(ell)
    return _cases[ell]


def values(rng, n, kind="mixed"):
    """n scalars: `mixed` straddles 2^128 (the small_fraction rule) and carries the ends of the range; `small` is what a compiler emits;
    `large` is uniform in GF(l)"""
    if kind == "small":
        return [int(x) for x in rng.integers(0, 1 << 40, size=n)]
    if kind == "large":
        return [int.from_bytes(rng.bytes(40), "little") % Q for _ in range(n)]
    out = [int.from_bytes(rng.bytes(40), "little") % Q >> int(s) for s in rng.choice([0, 100, 124, 125, 200], size=n)]
    out[:6] = [0, 1, 2 ** 128 - 1, 2 ** 128, Q - 1, 2 ** 64][:n]
    return out


class Dev:
    """raw bytes in device memory"""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.arr = oa.DeviceArray(max(a.nbytes, 8), 1)
        if a.nbytes:
            assert oa.lib.otti_dev_upload(self.arr.ptr, a.ctypes.data_as(_vp), a.nbytes) == 0
        self.addr = self.arr.ptr.value


def msm_launches(fn):
    """fixed-base MSM launches (both kernel classes) the calling thread makes inside fn()"""
    oa.stats_enable(True)
    try:
        fn()
        s = oa.stats_read()
    finally:
        oa.stats_enable(False)
    print("launches:", {k: v[0] for k, v in s.items() if v[0]})
    return s["msm_rows"][0] + s["msm_small"][0]


def z_of(wit):
    """(z as (n, 32) uint8 Montgomery words, small_fraction) of a resident witness"""
    p, n, sf = wit.info
    out = np.zeros((n, 32), dtype=np.uint8)
    assert oa.lib.otti_dev_download(out.ctypes.data_as(_vp), p, out.nbytes) == 0
    return out, sf
