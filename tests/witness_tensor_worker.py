"""Child process of test_gpu_witness_tensor.py, and the small integer-witness circuits the witness tests share.

As a program: imports torch FIRST (torch has to bring the GPU up before libottispartan.so is loaded, so that both use one HIP runtime), computes
an int64 assignment with ordinary tensor operations, once on torch's default stream and once on a non-default one, and hands a strided view of
it to Witness.from_tensor without synchronising — under `torch.cuda.stream(s)` also a packed copy and the same values as an (n, 32) uint8 tensor.  Prints one line per proof:
    digest <name> <sha256 of the proof bytes>
or `skip <reason>` (exit status 0) when torch sees no GPU.  Importing this module imports neither torch nor anything from the GPU."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2 ** 252 + 27742317777372353535851937790883648493
N, NI, LABEL, SEED = 1 << 10, 3, b"witness_tensor", b"\x37" * 32


def bytes32(xs):
    return np.array([np.frombuffer((int(x) % L).to_bytes(32, "little"), dtype=np.uint8) for x in xs], dtype=np.uint8).reshape(-1, 32)


def tensor_values(n=N):
    """what the child computes on the GPU, as numpy int64: 2 n values, mixed signs, none zero; the witness is every second one"""
    k = np.arange(2 * n, dtype=np.int64)
    t = (k * 7919 + 13) % 1000003 - 500000
    t = t * 40009 + (k % 5)
    return np.where(t == 0, 1, t)


def int_r1cs(var_ints, input_ints, seed=3):
    """A satisfiable R1CS over the given integer assignment (every value non-zero mod l): row i reads variable i in A, a random entry of z in B
    and one in C, whose coefficient is solved for.  Returns the dict shape of oa.synth_r1cs plus `rows`: (a, b, c, coef) per row."""
    import otti_amd as oa
    n, ni = len(var_ints), len(input_ints)
    z = [int(x) % L for x in var_ints] + [1] + [int(x) % L for x in input_ints]
    assert all(z), "a zero in the assignment"
    rng = np.random.default_rng(seed)
    b, c = rng.integers(0, n + 1 + ni, size=n), rng.integers(0, n + 1 + ni, size=n)
    rows = [(i, int(b[i]), int(c[i]), z[i] * z[int(b[i])] * pow(z[int(c[i])], -1, L) % L) for i in range(n)]
    mats = []
    for cols, vals in (([r[0] for r in rows], [1] * n), ([r[1] for r in rows], [1] * n), ([r[2] for r in rows], [r[3] for r in rows])):
        e = np.zeros(n, dtype=oa.ENTRY_DTYPE)
        e["row"] = np.arange(n); e["col"] = cols; e["val"] = bytes32(vals)
        mats.append(e)
    return dict(num_cons=n, num_vars=n, num_inputs=ni, A=mats[0], B=mats[1], C=mats[2], vars=bytes32(var_ints), inputs=bytes32(input_ints), rows=rows)


def tensor_case():
    return int_r1cs(tensor_values()[::2], [5, 6, 7][:NI])


def main():
    import torch                                               # before otti_amd: see the module docstring
    if not torch.cuda.is_available():
        print("skip torch.cuda.is_available() is false")
        return 0
    sys.path.insert(0, ROOT)
    import otti_amd as oa
    r = tensor_case()
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    inputs = oa.InputsAssignment.new(r["inputs"])
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    canon = torch.from_numpy(np.ascontiguousarray(r["vars"])).to(dev)          # (n, 32) uint8, on the default stream
    torch.cuda.current_stream(dev).synchronize()

    def compute():
        k = torch.arange(2 * N, dtype=torch.int64, device=dev)
        t = (k * 7919 + 13) % 1000003 - 500000
        t = t * 40009 + (k % 5)
        return torch.where(t == 0, torch.ones_like(t), t)

    # on torch's default stream (HIP's null stream, which cannot be named to the library: from_tensor waits for it on the host)
    assert torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev)
    w_default = oa.Witness.from_tensor(inst, compute()[::2], inputs)
    with torch.cuda.stream(s):
        t = compute()
        view = t[::2]
        assert view.stride(0) == 2 and not view.is_contiguous()
        w_view = oa.Witness.from_tensor(inst, view, inputs)                   # no synchronisation in between: the ingest waits on the device
        w_packed = oa.Witness.from_tensor(inst, view.contiguous(), inputs)
        w_canon = oa.Witness.from_tensor(inst, canon, inputs)
    for name, w in (("default_stream_int64", w_default), ("strided_int64", w_view), ("packed_int64", w_packed), ("canonical_uint8", w_canon)):
        assert w.check_sat(inst).n_unsat == 0, name
        p = oa.NIZK.prove(inst, w, None, gens, LABEL, SEED)
        print("digest", name, hashlib.sha256(p.bytes).hexdigest())
    return 0


if __name__ == "__main__":
    sys.exit(main())
