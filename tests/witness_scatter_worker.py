"""Child process of test_gpu_witness_scatter.py, and the circuit both share.

As a program: imports torch FIRST (torch has to bring the GPU up before libottispartan.so is loaded, so that both use one HIP runtime), uploads an
int64 assignment, keeps its rows, computes unsorted int64 indices and new int64 values with ordinary tensor operations on a non-default torch
stream and hands both to Witness.scatter without synchronising.  Prints
    digest unsorted_int64 <sha256 of the proof bytes>
or `skip <reason>` (exit status 0) when torch sees no GPU.  Importing this module imports neither torch nor anything from the GPU."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2 ** 252 + 27742317777372353535851937790883648493
N, NI, K, LABEL, SEED = 1 << 10, 2, 96, b"witness_scatter", b"\x37" * 32


def bytes32(xs):
    return np.array([np.frombuffer((int(x) % L).to_bytes(32, "little"), dtype=np.uint8) for x in xs], dtype=np.uint8).reshape(-1, 32)


def start_values(n=N):
    k = np.arange(n, dtype=np.int64)
    return (k * 7919 + 13) % 1000003 - 500000


def scatter_lists(n=N, count=K):
    """what the child computes on the GPU, as numpy int64: `count` distinct indices below n in no order, and their new values (mixed signs)"""
    k = np.arange(count, dtype=np.int64)
    idx = (k * 389 + 17) % n                                   # 389 is odd: distinct while count <= n
    new = (k * 40009 + 3) % 2000003 - 1000001
    return idx, new


def scatter_case():
    """a circuit every assignment satisfies (row i: (k_i * v_i) * 1 = k_i * v_i), in the dict shape of oa.synth_r1cs, and the scatter lists"""
    import otti_amd as oa
    coef = [3 + 2 * i for i in range(N)]
    A, B = np.zeros(N, dtype=oa.ENTRY_DTYPE), np.zeros(N, dtype=oa.ENTRY_DTYPE)
    A["row"] = B["row"] = np.arange(N)
    A["col"] = np.arange(N); A["val"] = bytes32(coef)
    B["col"] = N; B["val"] = bytes32([1] * N)
    r = dict(num_cons=N, num_vars=N, num_inputs=NI, A=A, B=B, C=A, inputs=bytes32([5, 6][:NI]))
    idx, new = scatter_lists()
    return r, idx, new


def main():
    import torch                                               # before otti_amd: see the module docstring
    if not torch.cuda.is_available():
        print("skip torch.cuda.is_available() is false")
        return 0
    sys.path.insert(0, ROOT)
    import otti_amd as oa
    r, _, _ = scatter_case()
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    inputs = oa.InputsAssignment.new(r["inputs"])
    wit = oa.Witness.from_ints(inst, start_values(), inputs)
    wit.keep_rows(inst, gens)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        k = torch.arange(K, dtype=torch.int64, device=dev)
        idx = (k * 389 + 17) % N
        new = (k * 40009 + 3) % 2000003 - 1000001
        wit.scatter(inst, idx, new)                            # no synchronisation in between: the library's stream waits on the device
    assert wit.scatter_info()[0] == 1 and wit.scatter_info()[2] == K and wit.rows_info()[3] == 0
    p = oa.NIZK.prove(inst, wit, None, gens, LABEL, SEED)
    print("digest unsorted_int64", hashlib.sha256(p.bytes).hexdigest())
    return 0


if __name__ == "__main__":
    sys.exit(main())
