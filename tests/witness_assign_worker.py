"""Child process of test_gpu_witness_assign.py; the circuit and start values are witness_scatter_worker's.

As a program: imports torch FIRST (torch has to bring the GPU up before libottispartan.so is loaded, so that both use one HIP runtime), uploads an
int64 assignment, keeps its rows, computes the whole next assignment with ordinary tensor operations on a non-default torch stream — most elements
as they were, every 11th moved — and hands the tensor to Witness.assign without synchronising.  Prints
    digest int64_tensor <sha256 of the proof bytes>
    digest changed <the number assign returned>
or `skip <reason>` (exit status 0) when torch sees no GPU, which the parent reports as a failure.  Importing this module imports neither torch nor anything from the GPU."""
import hashlib
import sys

import numpy as np

import witness_scatter_worker as S

N, LABEL, SEED = S.N, b"witness_assign", b"\x39" * 32


def next_values(start):
    """what the child computes on the GPU, as numpy int64: every 11th element moved (by a multiple of 1000003 among them: by nothing mod that, but
    the VALUE moves), the others as they were"""
    k = np.arange(start.shape[0], dtype=np.int64)
    return np.where(k % 11 == 3, start * 3 - 1000003 * (k % 5), start)


def assign_case():
    """(the circuit in the dict shape of oa.synth_r1cs, the next assignment as numpy int64, how many elements it moves)"""
    r, _, _ = S.scatter_case()
    start = S.start_values()
    new = next_values(start)
    return r, new, int((new != start).sum())


def main():
    import torch                                               # before otti_amd: see the module docstring
    if not torch.cuda.is_available():
        print("skip torch.cuda.is_available() is false")
        return 0
    sys.path.insert(0, S.ROOT)
    import otti_amd as oa
    r, _, _ = S.scatter_case()
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    inputs = oa.InputsAssignment.new(r["inputs"])
    wit = oa.Witness.from_ints(inst, S.start_values(), inputs)
    wit.keep_rows(inst, gens)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        k = torch.arange(N, dtype=torch.int64, device=dev)
        start = (k * 7919 + 13) % 1000003 - 500000
        new = torch.where(k % 11 == 3, start * 3 - 1000003 * (k % 5), start)
        n = wit.assign(inst, new)                              # no synchronisation in between: the library's stream waits on the device
    assert wit.assign_info()[:2] == (1, n) and wit.scatter_info()[0] == 0
    p = oa.NIZK.prove(inst, wit, None, gens, LABEL, SEED)
    print("digest int64_tensor", hashlib.sha256(p.bytes).hexdigest())
    print("digest changed", n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
