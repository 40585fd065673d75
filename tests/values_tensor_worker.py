"""Child process of test_gpu_instance_set_values.py's device-source route.

As a program: imports torch FIRST (torch has to bring the GPU up before libottispartan.so is loaded, so that both use one HIP runtime).  For every
structure of values_cases.py and every coefficient format and stride it builds the instance from V0 (Instance.from_coo, host arrays), computes the
new coefficients as GPU tensors with ordinary tensor operations on a non-default torch stream — strided views where the stride asks for one — and
hands them to Instance.set_values without synchronising: V0 -> V1 under `torch.cuda.stream(s)` with no stream named, then V1 -> V0 with the
stream's handle passed.  Prints one line per case:
    case <structure> <format> <stride> <digest after V1> <digest after V0>
a digest (digest()) being the sha256 of the three entry lists, device_info of both copies, the products, table and evaluations, and the NIZK proof
bytes under a fixed seed, verified.
Importing this module imports neither torch nor anything from the GPU."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
LABEL, SEED = b"instance_set_values", b"\x37" * 32


def scale_for(vc, cc, name, val_format):
    """the V1 of a case: the small scaling where an integer format can carry it (and the codes rule can fire), else uniform scalars"""
    return "small" if val_format in (cc.I64, cc.U64) and "small" in vc.scales(name) else "field"


def points(s):
    """two evaluation points (rx, ry) per structure, as integers"""
    import sparse_cases as sc
    rng = sc._rng("values-points", s.name)
    nrx, nry = s.ncp.bit_length() - 1, (2 * s.nvp).bit_length() - 1
    return [(sc._field(rng, nrx), sc._field(rng, nry)) for _ in range(2)]


def digest(oa, inst, s, gens):
    """sha256 over everything the host-array route compares: the entry lists, device_info of both copies, multiply_vec, eval_table_sparse and
    instance_evaluate on the structure's vectors and points, and the NIZK proof bytes — which the verifier has to accept first"""
    K = oa.kernels
    h = hashlib.sha256()
    for k in range(3):
        h.update(inst.entries(k).tobytes())
    h.update(repr([inst.device_info(by_col=b) for b in (False, True)]).encode())
    sp = s.sparse(s.V0)                                           # (the vectors alone: they do not depend on the coefficients)
    for a in K.multiply_vec(inst, oa.fr_from_ints(sp.z))[:3]:
        h.update(a.tobytes())
    h.update(K.eval_table_sparse(inst, oa.fr_from_ints(sp.eq), oa.fr_from_ints(sp.coef))[0].tobytes())
    pts = points(s)
    rx = oa.fr_from_ints([x for p in pts for x in p[0]]).reshape(len(pts), -1, 32)
    ry = oa.fr_from_ints([x for p in pts for x in p[1]]).reshape(len(pts), -1, 32)
    h.update(K.instance_evaluate(inst, rx, ry)[0].tobytes())
    inputs = oa.InputsAssignment.new(s.inputs32())
    proof = oa.NIZK.prove(inst, oa.VarsAssignment.new(s.vars32()), inputs, gens, LABEL, SEED)
    proof.verify(inst, inputs, gens, LABEL)
    h.update(proof.bytes)
    return h.hexdigest()


def main():
    import torch                                               # before otti_amd: see the module docstring
    assert torch.cuda.is_available(), "torch sees no GPU"
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import otti_amd as oa
    import coo_cases as cc
    import values_cases as vc
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)

    def tensor(xs, val_format, stride):
        """canonical integers -> a GPU tensor in the format at the stride, made by arithmetic on the current stream; (tensor, format used)"""
        arr, used = vc.value_list(val_format, 0, xs)
        if used != val_format:
            stride = 32
        packed = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64 if used in (cc.I64, cc.U64) else np.uint8)).pin_memory().to(dev, non_blocking=True)
        if used in (cc.I64, cc.U64):
            t = (packed + 5) - 5
            if stride == 16:
                t = torch.stack((t, torch.full_like(t, -77)), dim=1).reshape(-1)[::2]
            return (t.view(torch.uint64) if used == cc.U64 else t), used
        wide = torch.full((packed.shape[0], stride), 0xa5, dtype=torch.uint8, device=dev)
        wide[:, :32] = packed ^ 0                              # (passed through an operation: the view below is of memory the stream is still writing)
        return wide[:, :32], used

    for name in sorted(vc.STRUCTURES):
        s = vc.STRUCTURES[name]
        gens = oa.NIZKGens.new(*s.dims())
        for val_format, stride in vc.format_params():
            inst = oa.Instance.from_coo(*s.dims(), *s.coo(s.V0))
            V1 = s.V1(scale_for(vc, cc, name, val_format))
            montgomery = val_format == cc.M32
            with torch.cuda.stream(stream):
                ts = [tensor(xs, val_format, stride) for xs in V1]
                assert [u for _, u in ts] == vc.plan(val_format, V1)
                assert all(t.stride(0) * t.element_size() == stride for t, u in ts if u == val_format and t.shape[0] > 1)
                inst.set_values(*[t if t.shape[0] else None for t, _ in ts], montgomery=montgomery)       # no stream named: torch's current one
            d1 = digest(oa, inst, s, gens)
            with torch.cuda.stream(stream):
                ts = [tensor(xs, val_format, stride) for xs in s.V0]
            inst.set_values(*[t if t.shape[0] else None for t, _ in ts], montgomery=montgomery, stream=stream.cuda_stream)   # outside the block: the stream is named
            d0 = digest(oa, inst, s, gens)
            info = inst.values_info()
            assert info["generation"] == 2 and info["slots_resident"] and info["slot_bytes"] == 8 * sum(s.nnz()), info
            print("case", name, val_format, stride, d1, d0, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
