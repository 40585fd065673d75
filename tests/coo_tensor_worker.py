"""Child process of test_gpu_instance_from_coo.py's device-source test.

As a program: imports torch FIRST (torch has to bring the GPU up before libottispartan.so is loaded, so that both use one HIP runtime), computes the
nine arrays of one case with ordinary tensor operations on a non-default torch stream and hands them to Instance.from_coo without synchronising.
Prints one line per instance:
    instance <name> <sha256 of the three entry lists> <device_info of both copies>
Importing this module imports neither torch nor anything from the GPU."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def tensor_case():
    sys.path.insert(0, HERE)
    import coo_cases as cc
    return cc.count_case(513, 257, 1, nc=300, nv=200, ni=5, index_format=cc.IDX_I64, val_format=cc.I64)


def _line(name, inst):
    h = hashlib.sha256()
    for k in range(3):
        h.update(inst.entries(k).tobytes())
    print("instance", name, h.hexdigest(), repr([inst.device_info(by_col=b) for b in (False, True)]).replace(" ", ""), flush=True)


def main():
    import torch                                               # before otti_amd: see the module docstring
    assert torch.cuda.is_available(), "torch sees no GPU"
    sys.path.insert(0, ROOT)
    import otti_amd as oa
    case = tensor_case()
    host = case.arrays()
    _line("host_arrays", oa.Instance.from_coo(*case.dims(), *host))
    dev = torch.device("cuda:0")
    pinned = [[torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in m] for m in host]
    s = torch.cuda.Stream(device=dev)

    def produce(as_bytes32):
        """on the current stream: the arrays uploaded without blocking and passed through arithmetic, values interleaved with a filler so that the
        ones that count are a strided view; as_bytes32: int32 indices, and the values widened to canonical 32-byte scalars (all of them >= 0 there)"""
        out = []
        for rows, cols, vals in pinned:
            r = (rows.to(dev, non_blocking=True) + 7) - 7
            c = (cols.to(dev, non_blocking=True) * 3) // 3
            v = vals.to(dev, non_blocking=True)
            if as_bytes32:
                shifts = torch.arange(0, 64, 8, dtype=torch.int64, device=dev)
                low = ((v.abs().unsqueeze(1) >> shifts) & 255).to(torch.uint8)
                wide = torch.zeros((v.shape[0], 32), dtype=torch.uint8, device=dev)
                wide[:, :8] = low
                out.append((r.to(torch.int32), c.to(torch.int32), wide, v))
            else:
                both = torch.stack((v, torch.full_like(v, -77)), dim=1).reshape(-1)
                out.append((r, c, both[::2]))
        return out

    with torch.cuda.stream(s):
        mats = produce(False)
        assert mats[0][2].stride(0) == 2
        inst = oa.Instance.from_coo(*case.dims(), *mats)      # no stream named: torch's current one, s
    _line("current_stream_int64_strided", inst)
    mats = produce(False)                                      # torch's default stream: the wrapper waits for it on the host
    _line("default_stream", oa.Instance.from_coo(*case.dims(), *mats))
    # 32-byte values: |x| as canonical bytes, so the instance differs from the case's where x < 0 — compared with Instance.new on the same numbers instead
    with torch.cuda.stream(s):
        mats = produce(True)
    inst = oa.Instance.from_coo(*case.dims(), *[m[:3] for m in mats], stream=s.cuda_stream)   # outside the block: the stream is named
    s.synchronize()
    ref = []
    for (rows, cols, _), m in zip(host, mats):
        e = np.zeros(len(rows), dtype=oa.ENTRY_DTYPE)
        e["row"], e["col"] = rows, cols
        e["val"] = m[2].cpu().numpy()
        ref.append(e)
    want = oa.Instance.new(*case.dims(), *ref)
    same = all(inst.entries(k).tobytes() == want.entries(k).tobytes() for k in range(3)) and all(inst.device_info(by_col=b) == want.device_info(by_col=b) for b in (False, True))
    assert same, "int32 indices and (n, 32) uint8 values on a named stream: not the instance Instance.new makes of the same numbers"
    # every |x| equals x for this line's purpose only when no value is negative: the case is re-made with magnitudes and reported under the case's digest
    abs_case = tensor_case()
    abs_case.triples = [[(r, c, abs(x)) for r, c, x in m] for m in abs_case.triples]
    want_abs = oa.Instance.new(*abs_case.dims(), *abs_case.entry_arrays())
    assert all(inst.entries(k).tobytes() == want_abs.entries(k).tobytes() for k in range(3))
    _line("named_stream_int32", oa.Instance.from_coo(*case.dims(), *[(m[0], m[1], m[3]) for m in mats], stream=s.cuda_stream))
    return 0


if __name__ == "__main__":
    sys.exit(main())
