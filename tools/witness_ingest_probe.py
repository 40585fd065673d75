"""How long a resident witness takes to fill, by source (profiles/witness_ingest.md): wall time of the whole call, the witness freed between
calls, median / min / max of `--reps` after `--warmup`, for each size of `--lg`:

  otti_witness_upload                       32-byte canonical scalars from host memory (the comparison: PCIe-bound)
  otti_witness_upload_ints                  int64 from host memory (8 bytes per variable over PCIe)
  otti_witness_from_device I64              int64 already in HBM
  otti_witness_from_device CANONICAL32      canonical scalars already in HBM
  otti_witness_update 1 %                   int64 from HBM into the middle of a resident witness (includes the recount of small_fraction)

    python tools/witness_ingest_probe.py [--lg 20 24] [--reps 10] [--warmup 2] [--out profiles/witness_ingest.md]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import otti_amd as oa  # noqa: E402

_vp = ctypes.c_void_p


def dev_bytes(a):
    d = oa.DeviceArray(a.nbytes, 1)
    assert oa.lib.otti_dev_upload(d.ptr, a.ctypes.data_as(_vp), a.nbytes) == 0
    return d


def wall_ms(f, warmup, reps):
    out = []
    for k in range(warmup + reps):
        t0 = time.perf_counter(); w = f(); dt = (time.perf_counter() - t0) * 1e3
        del w
        if k >= warmup:
            out.append(dt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, nargs="+", default=[20, 24]); ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_ingest.md"))
    a = ap.parse_args()
    if oa.device_count() < 1:
        raise SystemExit("witness_ingest_probe: no MI355X visible")
    rng = np.random.default_rng(1)
    lines = ["# Filling a resident witness, by source", "", f"    python tools/witness_ingest_probe.py --lg {' '.join(str(k) for k in a.lg)} --reps {a.reps} --warmup {a.warmup}", "",
             f"Wall time of the whole call in ms (median, min - max of {a.reps} after {a.warmup} warm-up calls; the witness is freed between calls, so every",
             "call allocates and zeroes z as well).  Values: 90 % non-negative integers below 2^63, 10 % negative.  The host upload of the same size in the",
             "same run is the comparison.", "",
             "| variables | otti_witness_upload (host, 32 B) | otti_witness_upload_ints (host, 8 B) | from_device I64 | from_device CANONICAL32 | update 1 % (I64, device) |",
             "|---|---|---|---|---|---|"]
    for lg in a.lg:
        n = 1 << lg
        e = np.zeros(2, dtype=oa.ENTRY_DTYPE); e["row"] = [0, 1]; e["col"] = [0, n]; e["val"][:, 0] = 1
        inst = oa.Instance.new(2, n, 0, e, e, e)                # z does not depend on the matrices
        inputs = oa.InputsAssignment.new(np.zeros((0, 32), dtype=np.uint8))
        x = rng.integers(0, 2 ** 63 - 1, size=n, dtype=np.int64)
        neg = rng.random(n) < 0.1
        x[neg] = -x[neg] - 1
        canon = np.zeros((n, 32), dtype=np.uint8)
        canon[:, :8] = np.where(neg, 0, x).astype("<i8").view(np.uint8).reshape(n, 8)
        lneg = oa.L_ORDER - 1                                    # (a negative x is l - |x|; for the host upload any large canonical value costs the same)
        canon[neg] = np.frombuffer(lneg.to_bytes(32, "little"), dtype=np.uint8)
        v = oa.VarsAssignment(canon)
        d_x, d_canon = dev_bytes(x), dev_bytes(canon)
        cols = [wall_ms(lambda: oa.Witness(inst, v, inputs), a.warmup, a.reps),
                wall_ms(lambda: oa.Witness.from_ints(inst, x, inputs), a.warmup, a.reps),
                wall_ms(lambda: oa.Witness.from_device(inst, d_x, n, oa.WIT_I64, inputs), a.warmup, a.reps),
                wall_ms(lambda: oa.Witness.from_device(inst, d_canon, n, oa.WIT_CANONICAL32, inputs), a.warmup, a.reps)]
        wit = oa.Witness.from_device(inst, d_x, n, oa.WIT_I64, inputs)
        count, first = max(1, n // 100), n // 3
        cols.append(wall_ms(lambda: wit.update(inst, first, (d_x.ptr.value + 8 * first, count), fmt=oa.WIT_I64), a.warmup, a.reps))
        row = f"| 2^{lg} | " + " | ".join(f"{statistics.median(c):.3f} ({min(c):.3f} - {max(c):.3f})" for c in cols) + " |"
        print(row, flush=True)
        lines.append(row)
        del wit, d_x, d_canon, inst
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
