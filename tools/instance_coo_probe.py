"""How long arrays take to become a ready, device-prepared instance, by route (profiles/instance_from_coo.md): wall time of the whole call, the
instance freed between calls, median / min / max of `--reps` after `--warmup`, for the uniform and the compiler-like synthetic circuit at each
size of `--lg`:

  Instance.new + prepare_device        otti_entry arrays (48 bytes per entry) validated and converted on the host, uploaded, CSR build
  from_coo host I64                    int64 rows / cols / coefficients in host memory (24 bytes per entry), staged as they are; a matrix whose
                                       coefficients do not fit 64 bits (the synthetic circuits' C) goes as CANONICAL32, and the table says which
  from_coo host CANONICAL32            int64 rows / cols and 32-byte canonical coefficients in host memory (48 bytes per entry)
  from_coo device I64                  the arrays of the I64 route already in HBM

and, for the last route, the kernel lap of otti_instance_ingest_info with the bandwidth it stands for: (bytes read + 40 bytes written per entry)
over that lap.  The lap is host time around the three launches and their synchronise, so at small sizes it is launch latency, not bandwidth.

    python tools/instance_coo_probe.py [--lg 16 20] [--reps 7] [--warmup 2] [--out profiles/instance_from_coo.md]
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
L = oa.L_ORDER


def dev_bytes(a, each=8):
    a = np.ascontiguousarray(a)
    d = oa.DeviceArray(max(1, a.nbytes // each), each)
    d.nbytes_each = each
    if a.nbytes:
        assert oa.lib.otti_dev_upload(d.ptr, a.ctypes.data_as(_vp), a.nbytes) == 0
    return d


def wall_ms(f, warmup, reps):
    out, last = [], None
    for k in range(warmup + reps):
        t0 = time.perf_counter(); inst = f(); dt = (time.perf_counter() - t0) * 1e3
        last = inst.ingest_info()
        del inst
        if k >= warmup:
            out.append(dt)
    return out, last


def as_int64(vals32):
    """(n, 32) canonical bytes -> int64 numbers x with x mod l equal to them (small magnitudes either sign), or None when one does not fit"""
    words = np.ascontiguousarray(vals32).view("<u8").reshape(-1, 4)
    pos = (words[:, 1:] == 0).all(axis=1) & (words[:, 0] < 2 ** 63)
    lw = np.array([(L >> (64 * k)) & (2 ** 64 - 1) for k in range(4)], dtype=np.uint64)
    neg = (words[:, 1:] == lw[1:]).all(axis=1) & (words[:, 0] < lw[0]) & (lw[0] - words[:, 0] <= np.uint64(2 ** 63)) & ~pos
    if not (pos | neg).all():
        return None
    out = words[:, 0].astype(np.int64)
    out[neg] = -(lw[0] - words[neg, 0]).astype(np.int64)
    return out


def device_call(dims, mats):
    """otti_instance_from_coo over arrays in HBM (no torch in this process: the C ABI is called with DeviceArray addresses)"""
    coo = (oa.api._Coo * 3)()
    for k, (r, c, v, n) in enumerate(mats):
        coo[k] = oa.api._Coo(r.ptr, c.ptr, v.ptr, n, oa.IDX_I64, oa.WIT_I64 if v.nbytes_each == 8 else oa.WIT_CANONICAL32, 0)
    h = _vp()
    oa.api._check(oa.lib.otti_instance_from_coo(*dims, coo, 1, None, ctypes.byref(h)))
    return oa.Instance(h, None)


def fmt(c):
    return f"{statistics.median(c):.2f} ({min(c):.2f} - {max(c):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, nargs="+", default=[16, 20]); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_from_coo.md"))
    a = ap.parse_args()
    if oa.device_count() < 1:
        raise SystemExit("instance_coo_probe: no MI355X visible")
    oa.Instance.new(2, 2, 0, *[np.zeros(0, dtype=oa.ENTRY_DTYPE)] * 3).prepare_device()       # the runtime and this thread's context are up before anything is timed
    lines = ["# Arrays to a ready instance, by route", "", f"    python tools/instance_coo_probe.py --lg {' '.join(str(k) for k in a.lg)} --reps {a.reps} --warmup {a.warmup}", "",
             f"Wall time of the whole call in ms (median, min - max of {a.reps} after {a.warmup} warm-up calls; the instance is freed between calls).  Every route ends",
             "with both CSR copies in HBM.  kernel: the device route's kernel lap (host time around the three launches and their synchronise) and",
             "(bytes read + 40 bytes written per entry) over it.", "",
             "| circuit | entries | Instance.new + prepare_device | from_coo host I64 | from_coo host CANONICAL32 | from_coo device I64 | kernel ms | kernel GB/s |",
             "|---|---|---|---|---|---|---|---|"]
    for lg in a.lg:
        for name, synth in (("uniform", oa.synth_r1cs), ("compiler-like", oa.synth_r1cs_compiler_like)):
            r = synth(1 << lg, 10, 1)
            dims = (r["num_cons"], r["num_vars"], r["num_inputs"])
            ents = [r[m] for m in "ABC"]
            total = sum(len(e) for e in ents)
            idx = [(np.ascontiguousarray(e["row"]).astype(np.int64), np.ascontiguousarray(e["col"]).astype(np.int64)) for e in ents]
            canon = [np.ascontiguousarray(e["val"]) for e in ents]
            ints = [as_int64(v) for v in canon]

            def host_new():
                inst = oa.Instance.new(*dims, *ents)
                inst.prepare_device()
                return inst
            mixed = [v if x is None else x for x, v in zip(ints, canon)]     # int64 where a matrix's coefficients fit, canonical bytes where not
            note = "".join("ABC"[k] for k, x in enumerate(ints) if x is None)
            note = f" ({note}: CANONICAL32)" if note else ""
            cols = [fmt(wall_ms(host_new, a.warmup, a.reps)[0]),
                    fmt(wall_ms(lambda: oa.Instance.from_coo(*dims, *[(i[0], i[1], x) for i, x in zip(idx, mixed)]), a.warmup, a.reps)[0]) + note,
                    fmt(wall_ms(lambda: oa.Instance.from_coo(*dims, *[(i[0], i[1], v) for i, v in zip(idx, canon)]), a.warmup, a.reps)[0])]
            dev = [(dev_bytes(i[0]), dev_bytes(i[1]), dev_bytes(x, 8 if x.ndim == 1 else 32), len(x)) for i, x in zip(idx, mixed)]
            t, info = wall_ms(lambda: device_call(dims, dev), a.warmup, a.reps)
            cols.append(fmt(t) + note)
            kernel = (f"{info['ms'][2]:.3f}", f"{(info['circuit_bytes'] + 40 * total) / (info['ms'][2] * 1e-3) / 1e9:.0f}")
            del dev
            row = f"| {name} 2^{lg} | {total} | " + " | ".join(cols) + f" | {kernel[0]} | {kernel[1]} |"
            print(row, flush=True)
            lines.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
