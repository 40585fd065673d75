"""What assigning a whole new vector to a resident witness with kept rows costs, by the share of it that changed (profiles/witness_assign.md), and
from which share on summing the touched rows again is no slower than patching them: the figure behind kAssignResumShare (witness.cpp).
For a size of `--lg`, for an int64 (small numbers) and a canonical-bytes (uniform in GF(l)) device source, in ONE process with one instance and one
generator table: two vectors in HBM that differ in k uniformly placed elements (other values of the same distribution), k = 0, 2^-16, 2^-10, 2^-6, 2^-3,
1/2 and 1 of the variables, assigned in turn, alternating inside one loop:

  (a) otti_witness_assign   the patch forced (OTTI_ASSIGN_RESUM_SHARE=2)
  (b) otti_witness_assign   the re-sum of rows idx_min / R .. idx_max / R forced (OTTI_ASSIGN_RESUM_SHARE=0)
  (c) otti_witness_update   over the whole range: what a caller without the list of changes does today; it rewrites every element and sums every row

    python tools/witness_assign_probe.py [--lg 20] [--reps 10] [--warmup 2] [--window C] [--out profiles/witness_assign.md]

Every timing is a host clock around one call that ends synchronised; each call finds the witness holding the other vector, so every timed (a) and (b)
changes exactly k elements.  The two directions are reported apart, and the switch is read off the round trip (median there + median back).  `--window` pins the table's window width (OTTI_MSM_WINDOW)."""
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
SHARES = (("0", 0.0), ("2^-16", 2.0 ** -16), ("2^-10", 2.0 ** -10), ("2^-6", 2.0 ** -6), ("2^-3", 2.0 ** -3), ("1/2", 0.5), ("1", 1.0))


def dev_bytes(a):
    a = np.ascontiguousarray(a)
    d = oa.DeviceArray(a.nbytes, 1)
    assert oa.lib.otti_dev_upload(d.ptr, a.ctypes.data_as(_vp), a.nbytes) == 0
    return d


def fmt(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} - {max(xs):.3f})" if xs else "-"


def pow2_floor(x):
    p = 1.0
    while p > x:
        p /= 2
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=20); ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_assign.md"))
    a = ap.parse_args()
    if a.window:
        os.environ["OTTI_MSM_WINDOW"] = str(a.window)
    if oa.device_count() < 1:
        raise SystemExit("witness_assign_probe: no MI355X visible")
    cmd = f"python tools/witness_assign_probe.py --lg {a.lg} --reps {a.reps} --warmup {a.warmup}" + (f" --window {a.window}" if a.window else "")
    lines = ["# Assigning a whole vector to a resident witness with kept rows", "", f"    {cmd}", "",
             f"Milliseconds, host clock around one call: median (min - max) of {a.reps} calls after {a.warmup} warm-up rounds; (a), (b) and (c) alternate inside one loop.",
             "Two device vectors, `base` and `other`, that differ in k uniformly placed elements (other values of the same distribution) are assigned in turn; the calls",
             "`there` (the witness holds base, other is assigned) and `back` are reported apart: they carry different deltas and need not cost the same.",
             "(a) otti_witness_assign with the patch forced; (b) otti_witness_assign with the re-sum of the touched rows forced; (c) otti_witness_update over the whole",
             f"range (rewrites every element, sums every row: the yardstick for what callers do today, not a candidate; both directions pooled, {2 * a.reps} calls).",
             "All three include the recount of small_fraction.  Round trip: the median there plus the median back, (a) / (b) / (c).", "",
             "| variables | source | window c | changed share | k | rows touched | (a) patch, there | (a) patch, back | (b) re-sum, there | (b) re-sum, back | (c) update | round trip (a) / (b) / (c) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    n = 1 << a.lg
    R = 1 << (a.lg - a.lg // 2)
    r = oa.synth_r1cs(n, 10, 1)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    inputs = oa.InputsAssignment.new(r["inputs"])
    inst.prepare_device(gens)
    trips = {}
    for kind, wfmt in (("int64, small numbers", oa.WIT_I64), ("canonical bytes, uniform", oa.WIT_CANONICAL32)):
        if wfmt == oa.WIT_I64:
            base = rng.integers(-2 ** 40, 2 ** 40, size=n).astype(np.int64)
            wit = oa.Witness.from_ints(inst, base, inputs)
        else:
            base = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
            base[:, 31] &= 0x0f                                 # below 2^252: canonical
            wit = oa.Witness(inst, oa.VarsAssignment.new(base), inputs)
        wit.keep_rows(inst, gens)
        d_base = dev_bytes(base)
        for name, share in SHARES:
            k = int(round(share * n))
            pos = np.sort(rng.choice(n, size=k, replace=False))
            other = base.copy()
            if wfmt == oa.WIT_I64:                               # other small numbers: the deltas are small, and negative (so l - |d|, every window) half the time
                fresh = rng.integers(-2 ** 40, 2 ** 40, size=k).astype(np.int64)
                other[pos] = np.where(fresh == base[pos], fresh + 1, fresh)
            else:                                                # other uniform elements: uniform deltas
                fresh = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
                fresh[:, 31] &= 0x0f
                fresh[:, 0] ^= (fresh == base[pos]).all(axis=1).astype(np.uint8)
                other[pos] = fresh
            d_other = dev_bytes(other)
            times = {how: ([], []) for how in ("2", "0", "update")}   # per way: the calls there (base -> other) and back, kept apart
            for rep in range(a.warmup + a.reps):
                for how in ("2", "0", "update"):
                    for back, d in enumerate((d_other, d_base)):   # there and back: the witness ends every round holding `base`
                        if how != "update":
                            os.environ["OTTI_ASSIGN_RESUM_SHARE"] = how
                        t0 = time.perf_counter()
                        if how == "update":
                            wit.update(inst, 0, (d.ptr.value, n), fmt=wfmt)
                        else:
                            got = wit.assign(inst, (d.ptr.value, n), fmt=wfmt)
                        t1 = time.perf_counter()
                        assert how == "update" or got == k, (got, k)
                        if rep >= a.warmup:
                            times[how][back].append((t1 - t0) * 1e3)
            rows = len(set((pos // R).tolist()))
            trip = {how: statistics.median(t[0]) + statistics.median(t[1]) for how, t in times.items()}   # a round trip by the medians of its halves
            row = (f"| 2^{a.lg} | {kind} | {gens.table_info[0]} | {name} | {k} | {rows} | {fmt(times['2'][0])} | {fmt(times['2'][1])} | {fmt(times['0'][0])} | "
                   f"{fmt(times['0'][1])} | {fmt(times['update'][0] + times['update'][1])} | {trip['2']:.3f} / {trip['0']:.3f} / {trip['update']:.3f} |")
            print(row, flush=True)
            lines.append(row)
            trips.setdefault(kind, []).append((name, share, k, trip))
            del d_other
        del wit, d_base
    os.environ.pop("OTTI_ASSIGN_RESUM_SHARE", None)
    lines += ["", "Per source: the smallest probed share at which the patch's round trip (a) is no longer shorter than the re-sum's (b), that share rounded down to a power",
              "of two, and the probed shares at which the assign — patching below that share, summing again from it on — takes longer than the update (c):", ""]
    for kind, rows_ in trips.items():
        sw = next(((name, share) for name, share, k, t in rows_ if k and t["2"] >= t["0"]), None)
        slower = [name for name, share, k, t in rows_ if t["0" if sw and k and share >= sw[1] else "2"] > t["update"]]
        lines.append(f"* {kind}: " + (f"{sw[0]} -> {pow2_floor(sw[1])}" if sw else "none: the patch is shorter at every probed share")
                     + "; slower than the update at: " + (", ".join(slower) if slower else "no probed share"))
    gens.release_device()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
