"""What keeping a resident witness's row sums buys and costs (profiles/witness_rows.md).  For each size of `--lg`, uniform and compiler-like
witness, in ONE process with one instance and one generator table:

  otti_nizk_prove_resident     stage_ms[0] (polycommit) and the total, rows not kept and rows kept (median, min - max of `--reps` after `--warmup`)
  otti_witness_keep_rows       wall time of the call on a witness without kept rows (the table is resident already)
  otti_witness_update          wall time of an update of 1, R and 16 R variables (int64 from HBM) with rows kept, and of the same updates without

    python tools/witness_rows_probe.py [--lg 20] [--reps 10] [--warmup 2] [--window C] [--out profiles/witness_rows.md]

`--window` pins the table's window width (OTTI_MSM_WINDOW); without it the library takes the widest that fits its budget, as bench.py does.
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


def fmt(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} - {max(xs):.3f})"


def prove_ms(inst, wit, gens, warmup, reps):
    """(polycommit, total) per timed proof; every proof has its own label and seed"""
    pc, tot = [], []
    for k in range(warmup + reps):
        p = oa.NIZK.prove(inst, wit, None, gens, b"rows probe %d" % k, bytes([k + 1]) * 32)
        if k >= warmup:
            pc.append(p.stage_ms["polycommit"]); tot.append(p.stage_ms["total"])
    return pc, tot


def wall_ms(f, warmup, reps):
    out = []
    for k in range(warmup + reps):
        t0 = time.perf_counter(); f(); dt = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            out.append(dt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, nargs="+", default=[20]); ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_rows.md"))
    a = ap.parse_args()
    if a.window:
        os.environ["OTTI_MSM_WINDOW"] = str(a.window)
    if oa.device_count() < 1:
        raise SystemExit("witness_rows_probe: no MI355X visible")
    cmd = f"python tools/witness_rows_probe.py --lg {' '.join(str(k) for k in a.lg)} --reps {a.reps} --warmup {a.warmup}" + (f" --window {a.window}" if a.window else "")
    lines = ["# A resident witness that keeps its row sums", "", f"    {cmd}", "",
             f"Milliseconds: median (min - max) of {a.reps} after {a.warmup} warm-up calls.  Proof columns are otti_nizk_prove_resident's own stage_ms[0] (polycommit)",
             "and total, from one process, one instance and one window table, first from a witness that keeps no rows, then from an identical one that",
             "does.  keep_rows and update are wall times of the whole call (update: int64 values already in HBM; it includes the recount of",
             "small_fraction, and with rows kept the re-sum of the rows it touches: 1, 1 and 16 of them).", "",
             "| variables | witness | window c | polycommit, not kept | polycommit, kept | total, not kept | total, kept | keep_rows | update 1 / R / 16 R, kept | update 1 / R / 16 R, not kept |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    for lg in a.lg:
        n = 1 << lg
        R = 1 << (lg - lg // 2)
        gens = None
        for kind, synth in (("uniform", oa.synth_r1cs), ("compiler-like", oa.synth_r1cs_compiler_like)):
            r = synth(n, 10, 1)
            inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
            if gens is None:
                gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])     # both witnesses of a size share the generators and their table
            v, inputs = oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"])
            plain, kept = oa.Witness(inst, v, inputs), oa.Witness(inst, v, inputs)
            inst.prepare_device(gens)
            pc0, tot0 = prove_ms(inst, plain, gens, a.warmup, a.reps)

            def timed_keep():
                out = []
                for k in range(a.warmup + a.reps):
                    w = oa.Witness(inst, v, inputs)
                    t0 = time.perf_counter(); w.keep_rows(inst, gens); dt = (time.perf_counter() - t0) * 1e3
                    if k >= a.warmup:
                        out.append(dt)
                return out
            keep = timed_keep()
            kept.keep_rows(inst, gens)
            pc1, tot1 = prove_ms(inst, kept, gens, a.warmup, a.reps)
            # updates that change nothing of value: small non-negative integers over a range of the middle (a compiler's witness stays one)
            x = rng.integers(0, 1 << 40, size=16 * R, dtype=np.int64)
            d_x = dev_bytes(x)
            first = (n // 3 // R) * R                                # row-aligned: R variables are one row, 16 R sixteen
            ups = [[wall_ms(lambda c=count: w.update(inst, first, (d_x.ptr.value, c), fmt=oa.WIT_I64), a.warmup, a.reps) for count in (1, R, 16 * R)]
                   for w in (kept, plain)]
            assert kept.rows_info()[0] and not plain.rows_info()[0]
            c_bits = gens.table_info[0]
            row = (f"| 2^{lg} | {kind} | {c_bits} | {fmt(pc0)} | {fmt(pc1)} | {fmt(tot0)} | {fmt(tot1)} | {fmt(keep)} | "
                   + " / ".join(fmt(u) for u in ups[0]) + " | " + " / ".join(fmt(u) for u in ups[1]) + " |")
            print(row, flush=True)
            lines.append(row)
            del plain, kept, d_x, inst
        gens.release_device()                                        # one wide table at a time fits the card
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
