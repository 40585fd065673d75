"""What a scatter update of a resident witness with kept rows costs against the range updates it replaces (profiles/witness_scatter.md).
For a size of `--lg`, uniform and compiler-like witness, in ONE process with one instance and one generator table, k changed variables
(1, 32 and 16384 drawn uniformly, 1024 as one per row), alternating inside one loop:

  (a) otti_witness_scatter     the k (index, value) pairs, canonical bytes already in HBM
  (b) otti_witness_update      ONE range update over [min index, max index] carrying the same final values
  (c) otti_witness_update      k single-element updates (k <= 32 only)

    python tools/witness_scatter_probe.py [--lg 20] [--reps 10] [--warmup 2] [--window C] [--out profiles/witness_scatter.md]

Every timing is a host clock around calls that end synchronised.  The new values are other elements of the same witness, so its distribution
(and with it the bulk kernel's variant in (b)) stays what it was.  `--window` pins the table's window width (OTTI_MSM_WINDOW)."""
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
    a = np.ascontiguousarray(a)
    d = oa.DeviceArray(a.nbytes, 1)
    assert oa.lib.otti_dev_upload(d.ptr, a.ctypes.data_as(_vp), a.nbytes) == 0
    return d


def fmt(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} - {max(xs):.3f})" if xs else "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=20); ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_scatter.md"))
    a = ap.parse_args()
    if a.window:
        os.environ["OTTI_MSM_WINDOW"] = str(a.window)
    if oa.device_count() < 1:
        raise SystemExit("witness_scatter_probe: no MI355X visible")
    cmd = f"python tools/witness_scatter_probe.py --lg {a.lg} --reps {a.reps} --warmup {a.warmup}" + (f" --window {a.window}" if a.window else "")
    lines = ["# Scatter update of a resident witness with kept rows", "", f"    {cmd}", "",
             f"Milliseconds, host clock around the call(s): median (min - max) of {a.reps} after {a.warmup} warm-up rounds; (a), (b) and (c) alternate inside one loop.",
             "(a) otti_witness_scatter of the k pairs; (b) one otti_witness_update over [min index, max index] with the same final values; (c) k single-element",
             "otti_witness_update calls.  Sources are canonical bytes already in HBM.  All three include the recount of small_fraction.", "",
             "| variables | witness | window c | k | rows touched | (a) scatter | (b) one range update | (c) k updates of one |", "|---|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    n = 1 << a.lg
    R = 1 << (a.lg - a.lg // 2)
    L = n // R
    gens = None
    for kind, synth in (("uniform", oa.synth_r1cs), ("compiler-like", oa.synth_r1cs_compiler_like)):
        r = synth(n, 10, 1)
        inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
        if gens is None:
            gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
        vars32 = np.zeros((n, 32), dtype=np.uint8)
        vars32[:r["vars"].shape[0]] = r["vars"]
        wit = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"]))
        inst.prepare_device(gens)
        wit.keep_rows(inst, gens)
        for k, how in ((1, "uniform"), (32, "uniform"), (min(1024, L), "one per row"), (min(16384, n), "uniform")):
            if how == "one per row":
                idx = np.arange(k, dtype=np.uint64) * np.uint64(R) + rng.integers(0, R, size=k).astype(np.uint64)
            else:
                idx = np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint64)
            lo, hi = int(idx[0]), int(idx[-1])
            ta, tb, tc = [], [], []
            for rep in range(a.warmup + a.reps):
                new = vars32[(idx.astype(np.int64) * 7 + 1 + rep) % n]           # other elements of the same witness
                span = vars32[lo:hi + 1].copy()
                span[idx.astype(np.int64) - lo] = new
                d_idx, d_new, d_span = dev_bytes(idx), dev_bytes(new), dev_bytes(span)
                t0 = time.perf_counter()
                rc = oa.lib.otti_witness_scatter(inst._h, wit._h, d_idx.ptr, d_new.ptr, k, oa.WIT_CANONICAL32, 0, 1, None)
                t1 = time.perf_counter()
                assert rc == 0, rc
                wit.update(inst, lo, (d_span.ptr.value, hi - lo + 1), fmt=oa.WIT_CANONICAL32)
                t2 = time.perf_counter()
                if k <= 32:
                    for i in range(k):
                        wit.update(inst, int(idx[i]), (d_new.ptr.value + 32 * i, 1), fmt=oa.WIT_CANONICAL32)
                t3 = time.perf_counter()
                vars32[lo:hi + 1] = span
                if rep >= a.warmup:
                    ta.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3)
                    if k <= 32:
                        tc.append((t3 - t2) * 1e3)
            rows = len(set(int(j) // R for j in idx))
            row = f"| 2^{a.lg} | {kind} | {gens.table_info[0]} | {k} {how} | {rows} | {fmt(ta)} | {fmt(tb)} | {fmt(tc)} |"
            print(row, flush=True)
            lines.append(row)
        del wit, inst
    gens.release_device()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
