"""What keeping a resident witness's products Az, Bz, Cz buys and costs (profiles/witness_products.md), and from which touched share of the rows on the
full pass is no slower than the patch: the figure behind kProductsFullShare (device.h).  For a size of `--lg`, on the uniform and the compiler-like
instance, in ONE process with one generator table, kept rows on everywhere:

  1. the step of a caller that changes k = 1, 64, 4096 variables: otti_witness_scatter, otti_witness_check_sat (the count alone) and
     otti_nizk_prove_resident, on a witness that keeps rows and one that keeps rows and products, alternating inside one loop;
  2. the patch against the touched share of the rows (otti_k_products_patch with OTTI_PRODUCTS_FULL_SHARE=1, its device time from the first launch
     to the last, the host's read of the touched count included), beside the full pass as the code without this feature runs it: dev_spmv3
     (otti_k_multiply_vec's kernel time) plus dev_sat_pass (otti_witness_check_sat's kernel time on a witness that keeps no products) — the code
     under test is never its own yardstick — and, for information, this feature's own full pass (OTTI_PRODUCTS_FULL_SHARE=0);
  3. otti_nizk_prove_resident alone, 3 x `--reps` proofs per witness, alternating: the condition is that rows + products is no slower than rows alone
     on the uniform instance within the spread recorded here.

    python tools/witness_products_probe.py [--lg 20] [--reps 15] [--warmup 3] [--out profiles/witness_products.md]

Host-clock timings are around calls that end synchronised."""
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


def pow2_floor(x):
    p = 1.0
    while p > x:
        p /= 2
    return p


def z_of(wit):
    p, n, _ = wit.info
    out = np.zeros((n, 32), dtype=np.uint8)
    assert oa.lib.otti_dev_download(out.ctypes.data_as(_vp), p, out.nbytes) == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=20); ap.add_argument("--reps", type=int, default=15); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_products.md"))
    a = ap.parse_args()
    if oa.device_count() < 1:
        raise SystemExit("witness_products_probe: no MI355X visible")
    os.environ.pop("OTTI_PRODUCTS_FULL_SHARE", None)
    n = 1 << a.lg
    rng = np.random.default_rng(1)
    label, seed = b"products probe", b"\x2a" * 32
    step = ["| constraints | instance | k | rows recomputed per scatter | scatter: rows / rows + products | check_sat: rows / rows + products | prove: rows / rows + products | multiply_vec stage: rows / rows + products |",
            "|---|---|---|---|---|---|---|---|"]
    curve = ["| constraints | instance | columns changed | rows touched | share of N | patch | full pass, yardstick (spmv3 + sat pass) | full pass, this feature |", "|---|---|---|---|---|---|---|---|"]
    prove = ["| constraints | instance | prove, rows | prove, rows + products | multiply_vec stage, rows | multiply_vec stage, rows + products |", "|---|---|---|---|---|---|"]
    cross = {}
    gens = None
    for kind, synth in (("uniform", oa.synth_r1cs), ("compiler-like", oa.synth_r1cs_compiler_like)):
        r = synth(n, 10, 1)
        inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
        N, V, _ = inst.dims
        if gens is None:
            gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
        vars32 = np.zeros((V, 32), dtype=np.uint8)
        vars32[:r["vars"].shape[0]] = r["vars"]
        inputs = oa.InputsAssignment.new(r["inputs"])
        inst.prepare_device(gens)
        wits = {}
        for name in ("rows", "rows + products"):
            w = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), inputs)
            w.keep_rows(inst, gens)
            if name != "rows":
                w.keep_products(inst)
            wits[name] = w
        order = ("rows", "rows + products")

        # ---- 3 first, on the untouched (satisfied) assignment: the proof alone
        tp, ts = {k: [] for k in order}, {k: [] for k in order}
        for rep in range(a.warmup + 3 * a.reps):
            for name in order:
                t0 = time.perf_counter()
                pf = oa.NIZK.prove(inst, wits[name], None, gens, label, seed)
                t1 = time.perf_counter()
                if rep >= a.warmup:
                    tp[name].append((t1 - t0) * 1e3); ts[name].append(pf.stage_ms["multiply_vec"])
        row = f"| 2^{a.lg} | {kind} | {fmt(tp['rows'])} | {fmt(tp['rows + products'])} | {fmt(ts['rows'])} | {fmt(ts['rows + products'])} |"
        print(row, flush=True); prove.append(row)

        # ---- 1. the step
        for k in (1, 64, 4096):
            idx = np.sort(rng.choice(V, size=k, replace=False)).astype(np.uint64)
            t = {name: {"scatter": [], "check": [], "prove": [], "stage": []} for name in order}
            before = wits["rows + products"].products_info()
            for rep in range(a.warmup + a.reps):
                new = vars32[(idx.astype(np.int64) * 7 + 1 + rep) % V]          # other elements of the same witness
                d_idx, d_new = dev_bytes(idx), dev_bytes(new)
                for name in order:
                    w = wits[name]
                    t0 = time.perf_counter()
                    rc = oa.lib.otti_witness_scatter(inst._h, w._h, d_idx.ptr, d_new.ptr, k, oa.WIT_CANONICAL32, 0, 1, None)
                    t1 = time.perf_counter()
                    assert rc == 0, rc
                    rep_ = w.check_sat(inst, max_rows=0, values=False)
                    t2 = time.perf_counter()
                    pf = oa.NIZK.prove(inst, w, None, gens, label, seed)
                    t3 = time.perf_counter()
                    if rep >= a.warmup:
                        t[name]["scatter"].append((t1 - t0) * 1e3); t[name]["check"].append((t2 - t1) * 1e3)
                        t[name]["prove"].append((t3 - t2) * 1e3); t[name]["stage"].append(pf.stage_ms["multiply_vec"])
                vars32[idx.astype(np.int64)] = new
            after = wits["rows + products"].products_info()
            calls = (after["patches"] + after["full_passes"]) - (before["patches"] + before["full_passes"])
            per = (after["rows_recomputed"] - before["rows_recomputed"]) / max(1, after["patches"] - before["patches"])
            how = f"{per:.0f}" + (f" ({after['full_passes'] - before['full_passes']} of {calls} calls took the full pass)" if after["full_passes"] != before["full_passes"] else "")
            row = (f"| 2^{a.lg} | {kind} | {k} | {how} | " + " | ".join(f"{fmt(t['rows'][c])} / {fmt(t['rows + products'][c])}" for c in ("scatter", "check", "prove", "stage")) + " |")
            print(row, flush=True); step.append(row)

        # ---- 2. the patch against the touched share, beside the full pass
        z = z_of(wits["rows"])
        Az, Bz, Cz, _ = oa.kernels.multiply_vec(inst, z)
        words = (N + 63) // 64
        d_bits = oa.DeviceArray(words, 8)
        unsat = oa.kernels_dev.check_sat(inst, oa.DeviceArray.from_host(z), d_bits)
        bits = d_bits.to_host().reshape(-1).view(np.uint64)
        points = []
        for lgk in (0, 4, 8, 12, 14, 16, 17, 18, 19, a.lg):
            k = min(1 << lgk, V)
            cols = np.sort(rng.choice(V, size=k, replace=False)).astype(np.uint64)
            z_new = z.copy()
            z_new[cols.astype(np.int64)] = z[(cols.astype(np.int64) * 7 + 1) % V]
            tpatch, tfull, tyard, touched = [], [], [], 0
            for rep in range(1 + max(5, a.reps // 2)):
                os.environ["OTTI_PRODUCTS_FULL_SHARE"] = "1"
                out = oa.kernels.products_patch(inst, z_new, Az, Bz, Cz, bits, unsat, cols=cols)
                assert not out[6]
                touched = len(out[5])
                os.environ["OTTI_PRODUCTS_FULL_SHARE"] = "0"
                out0 = oa.kernels.products_patch(inst, z_new, Az, Bz, Cz, bits, unsat, cols=cols)
                assert out0[6] and out0[4] == out[4]
                os.environ.pop("OTTI_PRODUCTS_FULL_SHARE")
                ms_spmv = oa.kernels.multiply_vec(inst, z_new)[3]
                ms_sat = wits["rows"].check_sat(inst, max_rows=0, values=False).kernel_ms
                if rep >= 1:
                    tpatch.append(out[7]); tfull.append(out0[7]); tyard.append(ms_spmv + ms_sat)
            share = touched / N
            points.append((share, statistics.median(tpatch), statistics.median(tyard)))
            row = f"| 2^{a.lg} | {kind} | {k} | {touched} | {share:.4f} | {fmt(tpatch)} | {fmt(tyard)} | {fmt(tfull)} |"
            print(row, flush=True); curve.append(row)
        sw = next((s for s, p, y in points if s > 0 and p >= y), None)
        cross[kind] = (sw, pow2_floor(sw) if sw else None)
        del wits, inst
    gens.release_device()
    cmd = f"python tools/witness_products_probe.py --lg {a.lg} --reps {a.reps} --warmup {a.warmup}"
    lines = ["# Kept products of a resident witness: Az, Bz, Cz patched by the touched rows", "", f"    {cmd}", "",
             "Milliseconds: median (min - max).  One MI355X, one process, one run of the probe; kept rows are on for every witness.", "",
             "## The proof alone", "",
             f"otti_nizk_prove_resident, host clock, {3 * a.reps} proofs per witness after {a.warmup} warm-up rounds, the two witnesses alternating; the multiply_vec stage is the",
             "prover's own stage clock (it ends when the host has the commitment, so it mostly shows the queue ahead of the products).", ""] + prove + ["",
             "## The step: scatter, check, prove", "",
             f"Host clock around each call, {a.reps} steps after {a.warmup} warm-up rounds, the two witnesses alternating inside one loop.  The scatter's values are other",
             "elements of the same witness; check_sat asks for the count alone (max_rows = 0).", ""] + step + ["",
             "## The patch against the touched share of the rows", "",
             "Device time (HIP events).  Patch: otti_k_products_patch with the patch forced, from its first launch to its last, the host's read of the touched count",
             "included.  Yardstick: the full pass on the code path that exists without this feature, dev_spmv3 (otti_k_multiply_vec's kernel time) plus dev_sat_pass",
             "(otti_witness_check_sat's kernel time on a witness that keeps no products).  Last column, for information: this feature's own full pass (forced).", ""] + curve + ["",
             "The smallest probed share at which the patch is no longer shorter than the yardstick, and that share rounded down to a power of two (toward the full pass):", ""]
    for kind, (sw, p2) in cross.items():
        lines.append(f"* {kind}: " + (f"{sw:.4f} -> {p2}" if sw else "none: the patch is shorter at every probed share"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
