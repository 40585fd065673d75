"""What new coefficients for a live instance cost, against building the instance again (profiles/instance_set_values.md).  For the uniform and the
compiler-like synthetic circuit at each size of `--lg`, with the new coefficients in host memory and in HBM (the arrays of instance_coo_probe's I64
route: int64 where a matrix's coefficients fit, canonical bytes where not), wall time in ms:

  set_values, first call      on an instance that has never been revalued: the call that builds the slot maps (one fresh instance per sample)
  set_values, later calls     median, min - max of `--reps` after `--warmup`
  free + from_coo             the instance dropped and otti_instance_from_coo run again over the same index arrays and the new coefficients — the
                              route there was before set_values, its code unchanged, timed in the same run
  revalue                     otti_comp_comm_revalue after a set_values
  encode                      otti_snark_encode of a fresh instance (the instance itself not counted)

and the two kernels of a later call by HIP events (otti_k_instance_values_kernel_ms) with the bytes they move: convert reads the source and writes
36 bytes per entry (value + code); place reads 40 (+ 4 with codes) and writes 64 (+ 8 with codes).

    python tools/instance_values_probe.py [--lg 16 20] [--reps 7] [--warmup 2] [--no-snark] [--out profiles/instance_set_values.md]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import otti_amd as oa  # noqa: E402
from instance_coo_probe import as_int64, dev_bytes, device_call  # noqa: E402

_vp = ctypes.c_void_p
Vals = oa.api._CooValues


def fmt(c):
    return f"{statistics.median(c):.2f} ({min(c):.2f} - {max(c):.2f})"


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def device_set(inst, dev):
    m = (Vals * 3)(*[Vals(v.ptr, n, oa.WIT_I64 if v.nbytes_each == 8 else oa.WIT_CANONICAL32, 0) for _, _, v, n in dev])
    oa.api._check(oa.lib.otti_instance_set_values(inst._h, m, 1, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, nargs="+", default=[16, 20]); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-snark", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_set_values.md"))
    a = ap.parse_args()
    if oa.device_count() < 1:
        raise SystemExit("instance_values_probe: no MI355X visible")
    oa.Instance.new(2, 2, 0, *[np.zeros(0, dtype=oa.ENTRY_DTYPE)] * 3).prepare_device()       # the runtime and this thread's context are up before anything is timed
    head = ["| circuit | entries | source | set_values first | set_values later | free + from_coo | later / rebuild | convert ms | convert GB/s | place ms | place GB/s |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    snark_head = ["| circuit | N | revalue | encode | revalue / encode |", "|---|---|---|---|---|"]
    rows, snark_rows, verdicts = [], [], []
    for lg in a.lg:
        for name, synth in (("uniform", oa.synth_r1cs), ("compiler-like", oa.synth_r1cs_compiler_like)):
            r = synth(1 << lg, 10, 1)
            dims = (r["num_cons"], r["num_vars"], r["num_inputs"])
            ents = [r[m] for m in "ABC"]
            total = sum(len(e) for e in ents)
            idx = [(np.ascontiguousarray(e["row"]).astype(np.int64), np.ascontiguousarray(e["col"]).astype(np.int64)) for e in ents]
            canon = [np.ascontiguousarray(e["val"]) for e in ents]
            mixed = [v if x is None else x for x, v in zip([as_int64(v) for v in canon], canon)]
            src_bytes = sum(x.nbytes for x in mixed)
            dev = [(dev_bytes(i[0]), dev_bytes(i[1]), dev_bytes(x, 8 if x.ndim == 1 else 32), len(x)) for i, x in zip(idx, mixed)]
            host_mats = [(i[0], i[1], x) for i, x in zip(idx, mixed)]
            for source in ("host", "device"):
                build = (lambda: oa.Instance.from_coo(*dims, *host_mats)) if source == "host" else (lambda: device_call(dims, dev))
                setv = (lambda inst: inst.set_values(*mixed)) if source == "host" else (lambda inst: device_set(inst, dev))
                first, later, rebuild = [], [], []
                for k in range(a.warmup + a.reps):
                    inst = build()
                    t = timed(lambda: setv(inst))[0]
                    if k >= a.warmup:
                        first.append(t)
                    del inst
                inst = build()
                setv(inst)
                codes = inst.device_info()["use_small"]
                for k in range(a.warmup + a.reps):
                    t = timed(lambda: setv(inst))[0]
                    if k >= a.warmup:
                        later.append(t)
                conv_ms, place_ms = inst.values_kernel_ms()
                for k in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    del inst
                    inst = build()
                    if k >= a.warmup:
                        rebuild.append((time.perf_counter() - t0) * 1e3)
                del inst
                conv_b, place_b = src_bytes + 36 * total, (40 + 64 + (12 if codes else 0)) * total
                ratio = statistics.median(later) / statistics.median(rebuild)
                row = (f"| {name} 2^{lg} | {total} | {source} | {fmt(first)} | {fmt(later)} | {fmt(rebuild)} | {ratio:.3f} | {conv_ms:.3f} | "
                       f"{conv_b / (conv_ms * 1e-3) / 1e9:.0f} | {place_ms:.3f} | {place_b / (place_ms * 1e-3) / 1e9:.0f} |")
                print(row, flush=True)
                rows.append(row)
                if lg == max(a.lg) and name == "compiler-like":
                    verdicts.append((f"set_values ({source} source, later calls) at 2^{lg} compiler-like", statistics.median(later), "free + from_coo", statistics.median(rebuild)))
            if a.no_snark:
                continue
            gens = oa.SNARKGens.new(*dims, max(len(e) for e in ents))
            inst = device_call(dims, dev)
            comm = oa.ComputationCommitment.encode(inst, gens)
            reval, enc = [], []
            for k in range(a.warmup + a.reps):
                device_set(inst, dev)
                t = timed(lambda: comm.revalue(inst, gens))[0]
                if k >= a.warmup:
                    reval.append(t)
            n_ops = comm.dims[3]
            del comm
            for k in range(a.warmup + a.reps):
                t, c2 = timed(lambda: oa.ComputationCommitment.encode(inst, gens))
                del c2
                if k >= a.warmup:
                    enc.append(t)
            del inst, gens
            row = f"| {name} 2^{lg} | {n_ops} | {fmt(reval)} | {fmt(enc)} | {statistics.median(reval) / statistics.median(enc):.3f} |"
            print(row, flush=True)
            snark_rows.append(row)
            if lg == max(a.lg) and name == "compiler-like":
                verdicts.append((f"revalue at 2^{lg} compiler-like", statistics.median(reval), "encode", statistics.median(enc)))
            del dev
    first_lines = [f"{what}: {x:.2f} ms against {other} {y:.2f} ms — {'faster' if x < y else 'NOT faster'}." for what, x, other, y in verdicts]
    lines = ["# New coefficients for a live instance against building it again", ""] + first_lines + ["",
             f"    python tools/instance_values_probe.py --lg {' '.join(str(k) for k in a.lg)} --reps {a.reps} --warmup {a.warmup}", "",
             f"Wall time of the whole call in ms (median, min - max of {a.reps} after {a.warmup} warm-up calls).  first: the call that builds the slot maps, on a fresh",
             "instance per sample.  free + from_coo: the instance dropped and built again from the same arrays — the only route before set_values, its",
             "code unchanged, timed in the same run.  convert / place: one later call's launches over all three matrices by HIP events, and the bytes",
             "they move over that time (convert: source + 36 per entry; place: 40 read + 64 written per entry, 12 more with codes).", ""] + head + rows
    if snark_rows:
        lines += ["", "revalue: otti_comp_comm_revalue behind a set_values (device source).  encode: otti_snark_encode of the same instance, the instance itself", "not counted.", ""]
        lines += snark_head + snark_rows
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
