#!/usr/bin/env python3
"""Witness ingest, host pair against device path, in one process on one box.

    python tools/witness_zkif_probe.py [--sizes 16,18,20] [--reps 7] [--out FILE]

For every size (2^k constraints) and both synthetic distributions it writes the zkInterface triple once, makes the instance once (outside every
timed region) and times, `reps` times each after one warm-up, the ways from the .inp.zkif and .wit.zkif files to a resident witness:
  host    otti_witness_from_zkif(OTTI_INGEST_HOST)      (the host loader's frame over the two files, then the upload path)
  device  otti_witness_from_zkif(OTTI_INGEST_DEVICE)    (its three laps from otti_witness_ingest_info)
and, as the yardstick a build without that call has too, what the witness file adds to the older calls:
  older   otti_zkif_load(circuit, inputs, witness) - otti_zkif_load(circuit, inputs) + otti_witness_upload     (medians)
The witness of a repetition is freed outside the timed region.  The pinned host-to-device rate is measured in the same run with a pinned torch
tensor of the witness file's size: `of rate` = (witness bytes / pinned rate) / device wall.  The device path "wins" at a size when host median -
device median exceeds both ways' (max - min).  A build without otti_witness_from_zkif prints the `older` column alone."""
import argparse
import gc
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pinned_rate(torch, nbytes, reps=5):
    src = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    best = 0.0
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); dst.copy_(src, non_blocking=True); b.record(); b.synchronize()
        best = max(best, nbytes / (a.elapsed_time(b) * 1e-3))
    del src, dst
    torch.cuda.empty_cache()
    return best


def timed(fn, reps):
    out = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        keep = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if k:
            out.append((dt, keep[1]))
        del keep
        gc.collect()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,18,20"); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--out")
    a = ap.parse_args()
    import torch                                               # before otti_amd: torch has to bring the GPU up first, so that both use one HIP runtime
    if not torch.cuda.is_available():
        raise SystemExit("witness_zkif_probe: torch sees no GPU")
    torch.cuda.init()
    sys.path.insert(0, ROOT)
    import otti_amd as oa
    have = hasattr(oa.Witness, "from_zkif")
    d = tempfile.mkdtemp(prefix="witness-p-")
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))
    med = lambda xs: statistics.median(xs)
    try:
        say("`tools/witness_zkif_probe.py --sizes %s --reps %d`: wall ms from the inputs and witness files to a resident witness, median of %d after one "
            "warm-up (min - max in brackets); the device path's three laps (medians); the pinned host-to-device rate of the same run; and what the witness "
            "file adds to the older calls (zkif_load with - without it, + upload)." % (a.sizes, a.reps, a.reps))
        say()
        say("| circuit | witness MB | host path ms | device path ms | host walk | staging + copies | kernel | pinned GB/s | of rate | device wins | older calls ms |")
        say("|---|---|---|---|---|---|---|---|---|---|---|")
        for k in sorted(int(s) for s in a.sizes.split(",")):
            for kind, synth in (("uniform", oa.synth_r1cs), ("compiler-like", oa.synth_r1cs_compiler_like)):
                paths = [os.path.join(d, "%s%d%s" % (kind[0], k, e)) for e in (".zkif", ".inp.zkif", ".wit.zkif")]
                oa.zkif_write(synth(1 << k, 10, 1), *paths)
                nbytes = os.path.getsize(paths[2])
                asg = oa.zkif_load(*paths)
                inst = oa.Instance.new(asg["num_cons"], asg["num_vars"], asg["num_inputs"], asg["A"], asg["B"], asg["C"])
                inst.prepare_device()
                v, i = oa.VarsAssignment.new(asg["vars"]), oa.InputsAssignment.new(asg["inputs"])
                del asg

                def load3():
                    return oa.zkif_load(*paths), None

                def load2():
                    return oa.zkif_load(paths[0], paths[1]), None

                def upload():
                    return oa.Witness(inst, v, i), None

                older = med([x[0] for x in timed(load3, a.reps)]) - med([x[0] for x in timed(load2, a.reps)]) + med([x[0] for x in timed(upload, a.reps)])
                if not have:
                    say("| 2^%d %s | %.1f | - | - | - | - | - | - | - | - | %.1f |" % (k, kind, nbytes / 1e6, older))
                    continue

                def host():
                    return oa.Witness.from_zkif(inst, paths[1], paths[2], mode="host")[0], None

                def device():
                    w = oa.Witness.from_zkif(inst, paths[1], paths[2], mode="device")[0]
                    return w, w.ingest_info()["ms"]

                h, dv = timed(host, a.reps), timed(device, a.reps)
                rate = pinned_rate(torch, nbytes)
                hw, dw = [x[0] for x in h], [x[0] for x in dv]
                laps = [med([x[1][j] for x in dv]) for j in range(3)]
                hm, dm = med(hw), med(dw)
                wins = hm - dm > max(max(hw) - min(hw), max(dw) - min(dw))
                say("| 2^%d %s | %.1f | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.2f | %.2f | %.2f | %.1f | %.0f %% | %s | %.1f |" % (
                    k, kind, nbytes / 1e6, hm, min(hw), max(hw), dm, min(dw), max(dw), laps[0], laps[1], laps[2], rate / 1e9,
                    100.0 * (nbytes / rate) / (dm * 1e-3), "yes" if wins else "no", older))
                for p in paths:
                    os.remove(p)
        if a.out:
            open(a.out, "w").write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
