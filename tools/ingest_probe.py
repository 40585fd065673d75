#!/usr/bin/env python3
"""Circuit ingest, host path against device path, in one process on one box.

    python tools/ingest_probe.py [--sizes 16,20] [--reps 7] [--out FILE]

For every size (2^k constraints) and both synthetic distributions it writes the zkInterface triple once and times, `reps` times each after one
warm-up, the two ways from the files to an instance whose device copy is ready:
  host    otti_instance_from_zkif(OTTI_INGEST_HOST) + otti_prepare_device   (zkif_load, Instance::new, upload, CSR build)
  device  otti_instance_from_zkif(OTTI_INGEST_DEVICE)                       (its four laps from otti_instance_ingest_info)
The instance of a repetition is freed outside the timed region.  The yardstick of the device path is the pinned host-to-device rate, measured in
the same run with a pinned torch tensor of the circuit file's size: `of rate` = (circuit bytes / pinned rate) / device wall.  `spread` is
(max - min) / median of a way's repetitions; the device path "wins" at a size when host median - device median exceeds both ways' (max - min)."""
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
    ap.add_argument("--sizes", default="16,20"); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--out")
    a = ap.parse_args()
    import torch                                               # before otti_amd: torch has to bring the GPU up first, so that both use one HIP runtime
    if not torch.cuda.is_available():
        raise SystemExit("ingest_probe: torch sees no GPU")
    torch.cuda.init()
    sys.path.insert(0, ROOT)
    import otti_amd as oa
    d = tempfile.mkdtemp(prefix="ingest-p-")
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))
    try:
        say("`tools/ingest_probe.py --sizes %s --reps %d`: wall ms from the three files to an instance with its device copy ready, median of %d after one "
            "warm-up (min - max in brackets); the device path's four laps (medians); the pinned host-to-device rate of the same run." % (a.sizes, a.reps, a.reps))
        say()
        say("| circuit | circuit MB | host path ms | device path ms | host walk + id map | staging + copies | kernels | CSR build | pinned GB/s | of rate | device wins |")
        say("|---|---|---|---|---|---|---|---|---|---|---|")
        for k in sorted(int(s) for s in a.sizes.split(",")):
            for kind, synth in (("uniform", oa.synth_r1cs), ("compiler-like", oa.synth_r1cs_compiler_like)):
                paths = [os.path.join(d, "%s%d%s" % (kind[0], k, e)) for e in (".zkif", ".inp.zkif", ".wit.zkif")]
                oa.zkif_write(synth(1 << k, 10, 1), *paths)
                nbytes = os.path.getsize(paths[0])

                def host():
                    inst, asg = oa.Instance.from_zkif(*paths, mode="host")
                    inst.prepare_device()
                    return inst, None

                def device():
                    inst, asg = oa.Instance.from_zkif(*paths, mode="device")
                    return inst, inst.ingest_info()["ms"]

                h, dv = timed(host, a.reps), timed(device, a.reps)
                rate = pinned_rate(torch, nbytes)
                hw, dw = [x[0] for x in h], [x[0] for x in dv]
                laps = [statistics.median(x[1][j] for x in dv) for j in range(4)]
                hm, dm = statistics.median(hw), statistics.median(dw)
                wins = hm - dm > max(max(hw) - min(hw), max(dw) - min(dw))
                say("| 2^%d %s | %.0f | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.1f | %.1f | %.1f | %.1f | %.1f | %.0f %% | %s |" % (
                    k, kind, nbytes / 1e6, hm, min(hw), max(hw), dm, min(dw), max(dw), laps[0], laps[1], laps[2], laps[3], rate / 1e9,
                    100.0 * (nbytes / rate) / (dm * 1e-3), "yes" if wins else "no"))
                for p in paths:
                    os.remove(p)
        if a.out:
            open(a.out, "w").write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
