#!/usr/bin/env python3
"""Served SNARK requests, this build against another build of the project (the parent commit's), on one box in one run.

    python tools/snark_ingest_probe.py --parent-root DIR [--sizes 16,20] [--reps 7] [--out FILE]
    python tools/snark_ingest_probe.py --kernels-only [--kernel-sizes 20,24] [--reps 7] [--out FILE]      (the two kernels' tables alone)

DIR holds the other build: DIR/otti_amd/{serve.py, spzk, spzk-client, libottispartan.so}.  For every size (2^k constraints) and both synthetic
distributions the zkInterface triple is written once; each build then runs one `spzk serve` (one worker, its default environment) and answers,
`reps` times each after one warm-up, a served `encode --comm-out` and a served `prove --comm-in --proof-out` of those files.  Reported: the
request's wall time at the client (median, min - max), the stage lines of its stdout (medians) and the `ingest` word of its `* served:` line (the
other build may print none).  A request "is no slower" on this build when its median exceeds the other's by no more than the smaller of the two
builds' (max - min) spreads.
Last, in this process and on this build alone, OTTI_TRACE's lap "entry lists: upload + expansion" of SNARK::encode for both fills of the
decommitment: from host lists (an instance of the host ingest: the copy-and-expand fill every instance took before) and from the entry lists in
HBM (an instance of the device ingest).  The lap runs from the start of encode: it holds the decommitment's allocations (16 N + 2 M elements) as
well, so the kernels themselves are timed apart, by HIP events around their launches (otti_k_decomm_entries, otti_k_shard_filter: kernel_ms), on
random lists, with the bytes they move: the fill 40 read per entry and 104 written per position, the filter as its table says."""
import argparse
import importlib.util
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = (("zkif_load", r"^\* zkif_load ([0-9.]+) ms"), ("setup", r"^\* setup .* ([0-9.]+) ms$"), ("encode", r"^\* SNARK::encode ([0-9.]+) ms"),
          ("attach", r"^\* attach.* ([0-9.]+) ms \("), ("prove", r"^\* SNARK::prove ([0-9.]+) ms"))
LAP = re.compile(r"snark_encode entry lists: upload \+ expansion\s+([0-9.]+) ms")


def load_serve(root):
    spec = importlib.util.spec_from_file_location("serve_" + re.sub(r"\W", "_", root), os.path.join(root, "otti_amd", "serve.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def served_leg(serve, work, names, reps, timeout):
    """{(name, request): [(wall ms, {stage: ms}, ingest word)] * reps} from one server of the build `serve` belongs to"""
    out = {}
    srv = serve.SpzkServer(socket_path=os.path.join(work, "sock"), jobs=1, idle_exit=600, start_timeout=120)
    srv.start()
    try:
        for name in names:
            files = [name + e for e in (".zkif", ".inp.zkif", ".wit.zkif")]
            for req, argv in (("encode", ["encode"] + files[:2] + ["--comm-out", name + ".comm"]),
                              ("prove", ["prove"] + files + ["--comm-in", name + ".comm", "--proof-out", name + ".proof", "--seed", "2a" * 32])):
                rows = []
                for k in range(reps + 1):
                    t0 = time.perf_counter()
                    res = srv.run(argv, cwd=work, timeout=timeout)
                    wall = (time.perf_counter() - t0) * 1e3
                    if res.returncode != 0:
                        raise SystemExit("snark_ingest_probe: %s %s failed: %s" % (req, name, res.stderr))
                    stages = {s: float(m.group(1)) for s, pat in STAGES for m in [re.search(pat, res.stdout, re.M)] if m}
                    m = re.search(r"^\* served: .*ingest (\w+)$", res.stdout, re.M)
                    if k:
                        rows.append((wall, stages, m.group(1) if m else "-"))
                out[(name, req)] = rows
    finally:
        status = srv.close(timeout=120)
    if status != 0 or srv.abnormal_end:
        raise SystemExit("snark_ingest_probe: the server ended badly: %s" % (srv.abnormal_end or status))
    return out


def med(rows, stage=None):
    v = [r[0] if stage is None else r[1].get(stage, float("nan")) for r in rows]
    return statistics.median(v)


def fill_laps(oa, paths, reps):
    """medians of the traced lap for both fills, in this process: stderr goes to a file while encode runs"""
    out = {}
    for mode in ("host", "device"):
        inst, a = oa.Instance.from_zkif(*paths, mode=mode)
        gens = oa.SNARKGens.new(a["num_cons"], a["num_vars"], a["num_inputs"], max(a["nA"], a["nB"], a["nC"]))
        laps = []
        for k in range(reps + 1):
            with tempfile.TemporaryFile() as f:
                sys.stderr.flush()
                keep = os.dup(2)
                os.dup2(f.fileno(), 2)
                try:
                    oa.ComputationCommitment.encode(inst, gens)
                finally:
                    os.dup2(keep, 2); os.close(keep)
                f.seek(0)
                m = LAP.search(f.read().decode(errors="replace"))
            if k and m:
                laps.append(float(m.group(1)))
        out[mode] = (statistics.median(laps) if laps else float("nan"), a, inst.host_lists_info()["materialised"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root"); ap.add_argument("--kernels-only", action="store_true"); ap.add_argument("--sizes", default="16,20"); ap.add_argument("--kernel-sizes", default="20,24"); ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=float, default=300.0); ap.add_argument("--out")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import otti_amd as oa
    if oa.device_count() < 1:
        raise SystemExit("snark_ingest_probe: no GPU")
    if not a.kernels_only and not a.parent_root:
        raise SystemExit("snark_ingest_probe: --parent-root DIR, or --kernels-only")
    work = tempfile.mkdtemp(prefix="snark-p-")
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))
    try:
        if not a.kernels_only:
            builds = (("parent", load_serve(os.path.abspath(a.parent_root))), ("this", load_serve(ROOT)))
            names, meta = [], {}
            for k in sorted(int(s) for s in a.sizes.split(",")):
                for kind, synth in (("uniform", oa.synth_r1cs), ("compiler-like", oa.synth_r1cs_compiler_like)):
                    name = "%s%d" % (kind[0], k)
                    oa.zkif_write(synth(1 << k, 10, 1), *[os.path.join(work, name + e) for e in (".zkif", ".inp.zkif", ".wit.zkif")])
                    names.append(name); meta[name] = ("2^%d %s" % (k, kind), os.path.getsize(os.path.join(work, name + ".zkif")), os.path.getsize(os.path.join(work, name + ".wit.zkif")))
            say("`tools/snark_ingest_probe.py --sizes %s --reps %d`: served SNARK requests, wall ms at the client, median of %d after one warm-up (min - max); "
                "stage lines of the request's stdout (medians)." % (a.sizes, a.reps, a.reps))
            say()
            res = {b: served_leg(serve, work, names, a.reps, a.timeout) for b, serve in builds}
            say("| circuit | circuit MB | witness MB | request | parent ms | this ms | this / parent | no slower | parent zkif_load + setup | this zkif_load + setup | parent encode or attach | this encode or attach | prove (parent, this) | ingest (parent, this) |")
            say("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
            for name in names:
                for req in ("encode", "prove"):
                    p, t = res["parent"][(name, req)], res["this"][(name, req)]
                    pw, tw = [r[0] for r in p], [r[0] for r in t]
                    ok = med(t) - med(p) <= min(max(pw) - min(pw), max(tw) - min(tw))
                    fill = "encode" if req == "encode" else "attach"
                    say("| %s | %.0f | %.0f | %s | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.2f | %s | %.1f + %.1f | %.1f + %.1f | %.1f | %.1f | %s | %s, %s |" % (
                        meta[name][0], meta[name][1] / 1e6, meta[name][2] / 1e6, req, med(p), min(pw), max(pw), med(t), min(tw), max(tw), med(t) / med(p), "yes" if ok else "NO",
                        med(p, "zkif_load"), med(p, "setup"), med(t, "zkif_load"), med(t, "setup"), med(p, fill), med(t, fill),
                        "%.1f, %.1f" % (med(p, "prove"), med(t, "prove")) if req == "prove" else "-", p[0][2], t[0][2]))
            say()
            say("The decommitment fill alone, this build, in one process (`OTTI_TRACE` lap \"entry lists: upload + expansion\" of SNARK::encode, median of %d after one warm-up):" % a.reps)
            say()
            say("| circuit | entries A + B + C | positions N | from host lists ms | from the lists in HBM ms | bytes moved | achieved GB/s | host lists made |")
            say("|---|---|---|---|---|---|---|---|")
            os.environ["OTTI_TRACE"] = "1"
            for name in names:
                laps = fill_laps(oa, [os.path.join(work, name + e) for e in (".zkif", ".inp.zkif", ".wit.zkif")], a.reps)
                asg = laps["device"][1]
                nnz = [asg["nA"], asg["nB"], asg["nC"]]
                N = 1 << max(1, (max(nnz) - 1).bit_length())
                moved = 40 * sum(nnz) + 3 * 104 * N + 32 * N                 # read per entry, written per position, and the zeroed sixteenth part
                say("| %s | %d | %d | %.3f | %.3f | %.1f MB | %.0f | %s, %s |" % (meta[name][0], sum(nnz), N, laps["host"][0], laps["device"][0], moved / 1e6,
                                                                             moved / (laps["device"][0] * 1e-3) / 1e9, "yes" if laps["host"][2] else "no", "yes" if laps["device"][2] else "no"))
        say()
        say("The shard filter alone (`otti_k_shard_filter`, a random list, world 2, rank 0; kernel ms = flag + scan + the read of the count + scatter, median of %d):" % a.reps)
        say()
        say("| entries | by | kernel ms | bytes moved | achieved GB/s |")
        say("|---|---|---|---|---|")
        import numpy as np
        rng = np.random.default_rng(1)
        fill_rows = []
        for k in sorted(int(s) for s in a.kernel_sizes.split(",")):
            n = 1 << k
            row, col = rng.integers(0, 2 ** 31, n, dtype=np.uint32), rng.integers(0, 2 ** 31, n, dtype=np.uint32)
            val = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            ms = [oa.kernels.decomm_entries(row, col, val, n)[5] for _ in range(a.reps + 1)][1:]
            fill_rows.append("| 2^%d | 2^%d | %.3f | %.1f MB | %.0f |" % (k, k, statistics.median(ms), 144 * n / 1e6, 144 * n / (statistics.median(ms) * 1e-3) / 1e9))
            for by_col in (False, True):
                ms, kept = [], 0
                for j in range(a.reps + 1):
                    r, _, _, t = oa.kernels.shard_filter(row, col, val, 2, 0, by_col)
                    kept = r.size
                    if j:
                        ms.append(t)
                moved = n * (4 + 4) + n * 8 + n * (8 + 4) + kept * (32 + 40)   # flag, scan, the scatter's reads, and what stays: value read, entry written
                say("| 2^%d | %s | %.3f | %.1f MB | %.0f |" % (k, "column" if by_col else "row", statistics.median(ms), moved / 1e6, moved / (statistics.median(ms) * 1e-3) / 1e9))
        say()
        say("The fill kernel alone (`otti_k_decomm_entries`, one matrix, a random list of n = N entries; kernel ms, median of %d):" % a.reps)
        say()
        say("| entries | positions N | kernel ms | bytes moved | achieved GB/s |")
        say("|---|---|---|---|---|")
        for r in fill_rows:
            say(r)
        if a.out:
            open(a.out, "w").write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
