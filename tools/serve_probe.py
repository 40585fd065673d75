#!/usr/bin/env python3
"""Wall time per request of `spzk-client` against a running `spzk serve` and of the one-shot `spzk`, same box, same run.

    python tools/serve_probe.py [--sizes 16,20] [--requests 20] [--warmups 2] [--table-gb G] [--window C] [--out FILE]

For every size (2^k constraints) and both synthetic distributions (uniform, compiler-like) it writes the zkInterface triple once, then times
`verify --nizk c i w` as a whole process, 2 warm-ups and 20 requests each way, and splits every request into zkif_load, setup, prove and
verify from the lines the request itself prints; the last column says where a served request's witness and circuit were read (`witness device|host`,
`ingest device|host` of its `* served:` line).  The served leg goes smallest size first, so the first request of each larger size is the
one that replaces the resident window table: its wall time is reported by itself (the rebuild), as are the table's width and bytes.
The expectation this is written to check: a served request pays no runtime start, so its wall time should be close to the sum of its own
printed stages.  Output: a markdown report (profiles/spzk_serve.md is one).  The probe process itself opens no GPU."""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import otti_amd as oa                                              # noqa: E402
from otti_amd.serve import SPZK, SPZK_CLIENT, SpzkServer           # noqa: E402

STAGES = (("zkif_load", r"^\* zkif_load ([0-9.]+) ms"), ("setup", r"^\* setup .* ([0-9.]+) ms$"), ("objs", r"^  \* host objects ([0-9.]+) ms"), ("prove", r"^\* NIZK::prove ([0-9.]+) ms"), ("verify", r"^\* NIZK::verify ([0-9.]+) ms"), ("queue", r"^\* served: queue ([0-9.]+) ms"))


def stages(stdout):
    out = {}
    for name, pat in STAGES:
        m = re.search(pat, stdout, re.M)
        out[name] = float(m.group(1)) if m else float("nan")
    return out


def served_words(stdout):
    """`witness device|host` and `ingest device|host` of a request's `* served:` line, as "witness/ingest" ("-" for a word the line does not carry:
    a one-shot has no such line, an older server no `witness` word)"""
    m = re.search(r"^\* served: (.*)$", stdout, re.M)
    line = m.group(1) if m else ""
    w, g = re.search(r"\bwitness (device|host)\b", line), re.search(r"\bingest (device|host)\b", line)
    return "%s/%s" % (w.group(1) if w else "-", g.group(1) if g else "-")


def timed(argv, cwd, env):
    t0 = time.perf_counter()
    r = subprocess.run(argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    wall = (time.perf_counter() - t0) * 1e3
    if r.returncode != 0 or not r.stdout.rstrip().endswith("Verification successful"):
        raise SystemExit("request failed (%d): %s\n%s" % (r.returncode, " ".join(argv), r.stdout + r.stderr))
    return wall, r.stdout


def leg(argv, cwd, env, warmups, requests):
    first_wall, first_out = timed(argv, cwd, env)
    for _ in range(max(0, warmups - 1)):
        timed(argv, cwd, env)
    walls, parts = [], []
    for _ in range(requests):
        w, out = timed(argv, cwd, env)
        walls.append(w); parts.append(stages(out))
    med = {k: statistics.median(p[k] for p in parts) for k, _ in STAGES}
    print("[serve_probe] %s %s: median %.1f ms" % (os.path.basename(argv[0]), argv[3], statistics.median(walls)), file=sys.stderr, flush=True)
    return dict(first_wall=first_wall, first_out=first_out, wall=statistics.median(walls), wall_min=min(walls), wall_max=max(walls), words=served_words(out), **med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20"); ap.add_argument("--requests", type=int, default=20); ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--table-gb"); ap.add_argument("--window"); ap.add_argument("--out")
    a = ap.parse_args()
    sizes = sorted(int(s) for s in a.sizes.split(","))
    env = dict(os.environ); env.pop("SPZK_SERVER", None)
    if a.table_gb:
        env["OTTI_MSM_TABLE_GB"] = a.table_gb
    if a.window:
        env["OTTI_MSM_WINDOW"] = a.window
    d = tempfile.mkdtemp(prefix="spzk-p-")
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))
    try:
        cases = []
        for k in sizes:
            for kind, synth in (("uniform", oa.synth_r1cs), ("compiler-like", oa.synth_r1cs_compiler_like)):
                name = "%s%d" % (kind[0], k)
                oa.zkif_write(synth(1 << k, 10, 1), *(os.path.join(d, name + e) for e in (".zkif", ".inp.zkif", ".wit.zkif")))
                mb = sum(os.path.getsize(os.path.join(d, name + e)) for e in (".zkif", ".inp.zkif", ".wit.zkif")) / 1e6
                cases.append((k, kind, name, mb))
        argv = lambda name: ["verify", "--nizk", name + ".zkif", name + ".inp.zkif", name + ".wit.zkif"]
        say("# `spzk-client` against `spzk serve`, and the one-shot `spzk`")
        say()
        say("`tools/serve_probe.py --sizes %s --requests %d --warmups %d%s%s`: wall time of the whole client process per request, median of %d after %d warm-ups "
            "(min – max in brackets), and the medians of the stages each request prints.  `rest` = wall − (zkif_load + setup + prove + verify)." % (
                a.sizes, a.requests, a.warmups, " --table-gb " + a.table_gb if a.table_gb else "", " --window " + a.window if a.window else "", a.requests, a.warmups))
        say()
        served, tables = {}, []
        with SpzkServer(socket_path=os.path.join(d, "s"), jobs=1, idle_exit=600, env=env, start_timeout=120) as srv:
            cenv = dict(env, SPZK_SERVER=srv.socket_path)
            last_size = None
            for k, kind, name, mb in cases:
                served[name] = leg([SPZK_CLIENT] + argv(name), d, cenv, a.warmups, a.requests)
                if k != last_size:
                    st = srv.status()
                    m = re.search(r"^\* served: .*$", served[name]["first_out"], re.M)
                    tables.append((k, kind, served[name]["first_wall"], stages(served[name]["first_out"])["setup"], m.group(0) if m else "", st["table"], st["tables_built"], st["adoptions"]))
                    last_size = k
            # the smallest size once more, now behind the largest size's table
            k, kind, name, mb = cases[0]
            again = leg([SPZK_CLIENT] + argv(name), d, cenv, a.warmups, a.requests) if len(sizes) > 1 else None
            final = srv.status()
        one = {name: leg([SPZK] + argv(name), d, env, a.warmups, a.requests) for _, _, name, _ in cases}
        say("| circuit | zkif MB | way | wall ms | zkif_load | setup | of it host objects | prove | verify | rest | of it queue | witness/ingest |")
        say("|---|---|---|---|---|---|---|---|---|---|---|---|")
        row = lambda label, mb, way, r: say("| %s | %.0f | %s | %.1f (%.1f – %.1f) | %.1f | %.1f | %.1f | %.2f | %.2f | %.1f | %.1f | %s |" % (
            label, mb, way, r["wall"], r["wall_min"], r["wall_max"], r["zkif_load"], r["setup"], r["objs"], r["prove"], r["verify"],
            r["wall"] - r["zkif_load"] - r["setup"] - r["prove"] - r["verify"], r["queue"], r["words"]))
        for k, kind, name, mb in cases:
            row("2^%d %s" % (k, kind), mb, "served", served[name]); row("2^%d %s" % (k, kind), mb, "one-shot", one[name])
        if again:
            k, kind, name, mb = cases[0]
            row("2^%d %s, adopted table" % (k, kind), mb, "served", again)
        say()
        say("The first request of each size (the server goes from the smallest size up; a larger size replaces the resident table):")
        say()
        say("| size | first request wall ms | its setup ms | its served line | table after it: c, bytes, bases | tables built | adoptions |")
        say("|---|---|---|---|---|---|---|")
        for k, kind, wall, setup, line, tab, built, adopt in tables:
            say("| 2^%d %s | %.1f | %.1f | `%s` | %d, %.2f GB, %d | %d | %d |" % (k, kind, wall, setup, line, tab["c"], tab["bytes"] / 1e9, tab["bases"], built, adopt))
        say()
        say("Server at the end: `%s`.  The one-shot runs with its own default (OTTI_MSM_WINDOW=10 unless set)." % final)
        if a.out:
            open(a.out, "w").write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
