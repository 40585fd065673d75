"""What verifying K proofs of one instance in one call buys (profiles/verify_many.md): the figures behind kEvalTile, kEvalChunk (device.h) and
kVerifyManyThreads (spartan.h).  Per size of `--lgs`, on the uniform and the compiler-like instance, K = 2, 4, 8, 16 proofs of one resident witness
(one seed each: the points differ), in ONE process, median of `--reps` after `--warmup`, with min - max:

  (i)  device time of the batched evaluation of A, B, C at the K points (otti_k_instance_evaluate's kernel_ms: eq tables, interleave, the walks)
       beside K x the device time of the single evaluation as otti_nizk_verify runs it on the same instance (otti_stats_read around the call: the
       eq, spmv and reduce classes, which in a verifier are the evaluation's launches alone) — the code under test is never its own yardstick;
  (ii) wall time of otti_nizk_verify_many with 2, 4 and 8 workers beside K sequential otti_nizk_verify calls and beside the same K calls issued
       from as many caller threads (the best a caller can do without the new entry), the three alternating inside one loop.

    python tools/verify_many_probe.py [--lgs 16,20] [--reps 7] [--warmup 1] [--out tables.md]

Host-clock timings are around calls that end synchronised.  The generator table is built with a 4 GiB budget (OTTI_MSM_TABLE_GB, unless set): the
table serves the six-odd proofs made here and the verifier's one fixed-base sum, the same for every column of a row."""
import argparse
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OTTI_MSM_TABLE_GB", "4")
import otti_amd as oa  # noqa: E402

L = 2 ** 252 + 27742317777372353535851937790883648493
R = (1 << 256) % L
KS, WORKERS = (2, 4, 8, 16), (2, 4, 8)


def fmt(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} - {max(xs):.3f})" if xs else "-"


def points_of(proof, nrx, nry):
    """(rx, ry) of a proof as Montgomery words: they are its last two vectors (u64 count, 32 canonical bytes each)"""
    o = len(proof) - (8 + 32 * nry) - 32 * nrx
    words = lambda b, n: np.frombuffer(b"".join((int.from_bytes(b[32 * i:32 * i + 32], "little") * R % L).to_bytes(32, "little") for i in range(n)), dtype=np.uint8).reshape(n, 32)
    return words(proof[o:o + 32 * nrx], nrx), words(proof[o + 32 * nrx + 8:], nry)


def single_eval_ms(verify_one):
    oa.stats_enable(True)
    verify_one()
    s = oa.stats_read()
    oa.stats_enable(False)
    return sum(s[k][1] for k in ("eq", "spmv", "reduce"))


def wall(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lgs", default="16,20"); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if oa.device_count() < 1:
        raise SystemExit("verify_many_probe: no MI355X visible")
    label = b"verify many probe"
    dev = ["| constraints | instance | layout | K | batched evaluation, ms | single evaluation, ms | K x single, ms | batched / (K x single) |", "|---|---|---|---|---|---|---|---|"]
    host = ["| constraints | instance | K | workers T | verify_many(T), ms | K sequential verify, ms | K verify from T caller threads, ms |", "|---|---|---|---|---|---|---|"]
    for lg in [int(x) for x in a.lgs.split(",")]:
        for name, make in (("uniform", lambda n: oa.synth_r1cs(n, 10, 1)), ("compiler-like", lambda n: oa.synth_r1cs_compiler_like(n, 10, 5))):
            r = make(1 << lg)
            inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
            gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
            inputs = oa.InputsAssignment.new(r["inputs"])
            wit = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), inputs)
            proofs = [oa.NIZK.prove(inst, wit, inputs, gens, label, bytes([s]) * 32) for s in range(1, max(KS) + 1)]
            nc, nv, _ = inst.dims
            nrx, nry = nc.bit_length() - 1, (2 * nv).bit_length() - 1
            info = inst.device_info()
            layout = ("quad" if info["quad"] else "lane") + (", codes" if info["use_small"] else "") + (", %d long rows" % info["n_heavy"] if info["n_heavy"] else "")
            pts = [points_of(p.bytes, nrx, nry) for p in proofs]
            one = lambda k=0: proofs[k].verify(inst, inputs, gens, label)
            for _ in range(a.warmup + 1):
                one()
            single = [single_eval_ms(one) for _ in range(a.reps)]
            for K in KS:
                rx, ry = np.stack([p[0] for p in pts[:K]]), np.stack([p[1] for p in pts[:K]])
                for _ in range(a.warmup):
                    oa.kernels.instance_evaluate(inst, rx, ry)
                batched = [oa.kernels.instance_evaluate(inst, rx, ry)[1] for _ in range(a.reps)]
                ratio = statistics.median(batched) / (K * statistics.median(single))
                dev.append(f"| 2^{lg} | {name} | {layout} | {K} | {fmt(batched)} | {fmt(single)} | {K * statistics.median(single):.3f} ({K * min(single):.3f} - {K * max(single):.3f}) | {ratio:.2f} |")
                print(dev[-1], flush=True)

                def sequential():
                    for k in range(K):
                        one(k)

                def threaded(T):
                    def run(t):
                        for k in range(t, K, T):
                            one(k)
                    th = [threading.Thread(target=run, args=(t,)) for t in range(T)]
                    for t in th:
                        t.start()
                    for t in th:
                        t.join()

                for T in WORKERS:
                    many = lambda: oa.NIZK.verify_many(inst, proofs[:K], inputs, gens, label, threads=T)
                    assert many() == [0] * K
                    for _ in range(a.warmup):
                        sequential(); threaded(T)
                    m, s, c = [], [], []
                    for _ in range(a.reps):
                        m.append(wall(many)); s.append(wall(sequential)); c.append(wall(lambda: threaded(T)))
                    host.append(f"| 2^{lg} | {name} | {K} | {T} | {fmt(m)} | {fmt(s)} | {fmt(c)} |")
                    print(host[-1], flush=True)
            del wit, inst, gens
    text = "\n".join(["## (i) Device time of the evaluation", "", *dev, "", "## (ii) Wall time of the verification", "", *host, ""])
    print(text)
    if a.out:                                                  # the two tables alone: profiles/verify_many.md quotes them beside what was decided from them
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
