"""What verifying K SNARK proofs of one commitment in one call buys (profiles/snark_verify_many.md): the figures behind kSnarkVerifyManyThreads,
kSnarkVerifyManyChunk and kRowSumDeviceMin (snark.h).  Per size of `--lgs`, on the uniform and the compiler-like instance, in ONE process, median of
`--reps` after `--warmup`, with min - max:

  (i)  device time (otti_stats_read: the decode and msm_var classes) of ONE batched pass of J = 2, 4, 8, 16 jobs through otti_k_row_sum_many, at the
       instance's comm_ops size (J jobs over one shared set, as a pass over the commitment's points is — there the set is even decoded ahead of
       time) and at its comm_derefs size (J jobs over J sets of their own), beside J x the decode + msm_var time of otti_k_row_sum at that size on
       the same build — the code under test is never its own yardstick;
  (ii) wall time of SNARK.verify_many with T = 2, 4 and 8 workers for K = 2, 4, 8, 16 proofs beside K sequential otti_snark_verify calls and beside
       the same K calls issued from T caller threads (the best a caller can do without the new entry), the three alternating inside one loop.

    python tools/snark_verify_many_probe.py [--lgs 16,20] [--reps 7] [--warmup 1] [--out tables.md]

Host-clock timings are around calls that end synchronised.  Generator tables are built with a 4 GiB budget (OTTI_MSM_TABLE_GB, unless set)."""
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

KS, WORKERS = (2, 4, 8, 16), (2, 4, 8)


def fmt(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} - {max(xs):.3f})" if xs else "-"


def wall(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3


def device_ms(f):
    """the decode + msm_var time of one call"""
    oa.stats_enable(True)
    f()
    s = oa.stats_read()
    oa.stats_enable(False)
    return s["decode"][1] + s["msm_var"][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lgs", default="16,20"); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if oa.device_count() < 1:
        raise SystemExit("snark_verify_many_probe: no MI355X visible")
    label = b"snark verify many probe"
    rng = np.random.default_rng(1)
    dev = ["| constraints | instance | points n | shape | J | batched pass, ms | single row sum, ms | J x single, ms | batched / (J x single) |", "|---|---|---|---|---|---|---|---|---|"]
    host = ["| constraints | instance | K | workers T | verify_many(T), ms | K sequential verify, ms | K verify from T caller threads, ms |", "|---|---|---|---|---|---|---|"]
    for lg in [int(x) for x in a.lgs.split(",")]:
        for name, make in (("uniform", lambda n: oa.synth_r1cs(n, 10, 1)), ("compiler-like", lambda n: oa.synth_r1cs_compiler_like(n, 10, 5))):
            r = make(1 << lg)
            nz = max(r["A"].size, r["B"].size, r["C"].size)
            inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
            gens = oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nz)
            pcomm = oa.ComputationCommitment.encode(inst, gens)
            inputs = oa.InputsAssignment.new(r["inputs"])
            wit = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), inputs)
            proofs = [oa.SNARK.prove(inst, pcomm, wit, None, gens, label, bytes([s]) * 32) for s in range(1, max(KS) + 1)]
            cb = pcomm.bytes
            comm = oa.ComputationCommitment.from_bytes(cb)    # the verifier's copy
            n_ops = int.from_bytes(cb[48:56], "little")
            lgnz = max(1, (max(nz, 2) - 1).bit_length())
            n_derefs = 1 << ((lgnz + 3) // 2)                  # snark_gens_new: derefs has lgnz + 3 variables, L = 2^(m / 2) rows
            del wit, inst, pcomm
            # ---- (i) one batched pass against J single row sums, on points that decode (the generator stream) and uniform scalars
            pts = gens.points("eval")
            for n, shape in ((n_ops, "one shared set (ops)"), (n_derefs, "a set per job (derefs)")):
                if n < 256 or n > pts.shape[0]:
                    continue                                   # the single row sum refuses fewer than 256 points: nothing to compare with
                C = pts[:n]
                sc = lambda: oa.fr_from_ints([int.from_bytes(rng.bytes(64), "little") % oa.L_ORDER for _ in range(n)])
                s0 = sc()
                for _ in range(a.warmup + 1):
                    oa.kernels.row_sum(C, s0)
                single = [device_ms(lambda: oa.kernels.row_sum(C, s0)) for _ in range(a.reps)]
                for J in KS:
                    ss = [sc() for _ in range(J)]
                    sets, jobs = ([C], [(0, s) for s in ss]) if shape.startswith("one") else ([C] * J, [(j, s) for j, s in enumerate(ss)])
                    for _ in range(a.warmup):
                        oa.kernels.row_sum_many(sets, jobs)
                    batched = [device_ms(lambda: oa.kernels.row_sum_many(sets, jobs)) for _ in range(a.reps)]
                    ratio = statistics.median(batched) / (J * statistics.median(single))
                    dev.append(f"| 2^{lg} | {name} | {n} | {shape} | {J} | {fmt(batched)} | {fmt(single)} | {J * statistics.median(single):.3f} ({J * min(single):.3f} - {J * max(single):.3f}) | {ratio:.2f} |")
                    print(dev[-1], flush=True)
            # ---- (ii) wall time of the whole verification
            one = lambda k=0: proofs[k].verify(comm, inputs, gens, label)
            for _ in range(a.warmup + 1):
                one()
            for K in KS:
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
                    many = lambda: oa.SNARK.verify_many(comm, proofs[:K], inputs, gens, label, threads=T)
                    assert many() == [0] * K
                    for _ in range(a.warmup):
                        sequential(); threaded(T)
                    m, s, c = [], [], []
                    for _ in range(a.reps):
                        m.append(wall(many)); s.append(wall(sequential)); c.append(wall(lambda: threaded(T)))
                    host.append(f"| 2^{lg} | {name} | {K} | {T} | {fmt(m)} | {fmt(s)} | {fmt(c)} |")
                    print(host[-1], flush=True)
            del gens, comm
    text = "\n".join(["## (i) Device time of one batched pass", "", *dev, "", "## (ii) Wall time of the verification", "", *host, ""])
    print(text)
    if a.out:                                                  # the two tables alone: profiles/snark_verify_many.md quotes them beside what was decided from them
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
