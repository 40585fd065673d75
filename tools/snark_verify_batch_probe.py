"""What verifying K SNARK proofs of one commitment as one randomised batch buys (profiles/snark_verify_batch.md): the figures behind
kSnarkVerifyBatchThreads and the decision to ship without a routing rule (snark.h).  Per size of `--lgs`, on the uniform and the compiler-like
instance, in ONE process, median of `--reps` after `--warmup`, with min - max, for K of `--ks`:

  (i)  wall time of SNARK.verify_batch with 4, 8 and 16 workers beside SNARK.verify_many with 4 and beside K sequential otti_snark_verify calls,
       alternating inside one loop of the same build — the code under test is never its own yardstick;
  (ii) the batch's counters; the device-event time of its sum's launches per pass (decode of the proofs' points, k_gen_runs, k_msm_var_many); the
       wall time of the same batch with OTTI_VERIFY_BATCH_RUNS=0 — every closing equation's n generator terms written out on the host, what the
       batch cost before the runs — and with the sum on the host cores; and a batch whose last proof is bad in a scalar only a deferred
       equation sees (the last 32 bytes of a proof: z2 of the derefs evaluation proof): the first sum, the localisation pass, one single verification.

    python tools/snark_verify_batch_probe.py [--lgs 12,16,20] [--ks 2,4,8,16,64] [--reps 7] [--warmup 1] [--out tables.md]

K proofs are `--distinct` different proofs repeated.  Host-clock timings are around calls that end synchronised.  Generator tables are built with a
4 GiB budget (OTTI_MSM_TABLE_GB, unless set)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OTTI_MSM_TABLE_GB", "4")
import otti_amd as oa  # noqa: E402

WORKERS = (4, 8, 16)


def fmt(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} - {max(xs):.3f})" if xs else "-"


def wall(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3


class env:
    def __init__(self, k, v):
        self.k, self.v = k, v

    def __enter__(self):
        self.old = os.environ.get(self.k); os.environ[self.k] = self.v

    def __exit__(self, *a):
        if self.old is None:
            del os.environ[self.k]
        else:
            os.environ[self.k] = self.old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lgs", default="12,16,20"); ap.add_argument("--ks", default="2,4,8,16,64"); ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=1); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if oa.device_count() < 1:
        raise SystemExit("snark_verify_batch_probe: no MI355X visible")
    KS = [int(x) for x in a.ks.split(",")]
    label = b"snark verify batch probe"
    t1 = ["| constraints | instance | K | " + " | ".join("batch(%d), ms" % T for T in WORKERS) + " | verify_many(4), ms | K sequential verify, ms |", "|---|---|---|" + "---|" * (len(WORKERS) + 2)]
    t2 = ["| constraints | instance | K | equations | points | generator slots | device ms of the sums | batch(4), runs written out, ms | batch(4), host sum, ms | batch(4), one bad proof, ms | its device ms |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for lg in [int(x) for x in a.lgs.split(",")]:
        for name, make in (("uniform", lambda n: oa.synth_r1cs(n, 10, 1)), ("compiler-like", lambda n: oa.synth_r1cs_compiler_like(n, 10, 5))):
            r = make(1 << lg)
            nz = max(r["A"].size, r["B"].size, r["C"].size)
            inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
            gens = oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nz)
            pcomm = oa.ComputationCommitment.encode(inst, gens)
            inputs = oa.InputsAssignment.new(r["inputs"])
            wit = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), inputs)
            distinct = [oa.SNARK.prove(inst, pcomm, wit, None, gens, label, bytes([s]) * 32) for s in range(1, a.distinct + 1)]
            comm = oa.ComputationCommitment.from_bytes(pcomm.bytes)    # the verifier's copy
            del wit, inst, pcomm
            for K in KS:
                proofs = [distinct[k % len(distinct)] for k in range(K)]
                batch = lambda T=4, ps=proofs: oa.SNARK.verify_batch(comm, ps, inputs, gens, label, threads=T, details=True)
                many = lambda: oa.SNARK.verify_many(comm, proofs, inputs, gens, label, threads=4)

                def sequential():
                    for p in proofs:
                        p.verify(comm, inputs, gens, label)

                bad_blob = bytearray(proofs[-1].bytes); bad_blob[-32:] = (5).to_bytes(32, "little")
                bad_list = [p.bytes for p in proofs[:-1]] + [bytes(bad_blob)]
                codes, info = batch()
                assert codes == [0] * K and info["accepted_first_pass"] == 1 and info["on_device"] == 1, (codes, info)
                codes, binfo = batch(4, bad_list)
                assert codes[:-1] == [0] * (K - 1) and codes[-1] != 0 and binfo["singles_rerun"] == 1 and binfo["localise_passes"] == 1, (codes, binfo)
                assert many() == [0] * K
                for _ in range(a.warmup):
                    many(); sequential()
                b = {T: [] for T in WORKERS}; m, s, dev_ms, off_ms, host_ms, bad_ms, bad_dev = [], [], [], [], [], [], []
                for _ in range(a.reps):
                    for T in WORKERS:
                        t0 = time.perf_counter(); i = batch(T)[1]; b[T].append((time.perf_counter() - t0) * 1e3)
                        if T == 4:
                            dev_ms.append(i["sum_ms"])
                    m.append(wall(many)); s.append(wall(sequential))
                    with env("OTTI_VERIFY_BATCH_RUNS", "0"):
                        off_ms.append(wall(batch))
                    with env("OTTI_VERIFY_BATCH_SUM", "host"):
                        host_ms.append(wall(batch))
                    t0 = time.perf_counter(); bi = batch(4, bad_list)[1]; bad_ms.append((time.perf_counter() - t0) * 1e3); bad_dev.append(bi["sum_ms"])
                t1.append(f"| 2^{lg} | {name} | {K} | " + " | ".join(fmt(b[T]) for T in WORKERS) + f" | {fmt(m)} | {fmt(s)} |")
                t2.append(f"| 2^{lg} | {name} | {K} | {info['equations']} | {info['points']} | {info['gen_slots']} | {fmt(dev_ms)} | {fmt(off_ms)} | {fmt(host_ms)} | {fmt(bad_ms)} | {fmt(bad_dev)} |")
                print(t1[-1], flush=True); print(t2[-1], flush=True)
            del gens, comm
    text = "\n".join(["## (i) Wall time of the verification", "", *t1, "", "## (ii) The sums, the runs, and a batch with one bad proof", "", *t2, ""])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
