"""What verifying K proofs of one instance as ONE randomised batch buys (profiles/verify_batch.md): the figures behind kVerifyBatchThreads and the
routing rules of nizk_verify_batch (spartan.h).  Per size of `--lgs`, on the uniform and the compiler-like instance, K = 2, 4, 8, 16, 64 proofs of
one resident witness (one seed each: the points differ), in ONE process, median of `--reps` after `--warmup`, with min - max:

  (i)  wall time of otti_nizk_verify_batch with 4, 8 and 16 workers and the sum on the device, and with the sum on the host cores
       (OTTI_VERIFY_BATCH_SUM=host, 8 workers), beside otti_nizk_verify_many with 4 workers and beside K sequential otti_nizk_verify calls from the
       same build, all alternating inside one loop;
  (ii) what the sum is: distinct points, generator slots, the device-event time of its launches; and the wall time of a batch in which ONE proof
       is bad (a scalar only a deferred equation sees): the first sum, the localisation pass and one single verification.

    python tools/verify_batch_probe.py [--lgs 12,16,20] [--ks 2,4,8,16,64] [--reps 7] [--warmup 1] [--out tables.md]

Host-clock timings are around calls that end synchronised.  The generator table is built with a 4 GiB budget (OTTI_MSM_TABLE_GB, unless set)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OTTI_MSM_TABLE_GB", "4")
os.environ["OTTI_VERIFY_BATCH_RULE"] = "0"                    # the K = 2 rows measure the batch itself, not the path the shipped rule routes them to
import otti_amd as oa  # noqa: E402

WORKERS = (4, 8, 16)


def fmt(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} - {max(xs):.3f})" if xs else "-"


def wall(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3


def deferred_only_mutant(proof, nc, nv):
    """z[0] of the first sum-check's first dot-product proof replaced.  Layout (NizkProof::serialize): comm_vars (u64 count, 32 bytes each), then
    sc1: comm_polys, comm_evals (u64 count, 32 bytes each), proofs (u64 count; each delta, beta, z (u64 count, 32 each), z_delta, z_beta)"""
    ell = nv.bit_length() - 1
    n_rows, nrx = 1 << (ell // 2), nc.bit_length() - 1
    at = 8 + 32 * n_rows + 2 * (8 + 32 * nrx) + 8 + 64 + 8
    assert int.from_bytes(proof[at - 8:at], "little") == 4, "the count in front of z: the offset is right"
    out = bytearray(proof); out[at:at + 32] = (5).to_bytes(32, "little")
    return bytes(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lgs", default="12,16,20"); ap.add_argument("--ks", default="2,4,8,16,64")
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=1); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if oa.device_count() < 1:
        raise SystemExit("verify_batch_probe: no MI355X visible")
    KS = [int(x) for x in a.ks.split(",")]
    label = b"verify batch probe"
    t1 = ["| constraints | instance | K | " + " | ".join("batch(%d), ms" % T for T in WORKERS) + " | batch(8), host sum, ms | verify_many(4), ms | K sequential verify, ms |",
          "|---|---|---|" + "---|" * (len(WORKERS) + 3)]
    t2 = ["| constraints | instance | K | equations | distinct points | generator slots | sum on the device, event ms | batch(4) with one bad proof, ms | its device ms |", "|---|---|---|---|---|---|---|---|---|"]
    for lg in [int(x) for x in a.lgs.split(",")]:
        for name, make in (("uniform", lambda n: oa.synth_r1cs(n, 10, 1)), ("compiler-like", lambda n: oa.synth_r1cs_compiler_like(n, 10, 5))):
            r = make(1 << lg)
            inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
            gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
            inputs = oa.InputsAssignment.new(r["inputs"])
            wit = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), inputs)
            proofs = [oa.NIZK.prove(inst, wit, inputs, gens, label, s.to_bytes(32, "little")).bytes for s in range(1, max(KS) + 1)]
            nc, nv, _ = inst.dims
            one = lambda k=0: oa.NIZK(proofs[k]).verify(inst, inputs, gens, label)
            for _ in range(a.warmup + 1):
                one()
            for K in KS:
                batch = lambda T, **kw: oa.NIZK.verify_batch(inst, proofs[:K], inputs, gens, label, threads=T, **kw)
                many = lambda: oa.NIZK.verify_many(inst, proofs[:K], inputs, gens, label, threads=4)

                def host_sum():
                    os.environ["OTTI_VERIFY_BATCH_SUM"] = "host"
                    try:
                        return batch(8, details=True)
                    finally:
                        del os.environ["OTTI_VERIFY_BATCH_SUM"]

                def sequential():
                    for k in range(K):
                        one(k)

                codes, info = batch(4, details=True)
                assert codes == [0] * K and info["on_device"] == 1 and info["accepted_first_pass"] == 1, info
                codes, hinfo = host_sum()
                assert codes == [0] * K and hinfo["on_device"] == 0 and hinfo["accepted_first_pass"] == 1, hinfo
                assert many() == [0] * K
                bad_list = proofs[:K - 1] + [deferred_only_mutant(proofs[K - 1], nc, nv)]
                with_bad = lambda: oa.NIZK.verify_batch(inst, bad_list, inputs, gens, label, threads=4, details=True)
                codes, binfo = with_bad()
                assert codes[:-1] == [0] * (K - 1) and codes[-1] != 0 and binfo["localise_passes"] == 1 and binfo["singles_rerun"] == 1, (codes, binfo)
                for _ in range(a.warmup):
                    for T in WORKERS:
                        batch(T)
                    host_sum(); many(); sequential(); with_bad()
                b = {T: [] for T in WORKERS}; h, m, s, dev_ms, bad_ms, bad_dev = [], [], [], [], [], []
                for _ in range(a.reps):
                    for T in WORKERS:
                        b[T].append(wall(lambda: batch(T)))
                    h.append(wall(host_sum)); m.append(wall(many)); s.append(wall(sequential))
                    dev_ms.append(batch(4, details=True)[1]["sum_ms"])
                    t0 = time.perf_counter(); bi = with_bad()[1]; bad_ms.append((time.perf_counter() - t0) * 1e3); bad_dev.append(bi["sum_ms"])
                t1.append(f"| 2^{lg} | {name} | {K} | " + " | ".join(fmt(b[T]) for T in WORKERS) + f" | {fmt(h)} | {fmt(m)} | {fmt(s)} |")
                t2.append(f"| 2^{lg} | {name} | {K} | {info['equations']} | {info['points']} | {info['gen_slots']} | {fmt(dev_ms)} | {fmt(bad_ms)} | {fmt(bad_dev)} |")
                print(t1[-1], flush=True); print(t2[-1], flush=True)
            del wit, inst, gens
    text = "\n".join(["## (i) Wall time of the verification", "", *t1, "", "## (ii) The sum, and a batch with one bad proof", "", *t2, ""])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
