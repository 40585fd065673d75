"""What proving K witnesses of one instance in one call buys (profiles/prove_many.md).  Per size of `--lgs`, on the uniform and the compiler-like
instance, K = 16 witnesses (the instance's own assignment with its variables rotated by k places: the same value distribution, other vectors), the
default generator window, in ONE process, every shape warmed, the legs alternating inside one loop, median of `--reps` with min - max:

  (1) wall time of otti_nizk_prove_many with 1, 4, 6 and 8 threads — as shipped, and with the front-half rule set aside (OTTI_PROVE_MANY_RULE=0:
      everything joint) at 1 and 4 threads — beside the paths the library had before it: K sequential otti_nizk_prove_resident calls, and the same
      K calls from a caller's own pool of 2, 4, 6 and 8 threads;
  (2) device-event time (kernel class spmv through otti_stats_*) of the many-vector product over the K vectors — interleave included — beside K
      single dev_spmv3 passes (otti_k_multiply_vec on each vector);
  (3) device-event time of the joint row job(s) of otti_k_prove_front (info.front_ms: staging apart) beside K single MSM_KEEP launches
      (otti_k_msm_job's kernel time on each vector's variables).

    python tools/prove_many_probe.py [--lgs 12,16,20] [--reps 5] [--warmup 1] [--out tables.md]

Host-clock timings are around calls that end synchronised.  The witnesses of (1) keep neither rows nor products."""
import argparse
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import otti_amd as oa  # noqa: E402

K = 16
MANY_T, POOL_T, JOINT_T = (1, 4, 6, 8), (2, 4, 6, 8), (1, 4)


def fmt(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} - {max(xs):.3f})" if xs else "-"


def wall(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3


def spmv_ms(f):
    oa.stats_enable(True, only="spmv")
    f()
    ms = oa.stats_read()["spmv"][1]
    oa.stats_enable(False)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lgs", default="12,16,20"); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if oa.device_count() < 1:
        raise SystemExit("prove_many_probe: no MI355X visible")
    label = b"prove many probe"
    seeds = [bytes([s + 1]) * 32 for s in range(K)]
    t_wall = ["| constraints | instance | prove_many, threads 1 / 4 / 6 / 8, ms | the same with everything joint (OTTI_PROVE_MANY_RULE=0), threads 1 / 4, ms | K sequential prove_resident, ms | caller's pool of 2 / 4 / 6 / 8 threads, ms |", "|---|---|---|---|---|---|"]
    t_spmv = ["| constraints | instance | layout | many-vector product of 16, ms | 16 single passes, ms | many / singles |", "|---|---|---|---|---|---|"]
    t_rows = ["| constraints | instance | joint job(s): kernel | joint, ms | staging, ms | 16 single MSM_KEEP launches, ms | joint / singles |", "|---|---|---|---|---|---|---|"]
    for lg in [int(x) for x in a.lgs.split(",")]:
        for name, make in (("uniform", lambda n: oa.synth_r1cs(n, 10, 1)), ("compiler-like", lambda n: oa.synth_r1cs_compiler_like(n, 10, 5))):
            r = make(1 << lg)
            inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
            gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
            inputs = oa.InputsAssignment.new(r["inputs"])
            nc, nv, ni = inst.dims
            vars_ = np.asarray(r["vars"], dtype=np.uint8)
            rolled = [np.ascontiguousarray(np.roll(vars_, k, axis=0)) for k in range(K)]
            wits = [oa.Witness(inst, oa.VarsAssignment.new(v), inputs) for v in rolled]
            info = inst.device_info()
            layout = ("quad" if info["quad"] else "lane") + (", codes" if info["use_small"] else "") + (", %d long rows" % info["n_heavy"] if info["n_heavy"] else "")
            small = wits[0].info[2] > 0.25

            # ---- (1) wall time
            single = lambda k: oa.NIZK.prove(inst, wits[k], None, gens, label, seeds[k])     # noqa: E731
            want = [single(k).bytes for k in range(K)]

            def sequential():
                for k in range(K):
                    single(k)

            def pool(T):
                def run(t):
                    for k in range(t, K, T):
                        single(k)
                th = [threading.Thread(target=run, args=(t,)) for t in range(T)]
                for t in th:
                    t.start()
                for t in th:
                    t.join()

            many = lambda T: oa.NIZK.prove_many(inst, wits, gens, label, seeds=seeds, threads=T)   # noqa: E731
            assert [p.bytes for p in many(4)] == want
            for _ in range(a.warmup):
                sequential()
                for T in MANY_T:
                    many(T)
                os.environ["OTTI_PROVE_MANY_RULE"] = "0"
                for T in JOINT_T:
                    many(T)
                del os.environ["OTTI_PROVE_MANY_RULE"]
                for T in POOL_T:
                    pool(T)
            m, s, c, j = {T: [] for T in MANY_T}, [], {T: [] for T in POOL_T}, {T: [] for T in JOINT_T}
            for _ in range(a.reps):
                s.append(wall(sequential))
                for T in MANY_T:
                    m[T].append(wall(lambda: many(T)))
                os.environ["OTTI_PROVE_MANY_RULE"] = "0"          # the front-half rule set aside: everything the plan allows is joint
                for T in JOINT_T:
                    j[T].append(wall(lambda: many(T)))
                del os.environ["OTTI_PROVE_MANY_RULE"]
                for T in POOL_T:
                    c[T].append(wall(lambda: pool(T)))
            t_wall.append(f"| 2^{lg} | {name} | {' / '.join(fmt(m[T]) for T in MANY_T)} | {' / '.join(fmt(j[T]) for T in JOINT_T)} | {fmt(s)} | {' / '.join(fmt(c[T]) for T in POOL_T)} |")
            print(t_wall[-1], flush=True)
            del wits

            # ---- (2), (3) device time on staged vectors
            tail = np.zeros((nv, 32), dtype=np.uint8)
            tail[0, 0] = 1
            tail[1:1 + ni] = np.asarray(r["inputs"], dtype=np.uint8)
            zs = [oa.kernels.from_canonical(np.concatenate([v, np.zeros((nv - v.shape[0], 32), dtype=np.uint8), tail])) for v in rolled]
            os.environ["OTTI_PROVE_MANY_RULE"] = "0"              # (2), (3) measure the joint passes themselves, wherever the rule would put them
            ell = nv.bit_length() - 1
            Lrows = 1 << (ell // 2)
            for _ in range(a.warmup):
                oa.kernels.multiply_vec_many(inst, zs); oa.kernels.multiply_vec(inst, zs[0])
                oa.kernels.prove_front(inst, gens, zs, [small] * K); oa.kernels.msm_job(gens, Lrows, dense=zs[0][:nv], mode="keep", sparse=int(small))
            mv, sv, jr, st, sr, kern = [], [], [], [], [], None
            for _ in range(a.reps):
                mv.append(spmv_ms(lambda: oa.kernels.multiply_vec_many(inst, zs)))
                sv.append(sum(spmv_ms(lambda z=z: oa.kernels.multiply_vec(inst, z)) for z in zs))
                fi = oa.kernels.prove_front(inst, gens, zs, [small] * K)[4]
                assert fi["rows_from_front"] == K, fi
                jr.append(fi["front_ms"]["row_sums"]); st.append(fi["front_ms"]["staging"]); kern = " + ".join(fi["row_kernel"])
                sr.append(sum(oa.kernels.msm_job(gens, Lrows, dense=z[:nv], mode="keep", sparse=int(small))[2] for z in zs))
            t_spmv.append(f"| 2^{lg} | {name} | {layout} | {fmt(mv)} | {fmt(sv)} | {statistics.median(mv) / statistics.median(sv):.2f} |")
            t_rows.append(f"| 2^{lg} | {name} | {kern} | {fmt(jr)} | {fmt(st)} | {fmt(sr)} | {statistics.median(jr) / statistics.median(sr):.2f} |")
            print(t_spmv[-1]); print(t_rows[-1], flush=True)
            del os.environ["OTTI_PROVE_MANY_RULE"]
            del zs, inst, gens
    text = "\n".join(["## (1) Wall time of 16 proofs", "", *t_wall, "", "## (2) Device time of the products", "", *t_spmv, "", "## (3) Device time of the row sums", "", *t_rows, ""])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
