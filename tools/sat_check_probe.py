"""The satisfiability pass against multiply_vec (profiles/sat_check.md): kernel time of otti_witness_check_sat and of otti_k_multiply_vec on the
same instance, launches alternating, median and spread of `--reps` after `--warmup`; the host's otti_instance_is_sat wall time; the whole
otti_witness_check_sat call for a satisfied witness and for one failing row.

    python tools/sat_check_probe.py [--lg 20] [--reps 20] [--warmup 3]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import otti_amd as oa  # noqa: E402


def z_mont(r):
    """z = vars || 1 || inputs || 0.. in Montgomery form (from_canonical on the device)"""
    n = r["num_vars"]
    z = np.zeros((2 * n, 32), dtype=np.uint8)
    z[:n] = r["vars"]; z[n, 0] = 1; z[n + 1:n + 1 + r["num_inputs"]] = r["inputs"]
    return oa.kernels.from_canonical(z)


def wall_ms(f, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=20); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if oa.device_count() < 1:
        raise SystemExit("sat_check_probe: no MI355X visible")
    n = 1 << a.lg
    for name, gen in (("uniform", oa.synth_r1cs), ("compiler_like", oa.synth_r1cs_compiler_like)):
        r = gen(n, 10, 1)
        inst = oa.Instance.new(n, n, 10, r["A"], r["B"], r["C"]); inst.prepare_device()
        v, i = oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"])
        wit = oa.Witness(inst, v, i)
        z = z_mont(r)
        nnz = sum(r[k].size for k in "ABC")
        mv, cs = [], []
        for k in range(a.warmup + a.reps):
            ms = oa.kernels.multiply_vec(inst, z)[3]
            rep = wit.check_sat(inst)
            assert rep.n_unsat == 0
            if k >= a.warmup:
                mv.append(ms); cs.append(rep.kernel_ms)
        s = max(mv) - min(mv)
        print(f"{name} 2^{a.lg}: nnz={nnz}  multiply_vec kernel_ms median {statistics.median(mv):.4f} min {min(mv):.4f} max {max(mv):.4f} spread {s:.4f} | "
              f"check_sat kernel_ms median {statistics.median(cs):.4f} min {min(cs):.4f} max {max(cs):.4f} | "
              f"target check_sat <= multiply_vec + spread = {statistics.median(mv) + s:.4f}: {'met' if statistics.median(cs) <= statistics.median(mv) + s else 'MISSED'}")
        e2e = wall_ms(lambda: wit.check_sat(inst), a.reps)
        bad = r["vars"].copy(); bad[12345 % n, 0] ^= 1
        wit_bad = oa.Witness(inst, oa.VarsAssignment.new(bad), i)
        rep = wit_bad.check_sat(inst)
        e2e_bad = wall_ms(lambda: wit_bad.check_sat(inst), a.reps)
        e2e_bad_count = wall_ms(lambda: wit_bad.check_sat(inst, max_rows=0), a.reps)
        host = wall_ms(lambda: inst.is_sat(v, i), 3)
        print(f"{name} 2^{a.lg}: otti_witness_check_sat wall ms, satisfied: median {statistics.median(e2e):.4f} | {rep.n_unsat} failing rows {rep.rows.tolist()} with values: "
              f"median {statistics.median(e2e_bad):.4f} | count alone: median {statistics.median(e2e_bad_count):.4f} | host otti_instance_is_sat wall ms: {min(host):.1f} (best of 3)")
        del wit, wit_bad, inst


if __name__ == "__main__":
    main()
