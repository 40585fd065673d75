"""Timing probe of the decommitment build (profiles/snark_attach.md).  One measurement per process:

  python tools/attach_probe.py encode <lg> <uniform|compiler>     one fresh SNARK::encode; run with OTTI_TRACE=1 for the laps on stderr
                                                                  (OTTI_DECOMM_HOST=1: the sequential host scans, else the device kernels)
  python tools/attach_probe.py attach <lg> <uniform|compiler>     wall time of attach, attach(verify=True) and a second encode (window table built)
  python tools/attach_probe.py kernel <lg>                        kernel time of otti_k_addr_timestamps alone on one side of the uniform instance
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import otti_amd as oa  # noqa: E402


def case(lg, kind):
    r = (oa.synth_r1cs if kind == "uniform" else oa.synth_r1cs_compiler_like)(1 << lg, 10, 1)
    nz = int(max(r["A"].size, r["B"].size, r["C"].size))
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    return r, inst, oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nz)


def main():
    what, lg = sys.argv[1], int(sys.argv[2])
    if what == "kernel":
        r, _, _ = case(lg, "uniform")
        N = 1 << lg
        a = np.zeros((3, N), dtype=np.uint32)
        for k, m in enumerate("ABC"):
            a[k, : r[m].size] = r[m]["col"]
        times = [oa.kernels.addr_timestamps(a, 2 * N)[2] for _ in range(6)]
        print(f"PROBE kernel lg={lg} one side, kernel_ms (6 calls, first is cold): " + " ".join(f"{t:.3f}" for t in times), flush=True)
        return
    kind = sys.argv[3]
    _, inst, gens = case(lg, kind)
    t0 = time.perf_counter(); comm = oa.ComputationCommitment.encode(inst, gens); t_first = time.perf_counter() - t0
    if what == "encode":
        print(f"PROBE encode lg={lg} {kind} host_scans={os.environ.get('OTTI_DECOMM_HOST', '0')} wall_ms={1e3 * t_first:.3f}", flush=True)
        return
    data = comm.bytes
    row = []
    for _ in range(5):
        t0 = time.perf_counter(); oa.ComputationCommitment.encode(inst, gens); t_enc = time.perf_counter() - t0
        c = oa.ComputationCommitment.from_bytes(data)
        t0 = time.perf_counter(); c.attach(inst, gens); t_att = time.perf_counter() - t0
        c = oa.ComputationCommitment.from_bytes(data)
        t0 = time.perf_counter(); c.attach(inst, gens, verify=True); t_ver = time.perf_counter() - t0
        row.append((1e3 * t_enc, 1e3 * t_att, 1e3 * t_ver))
    med = [sorted(x)[len(x) // 2] for x in zip(*row)]
    print(f"PROBE attach lg={lg} {kind}: encode (table built) {med[0]:.3f} ms, attach {med[1]:.3f} ms, attach+verify {med[2]:.3f} ms (medians of 5; all: {row})", flush=True)


if __name__ == "__main__":
    main()
