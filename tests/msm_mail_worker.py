"""Worker of tests/test_gpu_msm_small_mail.py and tests/test_gpu_msm_edges.py: in a fresh process (OTTI_SMALL_HOST_SUM is read once per process), either
  msm   — one- and two-row fixed-base sums of the latency-bound kind over several row lengths: prints "MSM <L> <lgV> <hex of the points>"
  edges — tests/test_gpu_msm_edges.py small_sum_lines(): the c = 8 digit rows and the one- and two-row shape jobs through oa.kernels.msm_job
          (OTTI_MSM_WINDOW=8 comes with the environment): prints "EDGE <name> <fuse> <hex of the points>"
  nizk <lg> — the committed golden NIZK instance of 2^lg constraints: prints "DIGEST <sha256 of the proof>"."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import otti_amd as oa  # noqa: E402
import orc  # noqa: E402

SHAPES = [(1, 2), (2, 2), (1, 4), (2, 6), (2, 8), (1, 10), (2, 10), (1, 12), (2, 12), (2, 14)]

if sys.argv[1] == "msm":
    rng = np.random.default_rng(20261016)
    for L, lgV in SHAPES:
        V = 1 << lgV
        gens = oa.NIZKGens.new(V, V, 1)
        R = orc.OGens(V, V, 1).R
        Z, bl = orc.rand_fr(rng, L * R), orc.rand_fr(rng, L)
        out, _ = oa.kernels.msm_rows(gens, Z, L, R, bl)
        print("MSM", L, lgV, np.asarray(out).tobytes().hex(), flush=True)
elif sys.argv[1] == "edges":
    from test_gpu_msm_edges import small_sum_lines  # noqa: E402
    for ln in small_sum_lines():
        print("EDGE", ln, flush=True)
else:
    n = 1 << int(sys.argv[2])
    g = [x for x in json.load(open(os.path.join(HERE, "golden", "proofs.json"))) if x["n"] == n][0]
    r = oa.synth_r1cs(g["n"], g["num_inputs"], g["instance_seed"])
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    p = oa.NIZK.prove(inst, oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"]), gens, g["label"].encode(), bytes.fromhex(g["tape_seed"]))
    q = oa.NIZK.prove(inst, oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"]), gens, g["label"].encode(), bytes.fromhex(g["tape_seed"]))
    assert p.bytes == q.bytes
    print("DIGEST", hashlib.sha256(p.bytes).hexdigest(), flush=True)
