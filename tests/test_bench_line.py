"""bench.py's N > 1 line must be gradeable before a multi-GPU node shows up: the driver's own launch command rehearsed with two rank
processes (GPU test: both share the box's one card, gloo bookkeeping — OTTI_BENCH_REHEARSE=1), and the rehearsal line kept under
profiles/ checked for the same keys on the CPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_sharded_line(d, world):
    assert d["n_gpus"] == world and d["scaling"] == "strong" and d["unit"] == "constraints/s" and d["value"] > 0
    assert d["equals_oracle_digest"] in (True, None)
    cb = d["cpu_baseline"]
    assert cb and cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] == "port" and cb["proof_equals_gpu_proof"] is True
    rf = d["roofline"]
    assert rf and rf["kernel"] == "msm_rows" and 0 < rf["frac"] < 1 and rf["alu"]["peak_isa"] > rf["alu"]["achieved"] > 0
    tr = d["transports"]
    assert tr and tr["mailbox"]["ms_per_proof"] > 0                      # the mailbox always works; RCCL is timed, or its refusal recorded (two ranks on one card)
    assert ("ms_per_proof" in tr["rccl"]) or tr["rccl"].get("error")
    sw = {k: v for k, v in d["sweep"].items() if k.startswith("2^")}
    assert sw and all(("skipped" in v) or (v["ms_per_proof"] > 0 and v["equals_oracle_digest"] in (True, None)) for v in sw.values())
    assert "sharded over %d GPUs" % world in d["config"]["parallelism"]


def test_committed_two_rank_rehearsal_line_carries_cpu_baseline_transports_and_sweep():
    path = os.path.join(ROOT, "profiles", "r3_bench_rehearse_2ranks_one_gpu.json")
    d = json.load(open(path))
    _check_sharded_line(d, 2)
    assert any(k in d["sweep"] for k in ("2^22", "2^24")), "the rehearsal kept under profiles/ covers north_star's target size"


def test_round4_rehearsal_line_has_the_sharded_snark_figure_and_the_early_scalars():
    d = json.load(open(os.path.join(ROOT, "profiles", "r4_bench_rehearse_2ranks_one_gpu.json")))
    _check_sharded_line(d, 2)
    sn = d["snark"]
    assert sn["scaling"] == "strong" and sn["replicas"]["scaling"] == "weak" and sn["equals_oracle_digest"] is True and sn["proof_sha256"] == sn["replicas"]["proof_sha256"]
    assert d["snark_ms_per_proof"] == sn["ms_per_proof"] and d["ms_per_step_p50"] <= d["ms_per_step_p99"] <= d["ms_per_step_max"]
    assert set(d["prepare_device_breakdown_ms"]) >= {"window_table_allocations", "window_table_upload_and_kernels", "instance_upload_and_csr_build"}


@pytest.mark.gpu
def test_two_rank_rehearsal_of_the_drivers_command(tmp_path):
    env = dict(os.environ); env["OTTI_BENCH_REHEARSE"] = "1"; env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OTTI_BENCH_REHEARSE_SNARK"] = "1"; env["OTTI_MSM_TABLE_GB"] = "16"          # the SNARK replicas leg too; two ranks' window tables on ONE card
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29533",
           os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "3", "--warmup", "1", "--log2-constraints", "18", "--sweep", "16", "--in-flight", "-1"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    _check_sharded_line(d, 2)
    sn = d["snark"]                                                      # SNARK mode at N > 1: ONE proof sharded over the ranks (strong), the replicas figure beside it (weak); digests checked
    assert sn and "error" not in sn and "sharded_error" not in sn and sn["value"] > 0 and sn["scaling"] == "strong" and sn["n_gpus"] == 2 and sn["equals_oracle_digest"] is True, sn
    rp = sn["replicas"]
    assert rp["scaling"] == "weak" and rp["value"] > 0 and rp["proof_sha256"] == sn["proof_sha256"], rp
    assert d["snark_ms_per_proof"] == sn["ms_per_proof"] and d["ms_per_step_p99"] >= d["ms_per_step_p50"] > 0


@pytest.mark.gpu
def test_sharded_bench_path_over_the_real_rccl_backend_with_a_world_of_one(tmp_path):
    """What a one-GPU box can run of the N > 1 path beyond the gloo rehearsal: `backend="nccl"` process group, witness broadcast, the exchange,
    BOTH transports timed (RCCL accepts a communicator of one rank), the sharded sweep — OTTI_FORCE_DIST + OTTI_FORCE_SHARD."""
    env = dict(os.environ)
    env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29547", "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0", "OTTI_FORCE_DIST": "1", "OTTI_FORCE_SHARD": "1"})
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--steps", "3", "--warmup", "1", "--log2-constraints", "16", "--sweep", "14", "--in-flight", "-1",
           "--no-e2e", "--no-snark"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), "rank 0 prints ONE line (RCCL's banner must not reach stdout): %r" % lines[:3]
    d = json.loads(lines[0])
    tr = d["transports"]
    assert tr["mailbox"]["ms_per_proof"] > 0 and tr["rccl"].get("ms_per_proof", 0) > 0, tr
    assert d["cpu_baseline"]["proof_equals_gpu_proof"] is True and d["sweep"]["2^14"]["equals_oracle_digest"] is True
