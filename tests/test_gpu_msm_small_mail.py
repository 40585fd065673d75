"""The latency-bound fixed-base MSMs (k_msm_small, one or two rows) hand every workgroup's chunk sum to the host, which adds them
(DevCtx::msm_host_sum); OTTI_SMALL_HOST_SUM=0 keeps the older form, where the last workgroup to arrive adds them on the device.  Both
must give the oracle's points at every shape — one chunk, power-of-two and other chunk counts, one and two rows — and whole proofs
with either must be the committed oracle digests."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import otti_amd as oa
import orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _worker(args, env, script="msm_mail_worker.py", with_stderr=False):
    e = dict(os.environ); e.update(env)
    res = subprocess.run([sys.executable, os.path.join(HERE, script)] + args, env=e, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    return (res.stdout, res.stderr) if with_stderr else res.stdout


@pytest.mark.parametrize("L,lgV", [(1, 2), (2, 2), (1, 6), (2, 6), (2, 8), (1, 10), (2, 12), (1, 14), (2, 14)])
def test_small_msm_rows_equal_oracle(rng, L, lgV):
    V = 1 << lgV
    gens, og = oa.NIZKGens.new(V, V, 1), orc.OGens(V, V, 1)
    R = og.R
    Z, bl = orc.rand_fr(rng, L * R), orc.rand_fr(rng, L)
    out, _ = oa.kernels.msm_rows(gens, Z, L, R, bl)
    assert np.array_equal(np.asarray(out), orc.commit_rows(og, Z, L, R, bl))


def test_host_sum_equals_device_sum():
    """the same shapes through both forms, each in a process of its own; the first against the oracle as well"""
    on = [ln.split() for ln in _worker(["msm"], {"OTTI_SMALL_HOST_SUM": "1"}).splitlines() if ln.startswith("MSM")]
    off = [ln.split() for ln in _worker(["msm"], {"OTTI_SMALL_HOST_SUM": "0"}).splitlines() if ln.startswith("MSM")]
    assert len(on) == len(off) >= 10 and on == off
    # the phase stamps name the form each launch took: the switch really selects the host sum (and its absence the device sum)
    out_on, err_on = _worker(["msm"], {"OTTI_SMALL_HOST_SUM": "1", "OTTI_MSM_STAMPS": "1"}, with_stderr=True)
    out_off, err_off = _worker(["msm"], {"OTTI_SMALL_HOST_SUM": "0", "OTTI_MSM_STAMPS": "1"}, with_stderr=True)
    stamped_on = [ln for ln in err_on.splitlines() if "k_msm_small" in ln]
    stamped_off = [ln for ln in err_off.splitlines() if "k_msm_small" in ln]
    assert stamped_on and all("host-sum:" in ln for ln in stamped_on), err_on[-2000:]
    assert stamped_off and not any("host-sum:" in ln for ln in stamped_off), err_off[-2000:]
    assert [ln.split() for ln in out_on.splitlines() if ln.startswith("MSM")] == on
    rng = np.random.default_rng(20261016)
    for (_, L, lgV, hx) in on[:6]:
        L, V = int(L), 1 << int(lgV)
        og = orc.OGens(V, V, 1)
        Z, bl = orc.rand_fr(rng, L * og.R), orc.rand_fr(rng, L)
        assert bytes.fromhex(hx) == orc.commit_rows(og, Z, L, og.R, bl).tobytes(), (L, lgV)


@pytest.mark.parametrize("lg,env", [(10, {"OTTI_SMALL_HOST_SUM": "1"}), (10, {"OTTI_SMALL_HOST_SUM": "0"}),
                                    (16, {"OTTI_SMALL_HOST_SUM": "1"}), (16, {"OTTI_SMALL_HOST_SUM": "0"}),
                                    (16, {"OTTI_HOST_THREADS": "1"}), (20, {"OTTI_HOST_THREADS": "16"})])
def test_nizk_proof_with_either_sum_is_the_golden_digest(lg, env):
    """OTTI_HOST_THREADS: the host sum without helpers, and at 2^20 (Cx / delta: 94 chunks in one row, bullet rounds: 2 x 52) with more
    helpers than it splits a launch over"""
    g = [x for x in json.load(open(os.path.join(HERE, "golden", "proofs.json"))) if x["n"] == 1 << lg][0]
    line = [ln for ln in _worker(["nizk", str(lg)], env).splitlines() if ln.startswith("DIGEST")][-1].split()
    assert line[1] == g["proof_sha256"]


@pytest.mark.parametrize("switch", ["1", "0"])
def test_snark_proof_with_either_sum_is_the_golden_digest(switch):
    g = {x["n"]: x for x in json.load(open(os.path.join(HERE, "golden", "snark_proofs.json")))}[1 << 12]
    line = [ln for ln in _worker(["12"], {"OTTI_SMALL_HOST_SUM": switch}, "snark_tail_worker.py").splitlines() if ln.startswith("DIGEST")][-1].split()
    assert line[1] == g["commitment_sha256"] and line[2] == g["proof_sha256"]
