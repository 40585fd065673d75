"""Witness.from_tensor: a torch tensor computed on torch's default stream or on a non-default one becomes the resident witness without the caller synchronising.

torch has to bring the GPU up before libottispartan.so is loaded, and this pytest process has loaded the library long since, so the work
happens in ONE fresh child process (witness_tensor_worker.py); the parent compares the digests it prints with the CPU oracle's proof of the
same circuit and assignment."""
import hashlib
import os
import subprocess
import sys

import pytest

import orc
import witness_tensor_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_from_tensor_on_a_torch_stream_gives_the_oracles_proof():
    r = W.tensor_case()
    oinst = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    ogens = orc.OGens(r["num_cons"], r["num_vars"], r["num_inputs"])
    assert oinst.is_sat(r["vars"], r["inputs"])
    want, _ = orc.nizk_prove(oinst, r["vars"], r["inputs"], ogens, W.LABEL, W.SEED)
    want = hashlib.sha256(want).hexdigest()
    res = subprocess.run([sys.executable, os.path.join(HERE, "witness_tensor_worker.py")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"the child ended with status {res.returncode}:\n{res.stdout}\n{res.stderr}"      # nothing further is started after a fault
    lines = res.stdout.split("\n")
    if any(ln.startswith("skip ") for ln in lines):
        pytest.skip(next(ln for ln in lines if ln.startswith("skip ")))
    got = dict(ln.split()[1:] for ln in lines if ln.startswith("digest "))
    assert set(got) == {"default_stream_int64", "strided_int64", "packed_int64", "canonical_uint8"}, res.stdout + res.stderr
    for name, digest in got.items():
        assert digest == want, f"{name}: {digest} is not the oracle's {want}"
