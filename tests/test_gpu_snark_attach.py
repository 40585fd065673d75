"""SNARK mode across processes, on the GPU: the address / timestamp kernels of the dense representation against the sequential scan that
defines them, a commitment read back from bytes completed with `attach` and proving byte-identically, `attach(verify=True)` refusing another
instance, the host-scan switch, and the three `spzk` roles as three processes.

Every GPU step is a child process of its own with a time limit of its own (tests/snark_attach_worker.py, or spzk itself); after a step
that ended in a fault, an abort or its time limit, no further step of this module is started."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import otti_amd as oa

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "snark_attach_worker.py")
SPZK = os.path.join(os.path.dirname(HERE), "otti_amd", "spzk")
_stopped = []                                                    # why no further GPU step is started


def _step(cmd, limit, env=None):
    if _stopped:
        pytest.fail(f"not started: an earlier GPU step of this module {_stopped[0]}")
    e = dict(os.environ); e.update(env or {})
    try:
        res = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as ex:
        _stopped.append(f"ran into its time limit of {limit} s: {' '.join(cmd[-3:])}")
        pytest.fail(f"time limit: {cmd}\n{ex.stdout}\n{ex.stderr}")
    if res.returncode < 0 or res.returncode in (124, 134, 137, 139):
        _stopped.append(f"ended with status {res.returncode}: {' '.join(cmd[-3:])}")
    return res


def _worker(args, limit=300, env=None):
    res = _step([sys.executable, WORKER] + [str(a) for a in args], limit, env)
    assert res.returncode == 0 and res.stdout.strip().splitlines()[-1].startswith("OK"), res.stdout + res.stderr
    return res.stdout


def _digests(out):
    return [ln for ln in out.splitlines() if ln.startswith("DIGEST")][-1].split()[1:]


@pytest.mark.parametrize("case", ["uniform", "one_address_zero", "one_address_nonzero", "ascending", "descending", "runs", "two_alternating", "shared_counter",
                                  "all_padding", "real_then_padding", "smallest", "N_above_M", "N_below_M", "M_not_a_power_of_two", "constant_column_2p20"])
def test_addr_timestamps_equal_the_sequential_scan(case):
    """kernels.addr_timestamps == the walk `read_ts[k][i] = audit[addr[k][i]]++` over one shared counter array (the worker's sequential_scan),
    element for element, on every distribution the kernel must not care about, and again when the call is repeated"""
    _worker(["kernel", case])


@pytest.mark.parametrize("lg,kind", [(12, "uniform"), (12, "compiler"), (16, "uniform"), (16, "compiler")])
def test_attached_commitment_proves_byte_identically(lg, kind):
    """from_bytes(comm.bytes).attach(inst, gens), then SNARK.prove: the encoder's proof, byte for byte (the worker asserts it, and that the
    oracle's verifier and a verifier with generators made from `dims` accept); for the uniform instances also the oracle's committed digests"""
    comm_sha, proof_sha = _digests(_worker(["attach", lg, kind], limit=600))
    if kind == "uniform":
        g = {e["n"]: e for e in json.load(open(os.path.join(HERE, "golden", "snark_proofs.json")))}[1 << lg]
        assert comm_sha == g["commitment_sha256"] and proof_sha == g["proof_sha256"]


@pytest.mark.parametrize("variant", ["coefficient", "column"])
def test_attach_verify_refuses_another_instance_and_trust_gives_a_rejected_proof(variant):
    _worker(["wrong", variant])


@pytest.mark.parametrize("lg", [12, 16])
def test_encode_bytes_do_not_depend_on_where_the_scans_run(lg):
    """OTTI_DECOMM_HOST=1 (the sequential host scans) and the device kernels give the same computation commitment; each in a fresh process"""
    dev = _digests(_worker(["encode", lg], env={"OTTI_DECOMM_HOST": "0"}))
    host = _digests(_worker(["encode", lg], env={"OTTI_DECOMM_HOST": "1"}))
    assert dev == host


def test_spzk_encode_prove_verify_as_three_processes(tmp_path):
    """encode -> prove --comm-in -> verify --comm-in --proof-in; the proof file equals the one the all-in-one `spzk verify` writes with the same seed"""
    r = oa.synth_r1cs_compiler_like(1 << 12, 5, 11)
    pre = str(tmp_path / "c"); files = [pre + ".zkif", pre + ".inp.zkif", pre + ".wit.zkif"]
    oa.zkif_write(r, *files)
    comm, proof, proof_one = pre + ".comm", pre + ".proof", pre + ".one.proof"
    res = _step([SPZK, "encode", files[0], files[1], "--comm-out", comm], 300)
    assert res.returncode == 0 and "SNARK::encode" in res.stdout, res.stdout + res.stderr
    res = _step([SPZK, "prove", *files, "--comm-in", comm, "--proof-out", proof, "--seed", "2a" * 32, "--verify-comm", "--check"], 300)
    assert res.returncode == 0 and "Proof written" in res.stdout and "attach" in res.stdout, res.stdout + res.stderr
    res = _step([SPZK, "verify", files[1], "--comm-in", comm, "--proof-in", proof], 300)
    assert res.returncode == 0 and "Verification successful" in res.stdout, res.stdout + res.stderr
    res = _step([SPZK, "verify", *files, "--seed", "2a" * 32, "--proof-out", proof_one], 300)
    assert res.returncode == 0 and "Verification successful" in res.stdout, res.stdout + res.stderr
    assert open(proof, "rb").read() == open(proof_one, "rb").read()
    res = _step([SPZK, "prove", *files, "--proof-out", pre + ".self.proof", "--seed", "2a" * 32], 300)        # no --comm-in: encodes itself
    assert res.returncode == 0 and hashlib.sha256(open(pre + ".self.proof", "rb").read()).digest() == hashlib.sha256(open(proof, "rb").read()).digest()
    other = oa.synth_r1cs(1 << 10, 5, 3)                                                                        # a circuit of other dimensions
    opre = str(tmp_path / "o"); oa.zkif_write(other, opre + ".zkif", opre + ".inp.zkif", opre + ".wit.zkif")
    res = _step([SPZK, "prove", opre + ".zkif", opre + ".inp.zkif", opre + ".wit.zkif", "--comm-in", comm, "--proof-out", opre + ".proof"], 300)
    assert res.returncode == 1 and "other dimensions" in res.stderr, res.stdout + res.stderr
