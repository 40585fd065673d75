"""SNARK mode across processes, the parts that need no GPU: the library's new entry points (dimensions of a parsed commitment, argument checks
of attach before any device is touched, generators made from the commitment's dimensions alone) and `spzk verify <inputs> --comm-in --proof-in`
accepting a commitment and a proof made by the CPU oracle — with no circuit file, no witness and no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import otti_amd as oa
import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SPZK = os.path.join(os.path.dirname(HERE), "otti_amd", "spzk")
LABEL, SEED = b"snark_example", b"\x2a" * 32
BAD_ARG, NO_DEVICE = -21, -20


def _next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


@pytest.fixture(scope="module")
def oracle_case(tmp_path_factory):
    """a 2^9 synthetic instance as zkif files, with the oracle's commitment and proof"""
    r = oa.synth_r1cs(1 << 9, 4, 5)
    nz = int(max(r["A"].size, r["B"].size, r["C"].size))
    d = tmp_path_factory.mktemp("attach")
    pre = str(d / "c"); files = [pre + ".zkif", pre + ".inp.zkif", pre + ".wit.zkif"]
    oa.zkif_write(r, *files)
    oi = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    og = orc.OSnarkGens(r["num_cons"], r["num_vars"], r["num_inputs"], nz)
    oc = orc.OSnarkComm.encode(oi, og)
    proof, _ = orc.snark_prove(oi, oc, r["vars"], r["inputs"], og, LABEL, SEED)
    comm_path, proof_path = pre + ".comm", pre + ".proof"
    open(comm_path, "wb").write(oc.bytes); open(proof_path, "wb").write(proof)
    return dict(r=r, nz=nz, files=files, oi=oi, comm=oc.bytes, proof=proof, comm_path=comm_path, proof_path=proof_path, dir=d)


def _spzk(*args):
    return subprocess.run([SPZK, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


def test_new_symbols_are_exported():
    for name in ("otti_comp_comm_attach", "otti_comp_comm_dims", "otti_k_addr_timestamps", "otti_snark_gens_points", "otti_zkif_load_inputs",
                 "otti_k_pc_round", "otti_k_pc_export", "otti_k_pc_tail", "otti_k_prod_layer", "otti_k_hash_mem", "otti_k_hash_ops", "otti_k_dot_many",
                 "otti_k_sum3", "otti_k_poly_bound_chunks", "otti_k_pc_grid_cap_override", "otti_k_pc_plan"):
        assert hasattr(oa.lib, name), name
    header = open(os.path.join(os.path.dirname(HERE), "include", "otti_spartan.h")).read()
    for name in ("pc_round", "pc_export", "pc_tail", "prod_layer", "hash_mem", "hash_ops", "dot_many", "sum3", "poly_bound_chunks", "pc_plan"):
        assert callable(getattr(oa.kernels, name)) and f"int32_t otti_k_{name}(" in header, name
    assert callable(oa.kernels.pc_grid_cap) and callable(oa.kernels.pc_grid_cap_restore) and "int32_t otti_k_pc_grid_cap_override(" in header
    assert callable(oa.ComputationCommitment.attach) and callable(oa.kernels.addr_timestamps)


def test_dims_of_a_parsed_oracle_commitment(oracle_case):
    c = oa.ComputationCommitment.from_bytes(oracle_case["comm"])
    oi = oracle_case["oi"]
    assert c.dims == (oi.num_cons, oi.num_vars, oi.num_inputs, _next_pow2(oracle_case["nz"]))
    assert c.has_decommitment is False
    assert oa.lib.otti_comp_comm_dims(None, None, None, None, None, None) == BAD_ARG
    assert oa.lib.otti_comp_comm_dims(c._h, None, None, None, None, None) == 0       # every out pointer is optional


def test_attach_reports_argument_errors_before_touching_a_device(oracle_case):
    r, nz = oracle_case["r"], oracle_case["nz"]
    c = oa.ComputationCommitment.from_bytes(oracle_case["comm"])
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nz)
    for args in ((None, inst._h, gens._h), (c._h, None, gens._h), (c._h, inst._h, None)):
        assert oa.lib.otti_comp_comm_attach(*args, 0) == BAD_ARG
    assert oa.lib.otti_comp_comm_attach(c._h, inst._h, gens._h, 0x10) == BAD_ARG          # an unknown flag
    for other in (oa.synth_r1cs(1 << 8, 4, 5), oa.synth_r1cs(1 << 9, 3, 5)):             # other sizes, another number of inputs
        wrong = oa.Instance.new(other["num_cons"], other["num_vars"], other["num_inputs"], other["A"], other["B"], other["C"])
        with pytest.raises(oa.SpartanError) as ex:
            c.attach(wrong, gens)
        assert ex.value.code == BAD_ARG and "other dimensions" in str(ex.value)
        assert not c.has_decommitment
    if oa.device_count() == 0:
        with pytest.raises(oa.NoDeviceError) as ex:
            c.attach(inst, gens)
        assert ex.value.code == NO_DEVICE and not c.has_decommitment
        with pytest.raises(oa.NoDeviceError):
            oa.kernels.addr_timestamps(np.zeros((3, 4), dtype=np.uint32), 4)
    else:                                                          # with a device the same call completes the commitment
        assert c.attach(inst, gens, verify=True).has_decommitment
    with pytest.raises(oa.SpartanError) as ex:                     # the kernel entry checks its lists before the device as well
        oa.kernels.addr_timestamps(np.full((3, 4), 4, dtype=np.uint32), 4)
    assert ex.value.code == BAD_ARG


def test_snark_kernel_entries_check_their_arguments_before_touching_a_device():
    """unequal table lengths, batches of 0 and 21 instances, a table of 3 elements, a tail of 3 workgroups per instance, and the other geometries
    the launch functions have no answer for: the library's bad-argument error, with or without a device (nothing is launched)"""
    K = oa.kernels
    z = lambda n: np.zeros((n, 32), dtype=np.uint8)
    bad = [
        lambda: K.pc_round([z(4), z(4)], [z(4), z(2)], [None, None], z(1)),                   # unequal lengths
        lambda: K.pc_round([z(4)], [z(4)], [z(2)], z(1)),
        lambda: K.pc_round([], [], [], z(0)),                                                 # ninst = 0
        lambda: K.pc_round([z(4)] * 21, [z(4)] * 21, [None] * 21, z(1)),                      # ninst = 21
        lambda: K.pc_round([z(3)], [z(3)], [None], z(0)),                                     # len = 3
        lambda: K.pc_round([z(2)], [z(2)], [None], z(0), z(1)),                               # a fold needs len >= 4
        lambda: K.pc_round([z(8)], [z(8)], [None], z(3), None, 3, 0),                         # G = 3
        lambda: K.pc_round([z(8)], [z(8)], [None], z(3), None, 2, 2),                         # rk = G
        lambda: K.pc_export([z(4)], [z(2)], [None]),
        lambda: K.pc_export([], [], []),
        lambda: K.pc_export([z(4)] * 21, [z(4)] * 21, [None] * 21),
        lambda: K.pc_export([z(3)], [z(3)], [None]),
        lambda: K.pc_export([z(256)] * 11, [z(256)] * 11, [z(256)] * 11),                     # more than the result buffer holds
        lambda: K.pc_tail([z(64)] * 2, [z(64)] * 2, [None] * 2, 3, 4, z(6), z(4)),            # W = 3
        lambda: K.pc_tail([z(64)], [z(32)], [None], 2, 4, z(6), z(4)),
        lambda: K.pc_tail([], [], [], 1, 4, z(6), z(4)),
        lambda: K.pc_tail([z(64)] * 21, [z(64)] * 21, [None] * 21, 1, 4, z(6), z(4)),
        lambda: K.pc_tail([z(48)], [z(48)], [None], 1, 4, z(5), z(3)),                        # len0 = 48
        lambda: K.pc_tail([z(64)], [z(64)], [None], 2, 1, z(6), z(6)),                        # t_out < W
        lambda: K.pc_tail([z(64)], [z(64)], [None], 1, 64, z(6), z(1)),                       # no round to play
        lambda: K.pc_tail([z(4096)], [z(4096)], [None], 2, 4, z(12), z(10)),                  # 2048 elements per workgroup
        lambda: K.pc_tail([z(64)] * 18, [z(64)] * 18, [None] * 18, 16, 16, z(6), z(2)),       # 288 workgroups
        lambda: K.prod_layer([z(4), z(8)], [z(4), z(8)]),
        lambda: K.prod_layer([z(4)] * 17, [z(4)] * 17),
        lambda: K.prod_layer([], []),
        lambda: K.hash_mem(z(8), z(4), z(1), z(1)),
        lambda: K.hash_mem(z(12), z(12), z(1), z(1)),
        lambda: K.hash_mem(z(4), z(4), z(1), z(1), 4, 0),                                     # one element per rank
        lambda: K.hash_ops(z(8), z(8), z(4), z(1), z(1)),
        lambda: K.hash_ops(z(8), z(8), z(8), z(1), z(1), 2, 2),
        lambda: K.dot_many(z(4), [z(4), z(2)]),
        lambda: K.dot_many(z(4), [z(4)] * 65),
        lambda: K.dot_many(z(4), []),
        lambda: K.sum3([z(4)], [z(4)], [z(2)]),
        lambda: K.sum3([z(4)] * 21, [z(4)] * 21, [z(4)] * 21),
        lambda: K.poly_bound_chunks(z(12), 4, 4, z(2)),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(oa.SpartanError) as ex:
            f()
        assert ex.value.code == BAD_ARG, (k, str(ex.value))


def test_generators_made_from_dims_alone_equal_the_encoders(oracle_case):
    """N = next_pow2(nnz), and the eval generators depend on ilog2(16 N) alone: a verifier needs no circuit to make them"""
    r, nz = oracle_case["r"], oracle_case["nz"]
    enc = oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nz)
    ver = oa.SNARKGens.new(*oa.ComputationCommitment.from_bytes(oracle_case["comm"]).dims)
    for which in ("sat", "eval"):
        a, b = enc.points(which), ver.points(which)
        assert a.shape == b.shape and a.shape[0] > 2 and np.array_equal(a, b), which
    odd = oa.synth_r1cs_compiler_like(300, 3, 2)                     # nnz not a power of two, unpadded sizes
    nz_odd = int(max(odd["A"].size, odd["B"].size, odd["C"].size))
    enc = oa.SNARKGens.new(odd["num_cons"], odd["num_vars"], odd["num_inputs"], nz_odd)
    oi = orc.OInstance(odd["num_cons"], odd["num_vars"], odd["num_inputs"], odd["A"], odd["B"], odd["C"])
    oc = orc.OSnarkComm.encode(oi, orc.OSnarkGens(odd["num_cons"], odd["num_vars"], odd["num_inputs"], nz_odd))
    ver = oa.SNARKGens.new(*oa.ComputationCommitment.from_bytes(oc.bytes).dims)
    for which in ("sat", "eval"):
        assert np.array_equal(enc.points(which), ver.points(which)), which


def test_spzk_verify_from_commitment_and_inputs_alone(oracle_case):
    """the oracle's commitment and proof, the inputs file, nothing else on the command line: exit 0"""
    c = oracle_case
    res = _spzk("verify", c["files"][1], "--comm-in", c["comm_path"], "--proof-in", c["proof_path"])
    assert res.returncode == 0 and "Verification successful" in res.stdout, res.stdout + res.stderr


def _flipped(path, data, at, suffix):
    b = bytearray(data); b[at] ^= 1
    out = str(path) + suffix
    open(out, "wb").write(bytes(b))
    return out


def test_spzk_verify_rejects_what_differs(oracle_case):
    c = oracle_case; inp = c["files"][1]
    bad_proof = _flipped(c["proof_path"], c["proof"], len(c["proof"]) // 3, ".flip")
    res = _spzk("verify", inp, "--comm-in", c["comm_path"], "--proof-in", bad_proof)
    assert res.returncode == 1 and "FAILED" in res.stdout, res.stdout + res.stderr
    bad_comm = _flipped(c["comm_path"], c["comm"], len(c["comm"]) - 40, ".flip")          # inside the last commitment point
    res = _spzk("verify", inp, "--comm-in", bad_comm, "--proof-in", c["proof_path"])
    assert res.returncode == 1, res.stdout + res.stderr
    res = _spzk("verify", inp, "--comm-in", c["comm_path"], "--proof-in", c["proof_path"], "--label", "another_label")
    assert res.returncode == 1 and "FAILED" in res.stdout, res.stdout + res.stderr
    other = dict(c["r"]); inputs = c["r"]["inputs"].copy(); inputs[0][0] ^= 1; other["inputs"] = inputs
    pre = str(c["dir"] / "other")
    oa.zkif_write(other, pre + ".zkif", pre + ".inp.zkif", pre + ".wit.zkif")
    res = _spzk("verify", pre + ".inp.zkif", "--comm-in", c["comm_path"], "--proof-in", c["proof_path"])
    assert res.returncode == 1 and "FAILED" in res.stdout, res.stdout + res.stderr


def test_spzk_verify_reports_a_commitment_file_that_does_not_parse(oracle_case):
    c = oracle_case
    short = c["comm_path"] + ".short"
    open(short, "wb").write(c["comm"][: len(c["comm"]) // 2])
    res = _spzk("verify", c["files"][1], "--comm-in", short, "--proof-in", c["proof_path"])
    assert res.returncode == 1 and "commitment parse failed" in res.stderr and len(res.stderr.strip().splitlines()[-1]) > len("spzk: commitment parse failed (-12): "), res.stdout + res.stderr
    res = _spzk("verify", c["files"][1], "--comm-in", c["comm_path"] + ".missing", "--proof-in", c["proof_path"])
    assert res.returncode == 1 and "cannot read" in res.stderr


def test_spzk_usage_errors_exit_2(oracle_case):
    c = oracle_case
    assert _spzk("encode", c["files"][0]).returncode == 2                                                        # no --comm-out
    assert _spzk("verify", c["files"][1], "--proof-in", c["proof_path"]).returncode == 2                         # SNARK mode: no --comm-in
    assert _spzk("verify", *c["files"][:2], "--comm-in", c["comm_path"], "--proof-in", c["proof_path"]).returncode == 2   # a circuit file too many
    assert _spzk("prove", *c["files"], "--comm-in", c["comm_path"]).returncode == 2                              # no --proof-out
    assert _spzk("prove", "--nizk", *c["files"], "--comm-in", c["comm_path"], "--proof-out", c["proof_path"] + ".x").returncode == 2
    assert _spzk("encode", "--nizk", c["files"][0], "--comm-out", c["comm_path"] + ".x").returncode == 2
    res = _spzk("frobnicate")
    assert res.returncode == 2 and "spzk encode" in res.stderr and "--comm-in" in res.stderr


def test_spzk_encode_and_prove_need_a_device(oracle_case):
    """without a device: the library's no-device message and a non-zero status, not a crash; with one: they work, and the three roles chain"""
    c = oracle_case
    comm2, proof2 = c["comm_path"] + ".mine", c["proof_path"] + ".mine"
    enc = _spzk("encode", *c["files"][:2], "--comm-out", comm2)
    prv = _spzk("prove", *c["files"], "--comm-in", c["comm_path"], "--proof-out", proof2, "--seed", "2a" * 32)
    if oa.device_count() == 0:
        for res in (enc, prv):
            assert res.returncode == 1 and "no HIP device" in res.stderr and "(-20)" in res.stderr, res.stdout + res.stderr
        assert not os.path.exists(comm2) and not os.path.exists(proof2)
    else:
        assert enc.returncode == 0 and open(comm2, "rb").read() == c["comm"], enc.stdout + enc.stderr
        assert prv.returncode == 0 and open(proof2, "rb").read() == c["proof"], prv.stdout + prv.stderr
