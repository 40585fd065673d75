"""Worker of tests/test_gpu_snark_attach.py: ONE GPU step in a fresh process (the test gives each step its own time limit and starts no
further step after one that failed).  Exit status 0 and a last line starting with OK mean the step passed.

  kernel <case>            kernels.addr_timestamps against the sequential scan written out below, twice
  attach <lg> <kind>       from_bytes(comm.bytes).attach(inst, gens) proves byte-identically to the encoder's own commitment; prints DIGEST
  wrong <variant>          attach(verify=True) refuses an instance that differs in one entry; attach(verify=False) gives a rejected proof
  encode <lg>              prints DIGEST of ComputationCommitment.encode(...).bytes (run with and without OTTI_DECOMM_HOST=1)
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import otti_amd as oa  # noqa: E402

LABEL, SEED = b"snark_example", b"\x2a" * 32


def sequential_scan(addr3, M):
    """the definition: one counter array shared by the three lists, walked k = 0, 1, 2 and i = 0 .. N - 1 in order"""
    audit = [0] * M
    read_ts = np.zeros(addr3.shape, dtype=np.uint32)
    for k in range(3):
        row, out = addr3[k].tolist(), []
        for a in row:
            out.append(audit[a])
            audit[a] += 1
        read_ts[k] = out
    return read_ts, np.array(audit, dtype=np.uint32)


def kernel_case(name):
    rng = np.random.default_rng(20261016)
    if name == "uniform":
        N, M = 1 << 12, 1 << 12; a = rng.integers(0, M, size=(3, N))
    elif name == "one_address_zero":
        N, M = 1 << 12, 1 << 10; a = np.zeros((3, N))
    elif name == "one_address_nonzero":
        N, M = 1 << 12, 1 << 10; a = np.full((3, N), 777)
    elif name == "ascending":
        N, M = 1 << 11, 1 << 11; a = np.tile(np.arange(N), (3, 1))
    elif name == "descending":
        N, M = 1 << 11, 1 << 11; a = np.tile(np.arange(N)[::-1], (3, 1))
    elif name == "runs":
        N, M = 1 << 13, 1 << 9; a = np.tile(np.repeat(np.arange(N // 37 + 1), 37)[:N] % M, (3, 1)); a[1] = a[1][::-1]
    elif name == "two_alternating":
        N, M = 1 << 12, 1 << 16; a = np.tile(np.where(np.arange(N) % 2 == 0, 5, 40000), (3, 1))
    elif name == "shared_counter":
        N, M = 64, 128; a = np.zeros((3, N)); a[0, 3] = a[1, 0] = a[1, 63] = a[2, 17] = 99; a[0, 5:9] = 7; a[2, 5:9] = 7
    elif name == "all_padding":
        N, M = 1 << 10, 1 << 10; a = np.zeros((3, N))
    elif name == "real_then_padding":                            # lists of different real lengths, zeros among the real entries, a zero-address tail
        N, M = 1 << 12, 1 << 11; a = rng.integers(0, 4, size=(3, N)) * rng.integers(0, M // 4, size=(3, N))
        a[0, 3000:] = 0; a[1, 17:] = 0; a[2, N - 1:] = 0
    elif name == "smallest":
        N, M = 2, 2; a = np.array([[1, 0], [1, 1], [0, 0]])
    elif name == "N_above_M":
        N, M = 1 << 14, 8; a = rng.integers(0, M, size=(3, N))
    elif name == "N_below_M":
        N, M = 16, 1 << 20; a = rng.integers(0, M, size=(3, N)); a[1, 4] = a[0, 9]; a[2, 0] = M - 1
    elif name == "M_not_a_power_of_two":
        N, M = 3000, 70001; a = rng.integers(0, M, size=(3, N))
    elif name == "constant_column_2p20":
        N, M = 1 << 20, 1 << 21; a = rng.integers(0, M, size=(3, N))
        a[rng.random((3, N)) < 0.4] = 1 << 20                    # the constant column: 40 % of all entries
        a[:, N - N // 8:] = 0                                    # and a padding tail
    else:
        raise SystemExit(f"unknown case {name}")
    a = np.ascontiguousarray(a, dtype=np.uint32)
    want_ts, want_audit = sequential_scan(a, M)
    for rep in range(2):                                         # repeated: the same numbers again
        ts, audit, ms = oa.kernels.addr_timestamps(a, M)
        bad = np.argwhere(ts != want_ts)
        assert bad.size == 0, f"{name} (call {rep}): read_ts differs first at {bad[0]}: got {ts[tuple(bad[0])]}, want {want_ts[tuple(bad[0])]}"
        assert np.array_equal(audit, want_audit), f"{name} (call {rep}): audit differs first at {np.argwhere(audit != want_audit)[0]}"
    print(f"OK kernel {name} N={N} M={M} kernel_ms={ms:.3f}", flush=True)


def synth(lg, kind):
    r = (oa.synth_r1cs if kind == "uniform" else oa.synth_r1cs_compiler_like)(1 << lg, 10, 1 if kind == "uniform" else 7)
    return r, int(max(r["A"].size, r["B"].size, r["C"].size))


def objects(r, nz):
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    return inst, oa.SNARKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"], nz)


def attach_case(lg, kind):
    import orc
    r, nz = synth(lg, kind)
    inst, gens = objects(r, nz)
    comm = oa.ComputationCommitment.encode(inst, gens)
    v, i = oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"])
    want = oa.SNARK.prove(inst, comm, v, i, gens, LABEL, SEED).bytes
    mine = oa.ComputationCommitment.from_bytes(comm.bytes)
    assert not mine.has_decommitment and comm.has_decommitment and mine.dims == comm.dims
    assert mine.attach(inst, gens) is mine and mine.has_decommitment
    got = oa.SNARK.prove(inst, mine, v, i, gens, LABEL, SEED)
    assert got.bytes == want, "the proof from the attached commitment differs from the proof from the encoder's own"
    mine.attach(inst, gens, verify=True)                         # already attached: nothing to do
    checked = oa.ComputationCommitment.from_bytes(comm.bytes).attach(inst, gens, verify=True)
    assert checked.has_decommitment and oa.SNARK.prove(inst, checked, v, i, gens, LABEL, SEED).bytes == want
    got.verify(oa.ComputationCommitment.from_bytes(comm.bytes), i, oa.SNARKGens.new(*mine.dims), LABEL)   # a verifier with the commitment alone
    og = orc.OSnarkGens(r["num_cons"], r["num_vars"], r["num_inputs"], nz)
    assert orc.snark_verify(orc.OSnarkComm.parse(comm.bytes), r["inputs"], og, got.bytes, LABEL) == 0, "the oracle's verifier rejects the proof"
    print("DIGEST", hashlib.sha256(comm.bytes).hexdigest(), hashlib.sha256(got.bytes).hexdigest(), flush=True)
    print("OK attach", lg, kind, flush=True)


def wrong_case(variant):
    r, nz = synth(12, "compiler")
    inst, gens = objects(r, nz)
    comm = oa.ComputationCommitment.encode(inst, gens)
    other = dict(r); A = r["A"].copy()
    e = A.size // 2
    if variant == "coefficient":
        A["val"][e][0] ^= 1
    elif variant == "column":
        A["col"][e] = (int(A["col"][e]) + 1) % int(r["num_vars"])
    else:
        raise SystemExit(f"unknown variant {variant}")
    other["A"] = A
    wrong = oa.Instance.new(other["num_cons"], other["num_vars"], other["num_inputs"], other["A"], other["B"], other["C"])
    mine = oa.ComputationCommitment.from_bytes(comm.bytes)
    try:
        mine.attach(wrong, gens, verify=True)
        raise AssertionError("attach(verify=True) accepted an instance the commitment was not made for")
    except oa.SpartanError as ex:
        assert ex.code == -21 and ("comm_ops" in str(ex) or "comm_mem" in str(ex)), str(ex)
    assert not mine.has_decommitment
    mine.attach(wrong, gens)                                     # trusting the caller: dimensions agree, nothing else is looked at
    assert mine.has_decommitment
    v, i = oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"])
    proof = oa.SNARK.prove(wrong, mine, v, i, gens, LABEL, SEED)
    try:
        proof.verify(oa.ComputationCommitment.from_bytes(comm.bytes), i, gens, LABEL)
        raise AssertionError("a proof made from the wrong instance's decommitment was accepted")
    except oa.ProofVerifyError:
        pass
    print("OK wrong", variant, flush=True)


def encode_case(lg):
    r, nz = synth(lg, "compiler")
    inst, gens = objects(r, nz)
    print("DIGEST", hashlib.sha256(oa.ComputationCommitment.encode(inst, gens).bytes).hexdigest(), flush=True)
    print("OK encode", lg, flush=True)


if __name__ == "__main__":
    what = sys.argv[1]
    if what == "kernel":
        kernel_case(sys.argv[2])
    elif what == "attach":
        attach_case(int(sys.argv[2]), sys.argv[3])
    elif what == "wrong":
        wrong_case(sys.argv[2])
    elif what == "encode":
        encode_case(int(sys.argv[2]))
    else:
        raise SystemExit(f"unknown step {what}")
