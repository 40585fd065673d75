"""What the otti_snark_verify_many tests share: the items they verify, built from six good SNARK proofs of one commitment; the calls they compare
(otti_snark_verify on each item alone against otti_snark_verify_many on the list); and a bank of points whose sums the oracle can state, for the
kernel-level test of the batched row sums.  Used by test_snark_verify_many_host.py (oracle proofs, host sums), test_gpu_snark_verify_many.py
(device proofs, batched device sums) and test_gpu_row_sum_many.py.

Proof layout (SnarkProof::serialize): the R1CS proof (row commitments: u64 count, 32 bytes each; the first sum-check's comm_polys likewise; ...),
the three inst_evals, then comm_derefs (u64 count, 32 bytes each), eval_row (init: the first scalar of the product layer), ...
Commitment layout (CompComm::serialize): six u64, comm_ops (u64 count, 32 bytes each), comm_mem likewise."""
import ctypes

import numpy as np

import otti_amd as oa
import orc

MALFORMED, DECOMPRESS, VERIFY_INTERNAL, INVALID_NUM_INPUTS, BAD_ARG = -12, -11, -10, -3, -21
KINDS = ("good", "good", "flipped_sumcheck_commitment", "truncated", "input_changed", "wrong_input_count", "derefs_undecodable", "derefs_rows_swapped",
         "product_scalar_and_derefs_undecodable")
UNDECODABLE = bytes([1] + [0] * 31)                        # s = 1 is odd: not a ristretto255 encoding


def _u64(b, pos):
    return int.from_bytes(b[pos:pos + 8], "little")


def derefs_offset(proof):
    """(offset of comm_derefs' first point, their count): a walk over the R1CS proof's fields, as SnarkProof::serialize writes them"""
    pos = 0

    def pts():
        nonlocal pos
        pos += 8 + 32 * _u64(proof, pos)

    def sumcheck():
        nonlocal pos
        pts(); pts()
        k = _u64(proof, pos); pos += 8
        for _ in range(k):
            pos += 64                                        # delta, beta
            pos += 8 + 32 * _u64(proof, pos)                 # z
            pos += 64                                        # z_delta, z_beta

    pts()                                                    # comm_vars
    sumcheck()
    pos += 32 * 4 + 32 * 3 + 32 * 8 + 32 * 2                 # claims_phase2, pok, prod, eq1
    sumcheck()
    pos += 32                                                # comm_vars_at_ry
    pts(); pts(); pos += 32 * 4                              # polyeval: L_vec, R_vec, delta, beta, z1, z2
    pos += 32 * 2                                            # eq2
    pos += 32 * 3                                            # inst_evals
    n = _u64(proof, pos)
    assert 2 <= n <= 1 << 20 and n & (n - 1) == 0, n         # a power of two of rows: the walk ended where it should
    return pos + 8, n


def comm_sizes(comm_bytes):
    """(offset of comm_ops' first point, count of comm_ops, count of comm_mem)"""
    n_ops = _u64(comm_bytes, 48)
    n_mem = _u64(comm_bytes, 56 + 32 * n_ops)
    assert len(comm_bytes) == 64 + 32 * (n_ops + n_mem)
    return 56, n_ops, n_mem


def tamper_list(proofs, inputs32):
    """[(proof bytes, inputs (n, 32) uint8)] for KINDS, from six good proofs and the instance's inputs (at least one)"""
    assert len(proofs) == 6 and inputs32.shape[0] >= 1
    n_rows = _u64(proofs[2], 0)
    flipped = bytearray(proofs[2]); flipped[8 + 32 * n_rows + 8 + 5] ^= 0x10           # inside comm_polys[0] of the first sum-check
    changed = inputs32.copy(); changed[0, 0] ^= 1
    d0, nd = derefs_offset(proofs[4])
    undec = bytearray(proofs[4]); undec[d0 + 32 * (nd // 3):d0 + 32 * (nd // 3) + 32] = UNDECODABLE
    d5, n5 = derefs_offset(proofs[5])
    swapped = bytearray(proofs[5]); swapped[d5:d5 + 32], swapped[d5 + 32:d5 + 64] = proofs[5][d5 + 32:d5 + 64], proofs[5][d5:d5 + 32]
    assert bytes(swapped) != proofs[5]
    d3, n3 = derefs_offset(proofs[3])
    both = bytearray(proofs[3]); both[d3 + 32 * n3] ^= 1                               # eval_row.init, the product layer's first scalar
    both[d3 + 32 * (n3 - 1):d3 + 32 * n3] = UNDECODABLE
    return [(proofs[0], inputs32), (proofs[1], inputs32), (bytes(flipped), inputs32), (proofs[3][:-7], inputs32), (proofs[0], changed),
            (proofs[1], inputs32[:-1]), (bytes(undec), inputs32), (bytes(swapped), inputs32), (bytes(both), inputs32)]


def single_code(comm, gens, label, proof, inputs32):
    """what otti_snark_verify returns for this item alone"""
    i = np.ascontiguousarray(inputs32, dtype=np.uint8); buf = np.frombuffer(proof, dtype=np.uint8)
    return int(oa.lib.otti_snark_verify(comm._h, oa.api._ptr(i), i.shape[0], gens._h, label, len(label), oa.api._ptr(buf), buf.size))


def many(comm, gens, label, items, threads=0):
    """otti_snark_verify_many through the Python entry: the list of result codes"""
    return oa.SNARK.verify_many(comm, [p for p, _ in items], [oa.InputsAssignment.new(i) for _, i in items], gens, label, threads)


def raw_many(comm_h, gens_h, label, items, threads=0, results=True, null_proof_at=None, arrays=True):
    """the C entry itself: (return code, results, n_rejected)"""
    n = len(items)
    _vp, _sz, _i32 = oa.api._vp, oa.api._sz, oa.api._i32
    keep = [(np.frombuffer(p, dtype=np.uint8), np.ascontiguousarray(i, dtype=np.uint8)) for p, i in items]
    ip, ic, pp, pl = (_vp * max(1, n))(), (_sz * max(1, n))(), (_vp * max(1, n))(), (_sz * max(1, n))()
    for k, (p, i) in enumerate(keep):
        ip[k], ic[k], pp[k], pl[k] = oa.api._ptr(i), i.shape[0], (None if k == null_proof_at else p.ctypes.data_as(_vp)), p.size
    res, rej = (_i32 * max(1, n))(*([99] * max(1, n))), _sz(12345)
    a = (ip, ic, pp, pl) if arrays else (None, None, None, None)
    rc = oa.lib.otti_snark_verify_many(comm_h, gens_h, label, len(label), n, *a, threads, res if results else None, ctypes.byref(rej))
    return int(rc), [int(res[k]) for k in range(n)], int(rej.value)


def check_list(comm, gens, label, items, monkeypatch):
    """the list against the single verifier, code for code: every thread count, both orders, the host route, n_rejected; returns the codes"""
    singles = [single_code(comm, gens, label, p, i) for p, i in items]
    got = many(comm, gens, label, items)
    print("single codes", singles, "verify_many", got)
    assert got == singles
    for kind, code in zip(KINDS, got):
        assert (code == 0) == (kind == "good"), (kind, code)
    assert got[KINDS.index("truncated")] == MALFORMED and got[KINDS.index("wrong_input_count")] == INVALID_NUM_INPUTS
    rc, raw, rejected = raw_many(comm._h, gens._h, label, items)
    assert rc == 0 and raw == singles and rejected == sum(1 for c in singles if c != 0) == 7
    assert "7 of 9" in oa.api._last_error()
    for threads in (0, 1, 2, 4):
        assert many(comm, gens, label, items, threads) == singles, threads
        assert many(comm, gens, label, items[::-1], threads) == singles[::-1], threads
    with monkeypatch.context() as mp:
        mp.setenv("OTTI_VERIFY_HOST", "1")
        assert [single_code(comm, gens, label, p, i) for p, i in items] == singles
        assert many(comm, gens, label, items) == singles
        assert many(comm, gens, label, items[::-1], 2) == singles[::-1]
    for k in (0, 3, 6):                                                                  # a list of one equals the single call
        assert many(comm, gens, label, [items[k]]) == [singles[k]]
    return singles


def check_refusals(comm, gens, label, items):
    assert oa.SNARK.verify_many(comm, [], oa.InputsAssignment.new(items[0][1]), gens, label) == []
    rc, _, rejected = raw_many(comm._h, gens._h, label, [], arrays=False)
    assert rc == 0 and rejected == 0                                                    # count == 0: OTTI_OK with nothing done, null arrays and all
    assert raw_many(None, gens._h, label, items)[0] == BAD_ARG
    assert raw_many(comm._h, None, label, items)[0] == BAD_ARG
    assert raw_many(comm._h, gens._h, label, items, results=False)[0] == BAD_ARG
    assert raw_many(comm._h, gens._h, label, items, arrays=False)[0] == BAD_ARG
    rc, res, _ = raw_many(comm._h, gens._h, label, items, null_proof_at=1)
    assert rc == BAD_ARG and res == [99] * len(items)                                   # refused before anything is touched
    rc, res, _ = raw_many(comm._h, gens._h, label, items, threads=17)
    assert rc == BAD_ARG and res == [99] * len(items)
    assert raw_many(comm._h, gens._h, label, items, threads=16)[0] == 0


# ------------------------------------------------------------------------------------------------ points whose sums the oracle can state
BANK_POINTS = 2049


class RowBank:
    """rows of integers over 16 generators and the oracle's commitments to them, made once: [0] the zero row (the identity), D[i] = (i + 1) P_(i % 16)
    (BANK_POINTS distinct points), N[i] = -D[i], and 8 dense random rows.  want(idx, s) = the oracle's commitment to sum_i s[i] * row[idx[i]] mod l."""

    def __init__(self):
        self.og = orc.OGens(256, 256, 1)
        assert self.og.R == 16
        l = orc.L_ORDER
        rnd = np.random.default_rng(20261020)
        self.rows = [{}] + [{i % 16: i + 1} for i in range(BANK_POINTS)] + [{i % 16: l - (i + 1)} for i in range(BANK_POINTS)]
        self.rows += [{j: v for j, v in enumerate(orc.fr_to_ints(orc.rand_fr(rnd, 16)))} for _ in range(8)]
        self.zero, self.D, self.N, self.dense = 0, 1, 1 + BANK_POINTS, 1 + 2 * BANK_POINTS
        dense = orc.fr_from_ints([r.get(j, 0) for r in self.rows for j in range(16)])
        self.points = orc.commit_rows(self.og, dense, len(self.rows), 16, orc.fr_from_ints([0] * len(self.rows)))
        assert not self.points[0].any()

    def want(self, idx, s):
        acc = [0] * 16
        for i, k in zip(idx, s):
            for j, v in self.rows[i].items():
                acc[j] = (acc[j] + k * v) % orc.L_ORDER
        return orc.commit_rows(self.og, orc.fr_from_ints(acc), 1, 16, orc.fr_from_ints([0]))[0]


_bank = []


def row_bank():
    if not _bank:
        _bank.append(RowBank())
    return _bank[0]
