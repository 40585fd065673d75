"""The list of items the verify_many tests verify, built from six good proofs of one instance, and the calls they compare: otti_nizk_verify on
each item alone against otti_nizk_verify_many on the list.  Shared by test_verify_many_host.py (oracle proofs, host evaluation) and
test_gpu_verify_many.py (device proofs, batched device evaluation).  Proof layout (NizkProof::serialize): the row commitments (u64 count, 32 bytes
each), then the first sum-check's comm_polys (u64 count, 32 bytes each) ...; at the end rx and ry (u64 count, 32 bytes each)."""
import ctypes

import numpy as np

import otti_amd as oa

MALFORMED, VERIFY_INTERNAL, INVALID_NUM_INPUTS, BAD_ARG = -12, -10, -3, -21
KINDS = ("good", "good", "flipped_sumcheck_commitment", "truncated", "input_changed", "good", "rx0_replaced", "wrong_input_count")


def tamper_list(proofs, inputs32, num_cons_padded, num_vars_padded):
    """[(proof bytes, inputs (n, 32) uint8)] for KINDS, from six good proofs (their points differ) and the instance's inputs (at least one)"""
    assert len(proofs) == 6 and inputs32.shape[0] >= 1
    nrx, nry = num_cons_padded.bit_length() - 1, (2 * num_vars_padded).bit_length() - 1
    ell = num_vars_padded.bit_length() - 1
    n_rows = 1 << (ell // 2)
    flipped = bytearray(proofs[2]); flipped[8 + 32 * n_rows + 8 + 5] ^= 0x10          # inside comm_polys[0] of the first sum-check
    changed = inputs32.copy(); changed[0, 0] ^= 1
    rx0 = len(proofs[5]) - (8 + 32 * nry) - 32 * nrx
    assert int.from_bytes(proofs[5][rx0 - 8:rx0], "little") == nrx                     # the count in front of rx: the offset is right
    replaced = bytearray(proofs[5]); replaced[rx0:rx0 + 32] = (7).to_bytes(32, "little")
    return [(proofs[0], inputs32), (proofs[1], inputs32), (bytes(flipped), inputs32), (proofs[3][:-7], inputs32), (proofs[0], changed),
            (proofs[4], inputs32), (bytes(replaced), inputs32), (proofs[1], inputs32[:-1])]


def single_code(inst, gens, label, proof, inputs32):
    """what otti_nizk_verify returns for this item alone"""
    i = np.ascontiguousarray(inputs32, dtype=np.uint8); buf = np.frombuffer(proof, dtype=np.uint8)
    return int(oa.lib.otti_nizk_verify(inst._h, oa.api._ptr(i), i.shape[0], gens._h, label, len(label), oa.api._ptr(buf), buf.size))


def many(inst, gens, label, items, threads=0):
    """otti_nizk_verify_many through the Python entry: the list of result codes"""
    return oa.NIZK.verify_many(inst, [p for p, _ in items], [oa.InputsAssignment.new(i) for _, i in items], gens, label, threads)


def raw_many(inst_h, gens_h, label, items, threads=0, results=True, null_proof_at=None, arrays=True):
    """the C entry itself: (return code, results, n_rejected)"""
    n = len(items)
    _vp, _sz, _i32 = oa.api._vp, oa.api._sz, oa.api._i32
    keep = [(np.frombuffer(p, dtype=np.uint8), np.ascontiguousarray(i, dtype=np.uint8)) for p, i in items]
    ip, ic, pp, pl = (_vp * max(1, n))(), (_sz * max(1, n))(), (_vp * max(1, n))(), (_sz * max(1, n))()
    for k, (p, i) in enumerate(keep):
        ip[k], ic[k], pp[k], pl[k] = oa.api._ptr(i), i.shape[0], (None if k == null_proof_at else p.ctypes.data_as(_vp)), p.size
    res, rej = (_i32 * max(1, n))(*([99] * max(1, n))), _sz(12345)
    a = (ip, ic, pp, pl) if arrays else (None, None, None, None)
    rc = oa.lib.otti_nizk_verify_many(inst_h, gens_h, label, len(label), n, *a, threads, res if results else None, ctypes.byref(rej))
    return int(rc), [int(res[k]) for k in range(n)], int(rej.value)


def check_list(inst, gens, label, items):
    """assertions (a) - (d) of the issue and the thread counts; returns the codes"""
    singles = [single_code(inst, gens, label, p, i) for p, i in items]
    got = many(inst, gens, label, items)
    print("single codes", singles, "verify_many", got)
    assert got == singles                                                               # (a)
    for kind, code in zip(KINDS, got):                                                   # (b)
        assert (code == 0) == (kind == "good"), (kind, code)
    assert got[KINDS.index("truncated")] == MALFORMED and got[KINDS.index("wrong_input_count")] == INVALID_NUM_INPUTS
    rc, raw, rejected = raw_many(inst._h, gens._h, label, items)
    assert rc == 0 and raw == singles and rejected == sum(1 for c in singles if c != 0) == 5          # (c)
    assert "5 of 8" in oa.api._last_error()
    assert many(inst, gens, label, items[::-1]) == singles[::-1]                         # (d)
    for threads in (1, 3):
        assert many(inst, gens, label, items, threads) == singles, threads
    for k in (0, 3, 6):                                                                  # a list of one equals the single call
        assert many(inst, gens, label, [items[k]]) == [singles[k]]
    return singles


def check_refusals(inst, gens, label, items):
    assert oa.NIZK.verify_many(inst, [], oa.InputsAssignment.new(items[0][1]), gens, label) == []
    rc, _, rejected = raw_many(inst._h, gens._h, label, [], arrays=False)
    assert rc == 0 and rejected == 0                                                    # count == 0: OTTI_OK with nothing done, null arrays and all
    assert raw_many(None, gens._h, label, items)[0] == BAD_ARG
    assert raw_many(inst._h, None, label, items)[0] == BAD_ARG
    assert raw_many(inst._h, gens._h, label, items, results=False)[0] == BAD_ARG
    assert raw_many(inst._h, gens._h, label, items, arrays=False)[0] == BAD_ARG
    rc, res, _ = raw_many(inst._h, gens._h, label, items, null_proof_at=1)
    assert rc == BAD_ARG and res == [99] * len(items)                                   # refused before anything is touched
    rc, res, _ = raw_many(inst._h, gens._h, label, items, threads=17)
    assert rc == BAD_ARG and res == [99] * len(items)
    assert raw_many(inst._h, gens._h, label, items, threads=16)[0] == 0
