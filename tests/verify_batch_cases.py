"""What the otti_nizk_verify_batch tests share: the call through the Python entry, the C entry itself in the shape of verify_many_cases.raw_many, and
the walk of a one-mutant-per-field corpus in small batches.  Used by test_verify_batch_host.py (oracle proofs, host sum) and
test_gpu_verify_batch.py (the product's proofs, device sum)."""
import ctypes

import numpy as np

import otti_amd as oa

SEED = bytes(range(32))


def batch(inst, gens, label, items, threads=0, seed=SEED, details=False):
    return oa.NIZK.verify_batch(inst, [p for p, _ in items], [oa.InputsAssignment.new(i) for _, i in items], gens, label, threads, seed, details)


def raw_batch(inst_h, gens_h, label, items, threads=0, results=True, null_proof_at=None, arrays=True):
    """vm.raw_many's call on otti_nizk_verify_batch"""
    n = len(items)
    _vp, _sz, _i32 = oa.api._vp, oa.api._sz, oa.api._i32
    keep = [(np.frombuffer(p, dtype=np.uint8), np.ascontiguousarray(i, dtype=np.uint8)) for p, i in items]
    ip, ic, pp, pl = (_vp * max(1, n))(), (_sz * max(1, n))(), (_vp * max(1, n))(), (_sz * max(1, n))()
    for k, (p, i) in enumerate(keep):
        ip[k], ic[k], pp[k], pl[k] = oa.api._ptr(i), i.shape[0], (None if k == null_proof_at else p.ctypes.data_as(_vp)), p.size
    res, rej = (_i32 * max(1, n))(*([99] * max(1, n))), _sz(12345)
    a = (ip, ic, pp, pl) if arrays else (None, None, None, None)
    rc = oa.lib.otti_nizk_verify_batch(inst_h, gens_h, label, len(label), n, *a, threads, None, res if results else None, ctypes.byref(rej), None)
    return int(rc), [int(res[k]) for k in range(n)], int(rej.value)


def corpus_in_batches(run, verify_batch, size=8):
    """the corpus through verify_batch(blobs) -> (codes, info) in batches of `size` mutants with the good proof at both ends; returns the codes in
    with_good()'s layout and the infos"""
    blobs = [m for _, _, m in run.corpus.mutants]
    got, infos = [], []
    for at in range(0, len(blobs), size):
        part = blobs[at:at + size]
        codes, info = verify_batch([run.proof] + part + [run.proof])
        assert codes[0] == 0 and codes[-1] == 0, (at, codes)
        got += codes[1:-1]; infos.append(info)
    mid = len(blobs) // 2
    return [0] + got[:mid] + [0] + got[mid:] + [0], infos
