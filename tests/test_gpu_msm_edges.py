"""The fixed-base MSM kernels (otti_amd/csrc/k_msm.hip) one launch at a time, through oa.kernels.msm_job — a general MsmJob and the plan it took —
and oa.kernels.msm_scatter_rows, against orc.msm (the oracle's ge_decode / ge_msm / ge_encode) on the cases of tests/msm_cases.py, whose claims
tests/test_msm_cases_host.py proves: every table entry a scalar can reach at the narrow window widths, the ends of the table rows and of their
k_table_fill blocks at the wide ones, every window at both signs, in k_msm_rows<MSM_BULK>, <MSM_BULK_SPARSE>, k_msm_small (many rows; one and two
rows mailed to the host, or summed on the device in a child process) and k_msm_scatter; the sub-chunk seams of the three walking kernels with the
extra terms before, behind and across them (bulk_workgroups = 1: msm_plan.h); the job shapes the prover sends; bullet rounds at other widths.
Bit for bit on the compressed points.  Every test of msm_job asserts the plan the launch took.

Measured on an MI355X: the module takes 7.0 s (34 tests; the slowest is the c = 16 case at 1.6 s, then the bulk seams at c = 4 with 0.9 s).  The
c = 16, R = 1024 table (52 GB) builds in 1.53 s (gens.build_ms: 1448 ms of allocation, 85 ms of upload and kernels): less than the rest of the
module together; that case is the module's last test all the same, in a function of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import msm_cases as mc
import orc
import otti_amd as oa
from test_gpu_kernels import _edge_tables, fr_inv

pytestmark = pytest.mark.gpu
K = oa.kernels
HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS = (4, 7, 8, 9, 11, 12, 13, 15, 16, 17)
HOST_SUM = os.environ.get("OTTI_SMALL_HOST_SUM", "1") != "0"
_CACHE = {}


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def oracle_points(V):
    """(R, the oracle's R + 2 points decoded once) of the generator set of a 2^k = V instance"""
    if ("pts", V) not in _CACHE:
        og = orc.OGens(V, V, 1)
        _CACHE["pts", V] = (og.R, orc.decode_points(og.points()))
    return _CACHE["pts", V]


def want_of(key, V, vectors):
    """the reference: one orc.msm per row over all R + 2 points; computed once per key and never changed"""
    if ("want", key) not in _CACHE:
        raw = oracle_points(V)[1]
        w = np.stack([orc.msm(raw, v) for v in vectors]); w.setflags(write=False)
        _CACHE["want", key] = w
    return _CACHE["want", key]


class table:
    """a generator set whose window table has exactly width c (None: the library's own choice), built now and freed on the way out"""

    def __init__(self, monkeypatch, V, c):
        self.mp, self.V, self.c = monkeypatch, V, c

    def __enter__(self):
        if self.c is None:
            self.mp.delenv("OTTI_MSM_WINDOW", raising=False)
        else:
            self.mp.setenv("OTTI_MSM_WINDOW", str(self.c))
        self.gens = oa.NIZKGens.new(self.V, self.V, 1)
        oa.lib.otti_prepare_device(None, self.gens._h)
        assert self.c is None or self.gens.table_info[0] == self.c
        return self.gens

    def __exit__(self, *exc):
        self.gens.release_device()


def run(gens, job, **kw):
    flat = lambda rows: orc.fr_from_ints([s for r in rows for s in r])           # noqa: E731
    out, plan, _ = K.msm_job(gens, job["rows"], flat(job["dense"]) if job["n_dense"] else None, flat(job["extra"]) if job["extra_base"] else None,
                             job["extra_base"], mode=job["mode"], sparse=job["sparse"], force_bulk=job["force_bulk"], **kw)
    return out, plan


def plan_of(c, job, **kw):
    return mc.plan(c, job["rows"], job["n_dense"], len(job["extra_base"]), job["mode"], bool(job["sparse"]), job["force_bulk"], HOST_SUM, **kw)


def digit_case(c, R=16):
    rows = mc.digit_rows(c, R)
    return rows, want_of(("digits", c), R * R, rows)


def test_orc_msm_is_the_commitment_of_a_dense_row_with_a_blind(rng):
    V = 1 << 10
    og = orc.OGens(V, V, 1); R = og.R
    Z, bl = orc.rand_fr(rng, 2 * R), orc.rand_fr(rng, 2)
    want = orc.commit_rows(og, Z, 2, R, bl)
    z, b = orc.fr_to_ints(Z), orc.fr_to_ints(bl)
    for i in range(2):
        assert eq(orc.msm(og.points(), z[i * R: (i + 1) * R] + [0, b[i]]), want[i])
        assert eq(orc.msm(oracle_points(V)[1], np.concatenate([Z[i * R: (i + 1) * R], orc.fr_from_ints([0]), bl[i: i + 1]])), want[i])


# ------------------------------------------------------------------------------------------------ table contents
@pytest.mark.parametrize("kernel,c", [("bulk", 4), ("bulk", 8), ("small", 4), ("small", 7)])
def test_every_reachable_table_entry_of_every_base(monkeypatch, kernel, c):
    """16 generators + Q + h; every (base, window, magnitude, sign) a scalar below l can look up (test_msm_cases_host.py: none left out), all rows in
    one launch: the block starts and seams of k_table_starts / k_table_fill, read through k_msm_rows<MSM_BULK> and through k_msm_small (rows > 2: fuse 0)"""
    rows, want = digit_case(c)
    job = mc.rows_job(rows, 16, f"table-{kernel}-{c}", force_bulk=kernel == "bulk")
    with table(monkeypatch, 256, c) as gens:
        got, plan = run(gens, job)
    assert plan == plan_of(c, job) and plan["kernel"] == kernel and plan["fuse"] == 0 and len(rows) > 8 and plan["route"] == "device_encode"
    assert eq(got, want), np.nonzero((got != want).any(axis=1))[0][:8]


# ------------------------------------------------------------------------------------------------ digits per kernel
@pytest.mark.parametrize("c", WIDTHS)
def test_digit_rows_through_every_kernel(monkeypatch, c):
    rows, want = digit_case(c)
    R, W = 16, mc.windows(c)
    with table(monkeypatch, 256, c) as gens:
        for sparse in (0, 1):
            job = mc.rows_job(rows, R, f"digits-bulk-{c}", force_bulk=True, sparse=sparse)
            got, plan = run(gens, job)
            assert plan == plan_of(c, job) and plan["kernel"] == ("bulk_sparse" if sparse and W <= 32 else "bulk"), plan
            assert eq(got, want), (sparse, np.nonzero((got != want).any(axis=1))[0][:8])
        for step in (1, 2):                                       # k_msm_small, one and two rows: every workgroup mails its chunk's sum
            for i in range(0, len(rows) - step + 1, step):
                job = mc.rows_job(rows[i: i + step], R, f"digits-small-{c}")
                got, plan = run(gens, job)
                assert plan == plan_of(c, job) and plan["kernel"] == "small" and plan["fuse"] == (2 if HOST_SUM else 1), plan
                assert eq(got, want[i: i + step]), (step, i)
        if c in (4, 12, 16):                                      # k_msm_scatter has no extras: the dense part of every row, every column changed
            idx = np.arange(len(rows) * R, dtype=np.uint64)
            got, _ = K.msm_scatter_rows(gens, len(rows), idx, orc.fr_from_ints([s for v in rows for s in v[:R]]))
            assert eq(got, want_of(("digits-dense", c), R * R, [v[:R] + [0, 0] for v in rows]))


# ------------------------------------------------------------------------------------------------ seams
def _seam_jobs(monkeypatch, kind, c, V, sizes=None):
    R = oracle_points(V)[0]
    S, jobs = mc.seam_rows(kind, c, R, sizes=sizes)
    with table(monkeypatch, V, c) as gens:
        for job in jobs:
            got, plan = run(gens, job, bulk_workgroups=1)
            assert plan == dict(kernel="bulk_sparse" if kind == "sparse" else "bulk", chunk=job["n_dense"], nchunks=1, fuse=0, route="host_encode"), (job["name"], plan)
            want = want_of(job["name"], V, mc.job_vectors(job, R))
            assert eq(got, want), job["name"]
        return gens.build_ms


@pytest.mark.parametrize("c", [4, 8])
def test_bulk_kernel_walks_sub_chunks_of_1024(monkeypatch, c):
    """one workgroup, one chunk of up to 4096 terms (n_dense + extras = 1023, 1024, 1025, 2051, 4096; extras before, behind and across the seam): the
    walk a default plan reaches only from 2^22 constraints up.  4096 terms need the 4096 generators of a 2^24 instance (0.2 and 1.6 GB of table)."""
    _seam_jobs(monkeypatch, "bulk", c, 1 << 24)


@pytest.mark.parametrize("c", [8, 9, 13])
def test_sparse_kernel_walks_sub_chunks_of_its_list_cap(monkeypatch, c):
    """sub_cap = 260 (the list exactly full: 260 * 32 entries), 286, 416 terms; 4 * sub_cap terms need the 2048 generators of a 2^22 instance"""
    _seam_jobs(monkeypatch, "sparse", c, 1 << 22)


def test_scatter_kernel_walks_sub_chunks_of_256(monkeypatch):
    """k_msm_scatter at c = 8: rows 0 and 2 of three get a run of changed columns of the seam sizes (255 .. 1024), row 1 none"""
    V, c = 1 << 22, 8
    R = oracle_points(V)[0]
    S, jobs = mc.seam_rows("scatter", c, R)
    assert S == 256
    rng = np.random.default_rng(8)
    with table(monkeypatch, V, c) as gens:
        for job in jobs:
            n = job["n_dense"]
            idx, s, vectors = [], [], [[0] * (R + 2) for _ in range(3)]
            for r in (0, 2):
                cols = np.sort(rng.choice(R, size=n, replace=False)) if n < R else np.arange(R)
                cols[-1] = R - 1                                   # the row's last column: the run ends where the next row begins
                cols = np.unique(cols)
                for j, col in enumerate(cols):
                    idx.append(r * R + int(col)); s.append(job["dense"][r][j]); vectors[r][int(col)] = job["dense"][r][j]
            got, _ = K.msm_scatter_rows(gens, 3, np.array(idx, dtype=np.uint64), orc.fr_from_ints(s))
            assert eq(got, want_of("scatter-" + job["name"], V, vectors)), job["name"]
            assert not got[1].any()


# ------------------------------------------------------------------------------------------------ the prover's job shapes
@pytest.mark.parametrize("c", [8, None])
def test_job_shapes_the_prover_sends(monkeypatch, c):
    V = 1 << 14
    R = oracle_points(V)[0]
    assert R == 128
    jobs = mc.shape_jobs(R, 8)
    with table(monkeypatch, V, c) as gens:
        width = gens.table_info[0]
        for job in jobs:
            got, plan = run(gens, job)
            assert plan == plan_of(width, job), (job["name"], plan)
            assert eq(got, want_of("shape-" + job["name"], V, mc.job_vectors(job, R))), job["name"]
            if job.get("identity"):
                assert not got.any(), job["name"]                  # the identity compresses to 32 zero bytes
    kernels = {(j["name"].split("-")[0], plan_of(width, j)["kernel"], plan_of(width, j)["route"]) for j in jobs}
    assert {("extras", "small", "raw"), ("extras", "small", "mail" if HOST_SUM else "flag"), ("extras", "small", "device_encode"), ("keep", "bulk", "keep"),
            ("keep", "small", "keep"), ("bulk", "bulk_sparse" if mc.windows(width) <= 32 else "bulk", "host_encode")} <= kernels


# ------------------------------------------------------------------------------------------------ bullet rounds at other widths
@pytest.mark.parametrize("c", [4, 9, 16])
@pytest.mark.parametrize("lgn", [1, 3, 6])
def test_bullet_rounds_at_other_window_widths(rng, monkeypatch, c, lgn):
    """every round's L, R and folded a, b against the oracle's folding reduction, with a and b uniform and from the edge tables (zeros, l - 1, limb
    edges).  lgn = 1: one active term per row, and an empty dot-product slice in every workgroup but the first."""
    n = 1 << lgn; V = n * n
    og = orc.OGens(V, V, 1)
    assert og.R == n
    T = _edge_tables(rng, n, 4)
    one = orc.fr_from_ints([1])
    with table(monkeypatch, V, c) as gens:
        for a, b in ((orc.rand_fr(rng, n), orc.rand_fr(rng, n)), (T[0], T[1]), (T[1], T[3]), (T[2], T[0]), (T[3], T[2])):
            blinds, us = orc.rand_fr(rng, 2 * lgn), orc.rand_fr(rng, lgn); uis = fr_inv(us)
            s = np.repeat(one, n, axis=0)
            ca, cb, cur = a, b, n
            for k in range(lgn):
                fold = k > 0
                oa.stats_enable(True)                              # the round entry returns no plan: the launch counters say which kernel ran
                try:
                    LR, ca, cb, s, _ = K.bullet_round(gens, cur, ca, cb, s, blinds[2 * k: 2 * k + 2], us[k - 1: k] if fold else None, uis[k - 1: k] if fold else None)
                    st = oa.stats_read()
                finally:
                    oa.stats_enable(False)
                assert st["msm_small"][0] == 1 and st["msm_rows"][0] == 0, st
                wLR = orc.bullet_reduce(og, a, b, blinds, us[: k + 1])[0]
                assert eq(LR, wLR[k]), ("L/R of round", k)
                if fold:
                    pa, pb = orc.bullet_reduce(og, a, b, blinds, us[:k])[1:3]
                    assert eq(ca, pa) and eq(cb, pb), ("state before round", k)
                cur //= 2
            a1, b1, s = K.bullet_last_fold(ca[:2], cb[:2], s, us[lgn - 1: lgn], uis[lgn - 1: lgn])
            _, wa, wb, wG = orc.bullet_reduce(og, a, b, blinds, us)
            assert eq(a1, wa) and eq(b1, wb)
            got, plan, _ = K.msm_job(gens, 1, s, mode="raw")
            assert plan["kernel"] == "small" and plan["route"] == "raw" and eq(got, wG)


# ------------------------------------------------------------------------------------------------ the device sum
def small_sum_lines():
    """msm_cases.small_sum_lines on this process's device (the worker's "edges" mode calls this too); OTTI_MSM_WINDOW=8 is the caller's"""
    gens = {"digits": oa.NIZKGens.new(256, 256, 1), "shapes": oa.NIZKGens.new(1 << 14, 1 << 14, 1)}
    lines = mc.small_sum_lines(lambda which, job: run(gens[which], job))
    assert all(g.table_info[0] == 8 for g in gens.values())
    for g in gens.values():
        g.release_device()
    return lines


def test_device_sum_equals_host_sum_on_the_fused_cases(monkeypatch):
    """the c = 8 digit rows and the one- and two-row shape jobs once more with OTTI_SMALL_HOST_SUM=0 (read once per process: a child), where the last
    workgroup to arrive sums the chunk results: hex for hex what this process's mailed launches give — which the tests above hold against the oracle"""
    monkeypatch.setenv("OTTI_MSM_WINDOW", "8")
    mine = small_sum_lines()
    env = dict(os.environ, OTTI_SMALL_HOST_SUM="0", OTTI_MSM_WINDOW="8")
    res = subprocess.run([sys.executable, os.path.join(HERE, "msm_mail_worker.py"), "edges"], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    theirs = [ln[5:] for ln in res.stdout.splitlines() if ln.startswith("EDGE ")]
    assert len(mine) == len(theirs) > 400
    assert all(ln.split()[1] == "1" for ln in theirs) and all(ln.split()[1] == ("2" if HOST_SUM else "1") for ln in mine)
    assert [(ln.split()[0], ln.split()[2]) for ln in mine] == [(ln.split()[0], ln.split()[2]) for ln in theirs]
    rows, want = digit_case(8)
    assert mine[0].split()[2] == want[0].tobytes().hex() and mine[len(rows)].split()[2] == want[:2].tobytes().hex()


# ------------------------------------------------------------------------------------------------ the work list where kMsmBulkChunk is the cap
def test_sparse_kernel_at_width_16_where_the_chunk_is_the_cap(monkeypatch):
    """c = 16: W = 16 and sub_cap = kMsmBulkChunk = 512 itself.  1024 dense terms + 3 extras (2 S + 3) over the 1024 generators of a 2^20 instance: a
    52 GB table, the one case that needs it, behind the others (nothing else reaches this branch below 2^20 constraints)"""
    assert mc.sub_cap(16) == mc.K_MSM_BULK_CHUNK
    build_ms = _seam_jobs(monkeypatch, "sparse", 16, 1 << 20, sizes=[(1024, 3)])
    print(f"c = 16, R = 1024 table: build_ms = {build_ms}")
