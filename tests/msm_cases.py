"""Cases for the fixed-base MSM kernels (otti_amd/csrc/k_msm.hip), as plain Python: no GPU, no library.  tests/test_msm_cases_host.py proves what
is claimed here by brute force; tests/test_gpu_msm_edges.py runs the cases through oa.kernels.msm_job / msm_scatter_rows against orc.msm.

The recoding, restated: with K = sum_w 2^(c-1+cw) over the W = 253 // c + 1 windows, s' = s + K, and the signed digit of window w is
(window w of s') - 2^(c-1), in [-E, E-1] with E = 2^(c-1).  Digit d looks up table entry |d| - 1 of row (base, w) and negates it when d < 0, so the
last entry of a row (magnitude E) is reached only by the digit -E.  sum_w digit_w 2^(cw) = s, and that representation is unique.

A job is a dict: rows, n_dense, dense (rows lists of n_dense integers), extra_base, extra (rows lists of len(extra_base) integers), mode, sparse,
force_bulk, name.  job_vectors() folds a job's rows into integer vectors over the R + 2 generator points: the reference sum is their MSM."""
import random

L = 2 ** 252 + 27742317777372353535851937790883648493
# k_msm.hip / msm_plan.h
K_MSM_MAX_CHUNK, K_MSM_BULK_CHUNK, K_MSM_SCATTER_SUB = 1024, 512, 256
K_MSM_LIST_CAP = (K_MSM_BULK_CHUNK + 8) * 16
K_MSM_THREADS, K_SMALL_CHUNK, K_MSM_BULK_TERMS, K_MSM_BULK_WORKGROUPS, K_MSM_MAIL_CAP, K_HOST_ENCODE_ROWS = 256, 64, 4096, 1024, 512, 8
NARROW_MAX = 8                                   # widths up to this one are covered exhaustively


def windows(c):
    return 253 // c + 1


def recoding_constant(c):
    return sum(1 << (c - 1 + c * w) for w in range(windows(c)))


def digits(s, c):
    sp, mask, half = s + recoding_constant(c), (1 << c) - 1, 1 << (c - 1)
    return [((sp >> (c * w)) & mask) - half for w in range(windows(c))]


def table_block(c):
    """T: entries per k_table_fill block"""
    return 1 << min(6, c - 1)


def sub_cap(c):
    """terms per sub-chunk of the work-list kernel"""
    return min(K_MSM_BULK_CHUNK, K_MSM_LIST_CAP // windows(c))


def seam(kind, c):
    return {"bulk": K_MSM_MAX_CHUNK, "scatter": K_MSM_SCATTER_SUB, "sparse": sub_cap(c)}[kind]


def plan(c, rows, n_dense, n_extra, mode="compressed", sparse=False, force_bulk=False, host_sum=True, bulk_workgroups=K_MSM_BULK_WORKGROUPS):
    """msm_plan.h msm_plan() for a plain (no bullet, no addend) job: dict(kernel, chunk, nchunks, fuse, route)"""
    W = windows(c); lanes = K_MSM_THREADS // W
    bulk = rows * n_dense >= (1 << 16) or (force_bulk and n_dense > 0)
    if bulk:
        nchunks = max(1, (max(1, bulk_workgroups) + rows - 1) // rows)
        nchunks = min(nchunks, max(1, n_dense // lanes))
        nchunks = max(nchunks, (n_dense + K_MSM_BULK_TERMS - 1) // K_MSM_BULK_TERMS)
    else:
        per_wg = (3 if rows <= 2 else 4) * (K_MSM_THREADS // 4) // W
        terms_wg = per_wg - n_extra if per_wg > n_extra else 1
        nchunks = max(1, (n_dense + terms_wg - 1) // terms_wg)
        nchunks = min(nchunks, 256 if rows <= 2 else max(1, 2048 // rows))
        nchunks = min(nchunks, max(1, n_dense))
        nchunks = max(nchunks, (n_dense + K_SMALL_CHUNK - 1) // K_SMALL_CHUNK)
    if not n_dense:
        nchunks = 1
    chunk = (n_dense + nchunks - 1) // nchunks if n_dense else 1
    nchunks = (n_dense + chunk - 1) // chunk if n_dense else 1
    fuse = 1 if (not bulk and mode == "compressed" and rows <= 2 and rows * nchunks <= K_MSM_MAIL_CAP) else 0
    if fuse and host_sum:
        fuse = 2
    if fuse:
        route = "mail" if fuse == 2 else "flag"
    elif mode == "keep":
        route = "keep"
    elif mode == "raw":
        route = "raw"
    else:
        route = "device_encode" if rows > K_HOST_ENCODE_ROWS else "host_encode"
    return dict(kernel="bulk_sparse" if bulk and sparse and W <= 32 else "bulk" if bulk else "small", chunk=chunk, nchunks=nchunks, fuse=fuse, route=route)


# ------------------------------------------------------------------------------------------------ digits
def magnitudes(c):
    """the magnitudes the digit cases look up at every window: all of them at the narrow widths, the ends of the table row and of its
    k_table_fill blocks (T entries each) at the wide ones"""
    E, T = 1 << (c - 1), table_block(c)
    if c <= NARROW_MAX:
        return list(range(1, E + 1))
    return sorted(m for m in {1, 2, T - 1, T, T + 1, 2 * T, E - 1, E} if 1 <= m <= E)


def family(c, mags, ws=None):
    """m 2^(cw) (digit +m at w; -E and a carry for m = E) and (2^c - m) 2^(cw) (digit -m at w, +1 at w + 1), below l"""
    out = []
    for w in (range(windows(c)) if ws is None else ws):
        for m in mags:
            for s in (m << (c * w), ((1 << c) - m) << (c * w)):
                if s < L:
                    out.append(s)
    return out


def chain(c):
    """window 0 = E, windows 1 .. W-2 = E - 1: recodes to -E in every window but the top, and +1 there"""
    E = 1 << (c - 1)
    return E + sum((E - 1) << (c * w) for w in range(1, windows(c) - 1))


def top_scalars(c):
    """the largest top-window digit (l - 1 has it; so has that digit alone), 2^252 (at c = 11 the top window starts at bit 253 and its only digit
    is the carry out of bit 252), and the largest scalar below 2^252"""
    top = digits(L - 1, c)[-1]
    return [L - 1, top << (c * (windows(c) - 1)) if top > 0 and (top << (c * (windows(c) - 1))) < L else L - 2, 1 << 252, (1 << 252) - 1]


def always(c):
    return [chain(c), L - 1, 0, 1, 1 << 252] + top_scalars(c)


def entries(s, c):
    """{(window, magnitude, sign)} the scalar looks up"""
    return {(w, abs(d), 1 if d > 0 else -1) for w, d in enumerate(digits(s, c)) if d}


def reachable(c, mags=None):
    """the (window, magnitude, sign) a scalar below l can look up, from the two families, the chain and the top-window scalars;
    mags: the families of these magnitudes alone, and only entries of these magnitudes"""
    E = 1 << (c - 1)
    got = set()
    for s in family(c, range(1, E + 1) if mags is None else mags) + always(c):
        got |= entries(s, c)
    return got if mags is None else {e for e in got if e[1] in set(mags)}


def digit_scalars(c):
    """few scalars, many digits each, that between them look up reachable(c, magnitudes(c)) — all of reachable(c) at the narrow widths"""
    W, E, mags = windows(c), 1 << (c - 1), magnitudes(c)
    D = [-m for m in reversed(mags)] + [m for m in mags if m < E]
    n, out, covered = len(D), [], set()

    def add(s):
        assert 0 <= s < L
        out.append(s); covered.update(entries(s, c))

    def lower(i):                                                 # windows 0 .. W-3: scalar i takes digit D[(i + w) mod n] at window w
        return sum(D[(i + w) % n] * (1 << (c * w)) for w in range(W - 2))
    # the two top windows: not every digit fits below l there, so their configurations come from the families; the windows below ride along
    tops = sorted(set(family(c, mags, (W - 2, W - 1))))
    for i, s0 in enumerate(tops):
        s = s0 + lower(i)
        add(s if 0 <= s < L and digits(s, c)[W - 2:] == digits(s0, c)[W - 2:] else s0)
    for i in range(n):
        if all((w, abs(D[(i + w) % n]), 1 if D[(i + w) % n] > 0 else -1) in covered for w in range(W - 2)):
            continue
        s = lower(i)
        add(s + (1 << (c * (W - 2))) if s < 0 or D[(i + W - 3) % n] < 0 else s)
    for s in always(c):
        add(s)
    return out


def digit_rows(c, R):
    """rows over the R + 2 points: row i gives base b the scalar S[(i + b) mod |S|], so every base meets every scalar of digit_scalars(c)"""
    S = digit_scalars(c)
    return [[S[(i + b) % len(S)] for b in range(R + 2)] for i in range(len(S))]


def looked_up(rows, c):
    """{(base, window, magnitude, sign)} over rows of per-base scalars"""
    return {(b,) + e for row in rows for b, s in enumerate(row) for e in entries(s, c)}


def rows_job(vectors, R, name, **kw):
    """per-base vectors (length R + 2) as a job: the first R on the dense part, the last two as extras on Q (R) and h (R + 1)"""
    return dict(dict(name=name, rows=len(vectors), n_dense=R, dense=[v[:R] for v in vectors], extra_base=[R, R + 1], extra=[v[R:] for v in vectors],
                     mode="compressed", sparse=0, force_bulk=False), **kw)


def job_vectors(job, R):
    out = []
    for r in range(job["rows"]):
        v = [0] * (R + 2)
        for j, s in enumerate(job["dense"][r] if job["n_dense"] else []):
            v[j] = (v[j] + s) % L
        for b, s in zip(job["extra_base"], job["extra"][r] if job["extra_base"] else []):
            v[b] = (v[b] + s) % L
        out.append(v)
    return out


# ------------------------------------------------------------------------------------------------ seams
def full_scalar(c, rng):
    """a scalar below l whose digit is non-zero in EVERY window (the work list takes W entries for it)"""
    W, E = windows(c), 1 << (c - 1)
    assert c * (W - 1) <= 252
    ds = [rng.choice([d for d in (rng.randrange(-E, 0), rng.randrange(1, E))]) for _ in range(W - 2)] + [rng.randrange(-E, 0), 1]
    s = sum(d * (1 << (c * w)) for w, d in enumerate(ds))
    assert 0 < s < L and all(digits(s, c))
    return s


KINDS = ("full", "zero", "small", "uniform")


def seam_scalar(kind, c, rng, k):
    if kind == "full":
        return full_scalar(c, rng)
    if kind == "zero":
        return 0
    if kind == "small":
        return rng.randrange(2) if k & 1 else rng.randrange(1 << 64)
    return rng.randrange(L)


def seam_sizes(S):
    """(n_dense, n_extra): n_all = S - 1, S, S + 1, 2 S + 3, 4 S without extras or with few; then the extras wholly before the seam, wholly behind it
    (one extra alone in the next sub-chunk) and across it (four and four)"""
    return [(S - 1, 0), (S - 2, 1), (S, 0), (S - 1, 1), (S + 1, 0), (2 * S, 3), (4 * S - 5, 5), (S - 8, 8), (S, 1), (S - 4, 8)]


def seam_rows(kind, c, R, rows=3, sizes=None):
    """jobs (bulk, sparse) whose one chunk crosses the sub-chunk seam S of the kernel: sub-chunk k of row r is all zero, all full scalars (the
    work list at its cap), bits and 64-bit values, or uniform, by (k + r) mod 4; an extra term is never zero.  kind "scatter": the same sizes
    as runs of (column, scalar) pairs of one row, without extras."""
    S = seam(kind, c)
    rng = random.Random(1000 * c + len(kind))
    jobs = []
    bases = [R + 1, R, 0, 1, R + 1, 2, R, 3]
    for n_dense, n_extra in (sizes or seam_sizes(S)):
        if kind == "scatter":
            n_dense, n_extra = n_dense + n_extra, 0
            if any(j["n_dense"] == n_dense for j in jobs):
                continue
        assert n_dense <= R
        dense, extra = [], []
        for r in range(rows):
            row = []
            for t in range(n_dense + n_extra):
                what = KINDS[(t // S + r) % 4]
                if t >= n_dense and what in ("zero", "small"):
                    what = "uniform"
                s = seam_scalar(what, c, rng, t)
                row.append(s if t < n_dense or s else 1)
            dense.append(row[:n_dense]); extra.append(row[n_dense:])
        jobs.append(dict(name=f"{kind}-c{c}-{n_dense}+{n_extra}", rows=rows, n_dense=n_dense, dense=dense, extra_base=bases[:n_extra], extra=extra,
                         mode="compressed", sparse=1 if kind == "sparse" else 0, force_bulk=True))
    return S, jobs


# ------------------------------------------------------------------------------------------------ the prover's job shapes, at their smallest
def shape_jobs(R, c):
    """the launches tests/msm_plan_check.cpp pins, small: no dense part under 1, 6 and 8 extras (raw and compressed), dense parts shorter than the
    table, extras on h, on Q, twice on one base, an extra that cancels a dense term (the identity: 32 zero bytes), a row of zeros, kept sums,
    force_bulk"""
    assert R > 65
    rng = random.Random(77)                                        # the same scalars at every width: one reference serves them all
    u = lambda: rng.randrange(1, L)                                # noqa: E731
    jobs = []
    ex_bases = {1: [R + 1], 6: [R + 1, R, 0, R + 1, 5, R], 8: [R, R + 1, 1, 1, R - 1, 0, R, R + 1]}
    for rows in (1, 2, 3, 9, 164):
        for n_extra in (1, 6, 8):
            for mode in ("raw", "compressed"):
                ex = [[u() for _ in range(n_extra)] for _ in range(rows)]
                ex[rows // 2][0] = 0
                jobs.append(dict(name=f"extras-only-{rows}x{n_extra}-{mode}", rows=rows, n_dense=0, dense=[], extra_base=ex_bases[n_extra], extra=ex, mode=mode,
                                 sparse=0, force_bulk=False))
    for n_dense in (1, 2, 63, 64, 65):
        for rows, bases in ((1, [R + 1]), (2, [R]), (3, [R + 1, R + 1]), (9, [R, R + 1])):
            jobs.append(dict(name=f"short-{rows}x{n_dense}+{len(bases)}", rows=rows, n_dense=n_dense, dense=[[u() for _ in range(n_dense)] for _ in range(rows)],
                             extra_base=bases, extra=[[u() for _ in bases] for _ in range(rows)], mode="compressed", sparse=0, force_bulk=False))
    for rows in (1, 3):
        d = [[u() for _ in range(2)] for _ in range(rows)]
        jobs.append(dict(name=f"cancels-{rows}", rows=rows, n_dense=2, dense=[[x[0], 0] for x in d], extra_base=[0], extra=[[L - x[0]] for x in d],
                         mode="compressed", sparse=0, force_bulk=False, identity=True))
        jobs.append(dict(name=f"zeros-{rows}", rows=rows, n_dense=64, dense=[[0] * 64 for _ in range(rows)], extra_base=[R + 1], extra=[[0]] * rows,
                         mode="compressed", sparse=0, force_bulk=False, identity=True))
    for rows, n_dense, fb in ((2, 64, False), (64, 64, False), (3, 64, True), (3, 65, True)):
        jobs.append(dict(name=f"keep-{rows}x{n_dense}{'-bulk' if fb else ''}", rows=rows, n_dense=n_dense, dense=[[u() for _ in range(n_dense)] for _ in range(rows)],
                         extra_base=[], extra=[], mode="keep", sparse=0, force_bulk=fb))
    jobs.append(dict(name="bulk-3x64+1-sparse", rows=3, n_dense=64, dense=[[rng.randrange(1 << 64) for _ in range(64)] for _ in range(3)], extra_base=[R + 1],
                     extra=[[u()] for _ in range(3)], mode="compressed", sparse=1, force_bulk=True))
    return jobs


def small_sum_lines(run, c=8, R=16, R_shapes=128):
    """the c = 8 digit rows, one and two rows at a time, and the shape jobs of at most two compressed rows: the launches that fuse, whose chunk
    sums the host adds up by default and the last workgroup with OTTI_SMALL_HOST_SUM=0.  run(which, job) -> (points (rows, 32) uint8, plan), which =
    "digits" (the R-generator set) or "shapes" (the R_shapes one); returns lines "<name> <fuse> <hex>", the same in every process."""
    lines = []
    vectors = digit_rows(c, R)
    for step in (1, 2):
        for i in range(0, len(vectors) - step + 1, step):
            out, plan = run("digits", rows_job(vectors[i: i + step], R, f"digits-{step}-{i}"))
            lines.append(f"digits-{step}-{i} {plan['fuse']} {out.tobytes().hex()}")
    for job in shape_jobs(R_shapes, c):
        if job["rows"] <= 2 and job["mode"] == "compressed" and not job["force_bulk"]:
            out, plan = run("shapes", job)
            lines.append(f"{job['name']} {plan['fuse']} {out.tobytes().hex()}")
    return lines
