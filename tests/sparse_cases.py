"""Hand-built R1CS instances for the sparse kernels (k_sparse.hip) and their reference in Python integers.  Needs no GPU and nothing of the product.

Every builder returns a SparseCase: the three entry lists in the caller's numbering, the vectors the products are taken with, the kernel
variant the instance is BUILT to reach (layout, coefficient path) and, on demand, the expected outputs.  All arithmetic is exact in GF(l):
    multiply_vec        Az[r]   = sum over A's entries (r, c, v) of v * z[c']         c' = c shifted by the variable padding, as Instance::new does
    eval_table_sparse   T[c']   = sum_k coef_k * sum over M_k's entries (r, c, v) of v * eq[r]
    satisfiability      row r fails when Az[r] * Bz[r] mod l != Cz[r]
The rules that pick a variant are restated here from their definition (entries per row and matrix >= 3: a row per quad; at least 1024 entries
of which at least half are integers of magnitude <= 2^31 - 2: coefficient codes; a list longer than 64: the segmented path in segments of 2048),
so a test can hold what the device reports against what the instance was built for."""
import random

import numpy as np

L = 2 ** 252 + 27742317777372353535851937790883648493
R = (1 << 256) % L
R_INV = pow(R, -1, L)
ENTRY_DTYPE = np.dtype([("row", "<u8"), ("col", "<u8"), ("val", "u1", (32,))])
HEAVY_ROW, HEAVY_SEG, CODES_MIN_ENTRIES, QUAD_AVG_ROW, CODE_MAX = 64, 2048, 1024, 3.0, 2 ** 31 - 2

LADDER = (0, 1, 3, 4, 5, 63, 64, 65, 2047, 2048, 2049, 4096, 4097)
MIXES = ("codes", "nocodes", "codes_with_wide", "wide_with_codes")


def is_small(v):
    """the coefficient is an integer c with |c| <= 2^31 - 2 (zero included): it travels as a 4-byte code"""
    v %= L
    return v <= CODE_MAX or L - v <= CODE_MAX


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def _rng(*key):
    return random.Random(repr(key))                               # seeded by the case's own name: a case is the same wherever it is built


def _wide(rng):
    """a uniform value below 2^252 that is no small integer either way"""
    while True:
        v = rng.getrandbits(252)
        if not is_small(v):
            return v


def _code(rng):
    """a non-zero small integer, either sign; one in eight at the largest magnitude"""
    mag = CODE_MAX if rng.getrandbits(3) == 0 else rng.randint(1, CODE_MAX)
    return mag if rng.getrandbits(1) else L - mag


def _field(rng, n):
    return [rng.getrandbits(320) % L for _ in range(n)]


def mont_words(ints):
    """the Montgomery words (what the kernels hold and multiply) of canonical integers"""
    return [x % L * R % L for x in ints]


def from_mont_words(words):
    return [w * R_INV % L for w in words]


def entry_array(ents):
    e = np.zeros(len(ents), dtype=ENTRY_DTYPE)
    if ents:
        e["row"] = [t[0] for t in ents]
        e["col"] = [t[1] for t in ents]
        e["val"] = np.frombuffer(b"".join((t[2] % L).to_bytes(32, "little") for t in ents), dtype=np.uint8).reshape(-1, 32)
    return e


def bytes32(ints):
    return np.frombuffer(b"".join((x % L).to_bytes(32, "little") for x in ints), dtype=np.uint8).reshape(-1, 32).copy()


class SparseCase:
    """ents[k]: list of (row, col, value) of matrix k in the caller's numbering; z: 2 * nvp integers (vars || 0.. || z[nvp] || inputs || 0..);
    eq: ncp integers; coef: 3 integers.  layout / codes: what the instance is built to reach, for the by-row set (layout_col for the by-column one;
    None: not built for either)."""

    def __init__(self, name, nc, nv, ni, ents, z, eq, coef, layout, codes, layout_col="lane"):
        self.name, self.nc, self.nv, self.ni, self.ents = name, nc, nv, ni, ents
        self.nvp, self.ncp = next_pow2(max(nv, ni + 1)), max(2, next_pow2(nc))
        self.z, self.eq, self.coef = [x % L for x in z], [x % L for x in eq], [x % L for x in coef]
        assert len(self.z) == 2 * self.nvp and len(self.eq) == self.ncp and len(self.coef) == 3
        self.layout, self.codes, self.layout_col = layout, codes, layout_col
        for m in ents:
            assert all(0 <= r < nc and 0 <= c < nv + 1 + ni and 0 <= v < L for r, c, v in m)

    # ---- what goes to Instance::new and to the kernels
    def arrays(self):
        return [entry_array(m) for m in self.ents]

    def col_shifted(self, c):
        return c + self.nvp - self.nv if c >= self.nv else c

    def vars32(self):
        return bytes32(self.z[:self.nv])

    def inputs32(self):
        return bytes32(self.z[self.nvp + 1:self.nvp + 1 + self.ni])

    def is_assignment(self):
        """z is the vector an uploaded assignment gives: zero padding, the constant 1, inputs, zero padding"""
        z, nvp = self.z, self.nvp
        return not any(z[self.nv:nvp]) and z[nvp] == 1 and not any(z[nvp + 1 + self.ni:])

    # ---- the rules that pick a variant, from the entry lists alone
    def lengths(self, by_col=False):
        """(3, rows) list lengths of the by-row or the by-column set"""
        rows = 2 * self.nvp if by_col else self.ncp
        out = np.zeros((3, rows), dtype=np.int64)
        for k, m in enumerate(self.ents):
            major = [self.col_shifted(c) for _, c, _ in m] if by_col else [r for r, _, _ in m]
            if major:
                out[k] = np.bincount(np.array(major, dtype=np.int64), minlength=rows)
        return out

    def counts(self):
        total = sum(len(m) for m in self.ents)
        return total, sum(is_small(v) for m in self.ents for _, _, v in m)

    def variant(self, by_col=False):
        """dict(rows, entries, use_small, quad, n_heavy, n_seg) by the rules quoted in the module docstring"""
        ln = self.lengths(by_col)
        total, n_small = self.counts()
        longest = ln.max(axis=0)
        heavy = longest[longest > HEAVY_ROW]
        return dict(rows=ln.shape[1], entries=tuple(len(m) for m in self.ents), use_small=total >= CODES_MIN_ENTRIES and 2 * n_small >= total,
                    quad=total / (3.0 * ln.shape[1]) >= QUAD_AVG_ROW, n_heavy=len(heavy), n_seg=int(sum(-(-int(x) // HEAVY_SEG) for x in heavy)))

    # ---- the integer reference
    def multiply_vec(self, z=None):
        z = self.z if z is None else z
        out = []
        for m in self.ents:
            acc = [0] * self.ncp
            for r, c, v in m:
                acc[r] += v * z[self.col_shifted(c)]
            out.append([x % L for x in acc])
        return out

    def eval_table(self):
        acc = [0] * (2 * self.nvp)
        for k, m in enumerate(self.ents):
            for r, c, v in m:
                acc[self.col_shifted(c)] += self.coef[k] * v * self.eq[r]
        return [x % L for x in acc]

    def eval_tables(self):
        """the three tables apart (what the oracle returns)"""
        out = []
        for m in self.ents:
            acc = [0] * (2 * self.nvp)
            for r, c, v in m:
                acc[self.col_shifted(c)] += v * self.eq[r]
            out.append([x % L for x in acc])
        return out

    def failing(self):
        """(failing rows ascending, {row: (a, b, c)})"""
        a, b, c = self.multiply_vec()
        rows = [r for r in range(self.ncp) if a[r] * b[r] % L != c[r]]
        return rows, {r: (a[r], b[r], c[r]) for r in rows}


# ------------------------------------------------------------------------------------------------ coefficient mixes
def _coefficient(rng, mix, row, p):
    """entry p of a list in major index `row` under a mix.  The quarter of the other kind sits at p = row (mod 4): in every list of four or more"""
    other = (p - row) % 4 == 0
    if mix == "codes" or (mix == "codes_with_wide" and not other) or (mix == "wide_with_codes" and other):
        return _code(rng)
    return _wide(rng)


def _vectors(rng, ncp, nvp, nv, ni):
    """z as an assignment gives it (so the same case serves check_sat), eq and the three combination coefficients; a few words at the ends of the range"""
    z = _field(rng, nv) + [0] * (nvp - nv) + [1] + _field(rng, ni)
    z += [0] * (2 * nvp - len(z))
    eq = _field(rng, ncp)
    for vec, n in ((z, nv), (eq, ncp)):
        for i, w in enumerate((0, 1, L - 1, 2 ** 252 - 1, 2 ** 252, 2 ** 252 + 1)):
            if 2 * i + 1 < n:
                vec[2 * i + 1] = w * R_INV % L                 # the kernel's word there is w itself
    return z, eq, _field(rng, 3)


# rows (columns, in the transposed twin) of the ladder: the long lists at bit 0 and bit 63 of a word, at both ends of one word and in the last row,
# the short ones beside them so that a wave, and in the quad layout a quad's neighbours, hold lists of every kind
def ladder_places(n_major):
    last = n_major - 1
    return {0: 4097, 63: 65, 64: 2049, 127: 2048, last: 4096, 130: 2047, 2: 0, 5: 1, 6: 3, 7: 4, 9: 5, 65: 63, 66: 64}


def _distinct(rng, n_minor, n):
    return rng.sample(range(n_minor), n)


def ladder_case(layout, which, mix, transposed=False):
    """One matrix (`which` = 0, 1, 2) carries lists of the LADDER lengths over distinct minor indices; the others one entry per major index (four in
    the quad layout, whose filler lists are all four long).  transposed: the ladder runs over COLUMNS (the by-column set sees the lengths) and
    every constraint row holds about one entry."""
    nv, ni = 1 << 13, 3
    nc = 1 << 13 if (layout == "lane" or transposed) else 1 << 10
    assert not (transposed and layout != "lane")
    rng = _rng("ladder", layout, which, mix, transposed)
    n_cols = nv + 1 + ni
    n_major, n_minor = (n_cols, nc) if transposed else (nc, n_cols)
    places = ladder_places(n_major if not transposed else nv)   # transposed: among the variable columns (the last one: column nv - 1)
    fill = 4 if layout == "quad" else 1
    ents = [[], [], []]
    for k in range(3):
        for j in range(n_major):
            n = places.get(j, fill) if k == which else fill
            for p, i in enumerate(_distinct(rng, n_minor, n)):
                v = _coefficient(rng, mix, j, p)
                ents[k].append((i, j, v) if transposed else (j, i, v))
    # a repeated (row, col) pair and an explicit zero: Instance::new keeps both
    r0, c0 = (3, 11)
    ents[which] += [(r0, c0, _coefficient(rng, mix, r0, 1)), (r0, c0, _coefficient(rng, mix, r0, 2)), (r0, c0 + 1, 0)]
    z, eq, coef = _vectors(rng, nc, nv, nv, ni)
    name = "%s%s-%s-%s" % ("cols-" if transposed else "", layout, "ABC"[which], mix)
    return SparseCase(name, nc, nv, ni, ents, z, eq, coef, layout, mix in ("codes", "codes_with_wide"))


def ladder_params():
    return [(layout, which, mix, tr) for layout, tr in (("lane", False), ("quad", False), ("lane", True)) for which in range(3) for mix in MIXES]


def column_quad_case(mix):
    """The by-column set in the quad layout: 2^10 variables whose columns hold 5 .. 9 entries per matrix over distinct rows (none long), nothing in
    the padded half but the constant column and the inputs."""
    nc, nv, ni = 1 << 10, 1 << 10, 3
    rng = _rng("colquad", mix)
    ents = [[], [], []]
    for k in range(3):
        for c in range(nv + 1 + ni):
            for p, r in enumerate(_distinct(rng, nc, 5 + (c + k) % 5)):
                ents[k].append((r, c, _coefficient(rng, mix, c, p)))
    z, eq, coef = _vectors(rng, nc, nv, nv, ni)
    return SparseCase("colquad-" + mix, nc, nv, ni, ents, z, eq, coef, "quad", mix in ("codes", "codes_with_wide"), layout_col="quad")


# ------------------------------------------------------------------------------------------------ the ends of the code path
EDGE_COEFS = [0, 1, L - 1, 2, L - 2, CODE_MAX, L - CODE_MAX, 2 ** 31 - 1, L - (2 ** 31 - 1), 2 ** 31, L - 2 ** 31, 2 ** 32 - 1, (L + 1) // 2, (L - 1) // 2]
EDGE_MAGS = [2, 3, 5, 7, 1000, 65537, 2 ** 24 + 3, 2 ** 30 + 1, 2 ** 31 - 3, CODE_MAX]


def overshoot_words():
    """(m, w) with w * m mod 2^252 < m: the product's bits from 252 up, the quotient estimate of the small-integer product, are floor(w m / l) + 1"""
    out = []
    for m in EDGE_MAGS:
        for k in sorted({1, 2, 3, m // 3, m // 2, m - 2, m - 1}):
            if k < 1 or (k << 252) % m == 0:
                continue
            w = ((k << 252) // m) + 1
            assert w < L and w * m % 2 ** 252 < m
            out.append((m, w))
    return out


def edge_words():
    return [0, 1, L - 1, L - 2, 2 ** 252 - 1, 2 ** 252, 2 ** 252 + 1] + [w for _, w in overshoot_words()]


def code_edge_case(layout):
    """Every edge coefficient and every +-m of EDGE_MAGS against every edge word, by row (z) and by column (eq): entry (i, i, c) for word i, dealt
    round robin to A, B, C — word i's row and column hold all of them, codes and wide values side by side.  lane: 2^10 rows; quad: 64."""
    words = edge_words()
    n = 1 << 10 if layout == "lane" else 64
    assert len(words) <= n - 1
    nc, nv, ni = n, n, 2
    rng = _rng("code-edge", layout)
    coefs = EDGE_COEFS + [x for m in EDGE_MAGS for x in (m, L - m)]
    ents, k = [[], [], []], 0
    for i in range(len(words)):
        for c in coefs:
            ents[k % 3].append((i, i, c))
            k += 1
    z = from_mont_words(words) + _field(rng, nv - len(words)) + [1] + _field(rng, ni)
    z += [0] * (2 * nv - len(z))
    eq = from_mont_words(words) + _field(rng, nc - len(words))
    return SparseCase("code-edge-" + layout, nc, nv, ni, ents, z, eq, _field(rng, 3), layout, True, layout_col=layout)


def boundary_case(layout, total, n_small):
    """`total` entries of which exactly `n_small` are small integers, scattered; the flag is total >= 1024 and 2 * n_small >= total"""
    n = 256 if layout == "lane" else 64
    nc, nv, ni = n, n, 2
    rng = _rng("boundary", layout, total, n_small)
    small = set(rng.sample(range(total), n_small))
    ents = [[], [], []]
    for e in range(total):
        ents[e % 3].append((rng.randrange(nc), rng.randrange(nv + 1 + ni), _code(rng) if e in small else _wide(rng)))
    z, eq, coef = _vectors(rng, nc, nv, nv, ni)
    return SparseCase("boundary-%s-%d-%d" % (layout, total, n_small), nc, nv, ni, ents, z, eq, coef, layout, total >= 1024 and 2 * n_small >= total,
                      layout_col="lane")


BOUNDARIES = ((1023, 1023), (1024, 512), (1024, 511))


# ------------------------------------------------------------------------------------------------ satisfiable by construction
class SatLadder:
    """A carries the ladder, B the filler lists, and C_r is the single entry (constant column, a_r * b_r mod l): every row holds.  with_failing(rows)
    gives the case whose C coefficients of those rows are one more: exactly they fail."""

    def __init__(self, layout, codes, nc=None, nv=None):
        rng = _rng("sat", layout, codes, nc)
        tiny = nc is not None
        self.nc, self.nv, self.ni = (nc, nv, 1) if tiny else (1 << 13 if layout == "lane" else 1 << 10, 1 << 13, 3)
        n_cols = self.nv + 1 + self.ni
        places = {} if tiny else ladder_places(self.nc)
        fill = 4 if layout == "quad" else 1
        mix = "codes" if codes else "nocodes"
        self.A, self.B = [], []
        for r in range(self.nc):
            for m, n in ((self.A, places.get(r, fill + (r & 1) if tiny else fill)), (self.B, fill + 1 if tiny else fill)):
                for p, c in enumerate(_distinct(rng, n_cols, n)):
                    m.append((r, c, _coefficient(rng, mix, r, p)))
        self.layout, self.codes = layout, codes and not tiny     # below 1024 entries the codes are off whatever the coefficients
        nvp = next_pow2(max(self.nv, self.ni + 1))
        self.z = _field(rng, self.nv) + [0] * (nvp - self.nv) + [1] + _field(rng, self.ni)
        self.z += [0] * (2 * nvp - len(self.z))
        self.eq, self.coef = _field(rng, max(2, next_pow2(self.nc))), _field(rng, 3)
        base = SparseCase("sat", self.nc, self.nv, self.ni, [self.A, self.B, []], self.z, self.eq, self.coef, layout, codes)
        a, b, _ = base.multiply_vec()
        self.ab = [a[r] * b[r] % L for r in range(self.nc)]
        self.heavy_rows = sorted(r for r, n in places.items() if n > HEAVY_ROW)

    def with_failing(self, rows):
        bad = set(rows)
        C = [(r, self.nv, (self.ab[r] + (r in bad)) % L) for r in range(self.nc)]
        name = "sat-%s-%s-%d" % (self.layout, "codes" if self.codes else "nocodes", self.nc)
        return SparseCase(name, self.nc, self.nv, self.ni, [self.A, self.B, C], self.z, self.eq, self.coef, self.layout, self.codes,
                          layout_col="lane" if self.heavy_rows else None)   # the tiny instances are built for the by-row set alone

    def failing_sets(self):
        """name -> rows.  The long rows sit at 0, 63, 64, 127, 130 and the last row (ladder_places)."""
        nc, last = self.nc, self.nc - 1
        if not self.heavy_rows:                                   # the tiny instances: one partly filled word
            return {"none": [], "first": [0], "last": [last], "all": list(range(nc))}
        return {"none": [], "heavy_bit0": [0], "heavy_bit63": [63], "last_row": [last], "heavy_with_light": [64, 65, 66, 70, 100],
                "heavy_passes_alone": list(range(65, 128)), "all": list(range(nc))}
