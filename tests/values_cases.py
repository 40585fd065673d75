"""Structures and coefficient sets for Instance.set_values (otti_instance_set_values), in Python integers.  Needs no GPU and nothing of the product.

A Structure is the part of an R1CS instance that set_values leaves alone — for each of A, B, C the (row, col) of every entry in caller order — with
an assignment z and three coefficient sets over it, each a list of canonical integers per matrix:
    V0   mostly small integers: A signed, B positive, and C_r the single entry (r, constant column, a_r * b_r mod l), so z satisfies it.  (The
         structure with an empty C gets b_r = 0 from a second, wide coefficient in every row of B.)
    V1   every entry of row r of A and of C times the same non-zero s_r: <A_r, z> <B_r, z> = <C_r, z> still holds for z.  scale "field": uniform
         s_r, so A and C turn wide — where V0 read coefficient codes the variant flips to no codes; scale "small": s_r in {2, 3}, A stays small and the
         variant stays.
    V2   V0 with the C coefficient of three chosen rows one more: exactly those rows fail.
The rules that pick a sparse-kernel variant are sparse_cases.SparseCase.variant's.

An update hands a matrix over in a coefficient format with a stride (coo_cases.STRIDES).  A list that the format cannot hold — a wide value in I64,
a negative one in U64 — goes as packed canonical bytes instead: plan() says which, so a test can check that the format it names was exercised."""
import random

import numpy as np

import coo_cases as cc
import sparse_cases as sc

L, R = sc.L, sc.R
BROKEN_ROWS = 3


class Structure:
    def __init__(self, name, nc, nv, ni, a_cols, b_cols, empty_c=False, a_extra=(), specials=False):
        """a_cols[r], b_cols[r]: the columns of row r's entries (caller numbering); a_extra: (row, col, value) triples put into A as they are —
        duplicates, explicit zeros; specials: the ends of the int64 range among A's first coefficients"""
        self.name, self.nc, self.nv, self.ni, self.empty_c = name, nc, nv, ni, empty_c
        self.nvp, self.ncp = sc.next_pow2(max(nv, ni + 1)), max(2, sc.next_pow2(nc))
        rng = random.Random(repr(("values", name)))
        z = sc._field(rng, nv) + [0] * (self.nvp - nv) + [1] + sc._field(rng, ni)
        self.z = z + [0] * (2 * self.nvp - len(z))
        zc = lambda c: self.z[c + self.nvp - nv if c >= nv else c]
        A, B = [], []
        for r in range(nc):
            for c in a_cols[r]:
                x = rng.randint(-1000, 1000) if rng.getrandbits(4) or specials else sc._wide(rng)   # one in sixteen is no small integer (specials: none, so that A fits int64)
                A.append((r, c, x % L))
            cols = list(b_cols[r])
            for c in cols:
                B.append((r, c, rng.randint(1, 1000)))
            if empty_c:                                           # b_r = 0: the last coefficient cancels the others
                c_last = next(c for c in range(nv) if zc(c))
                b_r = sum(v * zc(c) for rr, c, v in B if rr == r) % L
                B.append((r, c_last, -b_r * pow(zc(c_last), -1, L) % L))
        A += [(r, c, x % L) for r, c, x in a_extra]
        if specials:
            for i, x in enumerate((cc.INT64_MIN, cc.INT64_MAX, -1, 0)):
                A[i] = (A[i][0], A[i][1], x % L)
        rng.shuffle(B)                                            # caller order is no row order
        self.pos = [[(r, c) for r, c, _ in A], [(r, c) for r, c, _ in B], [] if empty_c else [(r, nv) for r in range(nc)]]
        a = self._row_sums(0, [x for _, _, x in A])
        b = self._row_sums(1, [x for _, _, x in B])
        self.V0 = [[x for _, _, x in A], [x for _, _, x in B], [] if empty_c else [a[r] * b[r] % L for r in range(nc)]]
        assert not empty_c or not any(b)
        self.broken = [] if empty_c else sorted(random.Random(repr(("broken", name))).sample(range(nc), min(BROKEN_ROWS, nc)))

    def _row_sums(self, k, vals):
        acc = [0] * self.nc
        for (r, c), v in zip(self.pos[k], vals):
            acc[r] += v * self.z[c + self.nvp - self.nv if c >= self.nv else c]
        return [x % L for x in acc]

    def dims(self):
        return self.nc, self.nv, self.ni

    def nnz(self):
        return [len(p) for p in self.pos]

    def snark_n(self):
        return max(2, sc.next_pow2(max(self.nnz())))

    # ---- coefficient sets
    def V1(self, scale):
        rng = random.Random(repr(("scale", self.name, scale)))
        s = [rng.choice((2, 3)) if scale == "small" else rng.randrange(1, L) for _ in range(self.nc)]
        return [[v * s[r] % L for (r, _), v in zip(self.pos[0], self.V0[0])], list(self.V0[1]), [v * s[r] % L for (r, _), v in zip(self.pos[2], self.V0[2])]]

    def V2(self):
        assert self.broken
        return [list(self.V0[0]), list(self.V0[1]), [(v + (r in self.broken)) % L for (r, _), v in zip(self.pos[2], self.V0[2])]]

    def satisfied(self, vals):
        a, b, c = (self._row_sums(k, vals[k]) for k in range(3))
        return [r for r in range(self.nc) if a[r] * b[r] % L != c[r]]

    # ---- what goes to the product
    def triples(self, vals):
        return [[(r, c, v) for (r, c), v in zip(self.pos[k], vals[k])] for k in range(3)]

    def entry_arrays(self, vals):
        return [sc.entry_array(m) for m in self.triples(vals)]

    def coo(self, vals):
        """[(rows, cols, vals)] * 3 for Instance.from_coo: u32 indices, packed canonical bytes"""
        return cc.CooCase(self.name, self.nc, self.nv, self.ni, self.triples(vals), cc.IDX_U32, cc.C32).arrays()

    def sparse(self, vals):
        """the instance with these coefficients as a sparse_cases.SparseCase: variants and the integer reference of the products"""
        rng = random.Random(repr(("values-vectors", self.name)))
        return sc.SparseCase(self.name, self.nc, self.nv, self.ni, self.triples(vals), self.z, sc._field(rng, self.ncp), sc._field(rng, 3), None, False, None)

    def vars32(self):
        return sc.bytes32(self.z[:self.nv])

    def inputs32(self):
        return sc.bytes32(self.z[self.nvp + 1:self.nvp + 1 + self.ni])


# ------------------------------------------------------------------------------------------------ one list in a coefficient format
def fits(val_format, xs):
    if val_format == cc.I64:
        return all(x < 2 ** 63 or L - x <= 2 ** 63 for x in xs)
    if val_format == cc.U64:
        return all(x < 2 ** 64 for x in xs)
    return True


def value_list(val_format, stride, xs, raw_of=None):
    """(array, format used): canonical integers xs in val_format at `stride`, or — a list the format cannot hold — as packed canonical bytes.
    raw_of(canonical values) -> Montgomery words replaces this module's own arithmetic for MONTGOMERY32"""
    if not fits(val_format, xs):
        val_format, stride = cc.C32, 32
    if val_format == cc.I64:
        raws = [x if x < 2 ** 63 else x - L for x in xs]
    elif val_format == cc.M32:
        raws = raw_of(xs) if raw_of is not None else [x * R % L for x in xs]
    else:
        raws = xs
    return cc.value_array(val_format, raws, stride), val_format


def plan(val_format, vals):
    """the format each matrix of an update travels in"""
    return [val_format if fits(val_format, xs) else cc.C32 for xs in vals]


def format_params():
    return [(v, s) for v in cc.VAL_FORMATS for s in cc.STRIDES[v]]


# ------------------------------------------------------------------------------------------------ the structures, built once
def _rows(rng, nc, n_cols, per_row):
    return [rng.sample(range(n_cols), per_row(r)) for r in range(nc)]


def _build():
    out = {}

    def add(name, nc, nv, ni, a_per_row, b_per_row, **kw):
        rng = random.Random(repr(("structure", name)))
        n_cols = nv + 1 + ni
        out[name] = Structure(name, nc, nv, ni, _rows(rng, nc, n_cols, a_per_row), _rows(rng, nc, n_cols, b_per_row), **kw)

    add("padded40", 5, 5, 1, lambda r: 4, lambda r: 3)                                     # ~40 entries; nvp = 8, ncp = 8
    add("emptyC", 6, 6, 1, lambda r: 2, lambda r: 1, empty_c=True)
    add("dups_zeros", 7, 9, 2, lambda r: 3, lambda r: 2,
        a_extra=[(2, 3, 5), (2, 3, 5), (2, 3, -4), (4, 0, 0), (0, 9, 0), (6, 11, 7), (6, 11, 7)])   # a pair three times, explicit zeros, the constant and the last input
    add("heavy", 80, 2200, 2, lambda r: 2060 if r == 70 else 65 if r == 3 else 2, lambda r: 1)     # kHeavyRow and kHeavySeg seams by row; C: the constant column on 80 rows
    add("quad1280", 128, 60, 3, lambda r: 5, lambda r: 4, specials=True)                   # 1280 entries, ten per row: quad, codes under V0; SNARK N = 2^10
    add("n2", 2, 2, 1, lambda r: 1, lambda r: 1)
    add("n4", 3, 3, 1, lambda r: 2 if r == 0 else 1, lambda r: 1)
    add("n8", 4, 4, 1, lambda r: 2, lambda r: 1)
    return out


STRUCTURES = _build()
SNARK_STRUCTURES = ("n2", "n4", "n8", "quad1280")
assert [STRUCTURES[n].snark_n() for n in SNARK_STRUCTURES] == [2, 4, 8, 1024]
assert max(STRUCTURES["heavy"].sparse(STRUCTURES["heavy"].V0).lengths(False).max(axis=0)) > sc.HEAVY_SEG
assert STRUCTURES["heavy"].sparse(STRUCTURES["heavy"].V0).lengths(True).max() > sc.HEAVY_ROW


def scales(name):
    """the V1 scalings worth running on a structure: both where the codes rule can fire"""
    return ("field", "small") if sum(STRUCTURES[name].nnz()) >= sc.CODES_MIN_ENTRIES else ("field",)
