"""R1CS instances as row / column / coefficient arrays (Instance.from_coo) and what they have to become, in Python integers.  Needs no GPU and nothing
of the product.

A CooCase holds, per matrix, the triples (row, col, x) in the caller's numbering — x the NUMBER the coefficient array holds: a signed integer for
I64, an unsigned one for U64, the canonical value for the two 32-byte formats — one index format and one coefficient format with its stride.
From them: the nine arrays from_coo takes (arrays), the otti_entry arrays Instance.new takes for the same triples (entry_arrays), and the lists the
instance keeps, (row, padded column, canonical value) in caller order (expected): the column of a triple at or behind num_vars moves up by the
padding of the variable block, and an I64 number x < 0 is l - |x|."""
import random

import numpy as np

import sparse_cases as sc

L, R = sc.L, sc.R
IDX_U32, IDX_I32, IDX_U64, IDX_I64 = 0, 1, 2, 3
C32, M32, I64, U64 = 0, 1, 2, 3
INDEX_DTYPE = {IDX_U32: np.uint32, IDX_I32: np.int32, IDX_U64: np.uint64, IDX_I64: np.int64}
INDEX_FORMATS, VAL_FORMATS = (IDX_U32, IDX_I32, IDX_U64, IDX_I64), (C32, M32, I64, U64)
STRIDES = {C32: (32, 40, 64), M32: (32, 40, 64), I64: (8, 16), U64: (8, 16)}
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
SPECIALS = {I64: (-1, INT64_MIN, INT64_MAX, 0, 1), U64: (2 ** 64 - 1, 0, 1), C32: (0, L - 1, 1), M32: (0, L - 1, 1)}
BAD_ARG, INVALID_INDEX, INVALID_SCALAR = -21, -6, -5
MSG_ROW, MSG_COL, MSG_SCALAR = "row index out of range", "column index out of range", "non-canonical scalar in matrix"
WORKGROUP_SEAMS = (0, 1, 255, 256, 257, 513)


def canonical(val_format, x):
    """the field element a coefficient array's number x stands for"""
    return x % L


def raw_word(val_format, x):
    """the integer whose 32 little-endian bytes a 32-byte format's array holds for the canonical value x"""
    return x * R % L if val_format == M32 else x


def index_array(index_format, ints):
    """numbers -> the index array; a number outside the dtype's range wraps round (how a test writes -1 into an unsigned array on purpose: it does not)"""
    dt = np.dtype(INDEX_DTYPE[index_format])
    bits = 8 * dt.itemsize
    wrapped = [int(x) & (2 ** bits - 1) for x in ints]
    return np.array(wrapped, dtype=np.dtype("u%d" % dt.itemsize)).view(dt)


def value_array(val_format, raws, stride=0):
    """raws: for the integer formats the numbers themselves, for the 32-byte formats the RAW words (raw_word).  A view with `stride` bytes between
    elements (0: packed) into a buffer filled with 0xa5 elsewhere"""
    n = len(raws)
    if val_format in (I64, U64):
        stride = stride or 8
        assert stride % 8 == 0
        buf = np.full(max(1, n) * (stride // 8), 0xa5a5a5a5a5a5a5a5, dtype=np.uint64)
        view = buf[:n * (stride // 8):stride // 8] if n else buf[:0]
        view[:] = np.array([int(x) & (2 ** 64 - 1) for x in raws], dtype=np.uint64)
        return view.view(np.int64) if val_format == I64 else view
    stride = stride or 32
    buf = np.full((n, stride), 0xa5, dtype=np.uint8)
    view = buf[:, :32]
    if n:
        view[:] = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in raws), dtype=np.uint8).reshape(n, 32)
    return view


class CooCase:
    def __init__(self, name, nc, nv, ni, triples, index_format=IDX_I64, val_format=I64, stride=0):
        self.name, self.nc, self.nv, self.ni, self.triples = name, nc, nv, ni, triples
        self.index_format, self.val_format, self.stride = index_format, val_format, stride
        self.nvp, self.ncp = sc.next_pow2(max(nv, ni + 1)), max(2, sc.next_pow2(nc))

    def dims(self):
        return self.nc, self.nv, self.ni

    def arrays(self, raw_of=None):
        """[(rows, cols, vals)] * 3 for from_coo.  raw_of(canonical values) -> raw words replaces this module's own arithmetic for MONTGOMERY32"""
        out = []
        for m in self.triples:
            xs = [x for _, _, x in m]
            if self.val_format == M32 and raw_of is not None:
                raws = raw_of(xs)
            else:
                raws = [raw_word(self.val_format, x) for x in xs] if self.val_format in (C32, M32) else xs
            out.append((index_array(self.index_format, [r for r, _, _ in m]), index_array(self.index_format, [c for _, c, _ in m]),
                        value_array(self.val_format, raws, self.stride)))
        return out

    def entry_arrays(self):
        return [sc.entry_array([(r, c, canonical(self.val_format, x)) for r, c, x in m]) for m in self.triples]

    def col_shifted(self, c):
        return c + self.nvp - self.nv if c >= self.nv else c

    def col_unshifted(self, c):
        return c - (self.nvp - self.nv) if c >= self.nvp else c

    def expected(self, k):
        return [(r, self.col_shifted(c), canonical(self.val_format, x)) for r, c, x in self.triples[k]]

    def sparse(self):
        """the same instance as a sparse_cases.SparseCase with vectors of its own: the integer reference of multiply_vec"""
        rng = random.Random(repr(("coo-vectors", self.name)))
        z = sc._field(rng, self.nv) + [0] * (self.nvp - self.nv) + [1] + sc._field(rng, self.ni)
        z += [0] * (2 * self.nvp - len(z))
        ents = [[(r, c, canonical(self.val_format, x)) for r, c, x in m] for m in self.triples]
        return sc.SparseCase(self.name, self.nc, self.nv, self.ni, ents, z, sc._field(rng, self.ncp), sc._field(rng, 3), None, False, None)


def _number(rng, val_format, i):
    """coefficient i of a list: the format's special numbers first, then a mix of small and wide ones"""
    sp = SPECIALS[val_format]
    if i < len(sp):
        return sp[i]
    if val_format == I64:
        return rng.choice((rng.randint(-1000, 1000), rng.randint(INT64_MIN, INT64_MAX)))
    if val_format == U64:
        return rng.choice((rng.randint(0, 1000), rng.getrandbits(64)))
    return rng.choice((rng.randint(0, 1000), L - rng.randint(1, 1000), rng.getrandbits(300) % L))


def _triples(rng, nc, nv, ni, n, val_format):
    return [(rng.randrange(nc), rng.randrange(nv + 1 + ni), _number(rng, val_format, i)) for i in range(n)]


def count_case(nA, nB, nC, nc=37, nv=29, ni=3, index_format=IDX_I64, val_format=I64, stride=0):
    rng = random.Random(repr(("count", nA, nB, nC, index_format, val_format, stride)))
    name = "count-%d-%d-%d-i%d-v%d-s%d" % (nA, nB, nC, index_format, val_format, stride)
    return CooCase(name, nc, nv, ni, [_triples(rng, nc, nv, ni, n, val_format) for n in (nA, nB, nC)], index_format, val_format, stride)


def count_params():
    """every seam of a 256-thread workgroup in every matrix, and an empty A beside full B and C"""
    return [(n, WORKGROUP_SEAMS[(i + 1) % 6], WORKGROUP_SEAMS[(i + 2) % 6]) for i, n in enumerate(WORKGROUP_SEAMS)] + [(0, 513, 257), (0, 0, 0)]


def format_params():
    return [(i, v, s) for i in INDEX_FORMATS for v in VAL_FORMATS for s in STRIDES[v]]


def format_case(index_format, val_format, stride):
    return count_case(257, 257, 257, index_format=index_format, val_format=val_format, stride=stride)


PADDINGS = [(nv, ni, nc) for nv, ni in ((3, 5), (5, 1), (8, 0), (0, 3)) for nc in (1, 5)]


def padding_case(nv, ni, nc):
    """entries at the columns either side of the shift: num_vars - 1 (where there is one), num_vars (the constant) and num_vars + num_inputs (the last)"""
    rng = random.Random(repr(("padding", nv, ni, nc)))
    cols = [c for c in (nv - 1, nv, nv + ni, 0) if 0 <= c < nv + 1 + ni]
    triples = [[(rng.randrange(nc), c, rng.randint(-9, 9)) for c in cols] + [(nc - 1, cols[k % len(cols)], 7 + k)] for k in range(3)]
    return CooCase("padding-%d-%d-%d" % (nv, ni, nc), nc, nv, ni, triples, IDX_I32, I64)


def order_case():
    """a shuffled entry order, a (row, col) pair given three times and explicit zeros: all kept as Instance.new keeps them"""
    rng = random.Random("order")
    nc, nv, ni = 19, 23, 2
    triples = []
    for k in range(3):
        m = [(r, c, rng.randint(-5, 5) or 1) for r in range(nc) for c in rng.sample(range(nv + 1 + ni), 3)]
        rng.shuffle(m)
        m[5:5] = [(4, 11, 3), (4, 11, 3), (4, 11, -2), (6, 2, 0), (0, nv, 0)]
        triples.append(m)
    return CooCase("order", nc, nv, ni, triples, IDX_U32, I64)


def from_sparse(case, index_format=IDX_U32):
    """a sparse_cases.SparseCase through the new route: canonical coefficients, packed"""
    c = CooCase("coo-" + case.name, case.nc, case.nv, case.ni, case.ents, index_format, C32)
    return c


# ------------------------------------------------------------------------------------------------ refusals
def _with(case, k, pos, row=None, col=None):
    """case with matrix k's entry at pos given another row / column number (written into the index array as it is)"""
    r, c, x = case.triples[k][pos]
    case.triples[k][pos] = (r if row is None else row, c if col is None else col, x)


def error_cases():
    """[(name, arrays-builder, code, message)]: the builder returns (dims, [(rows, cols, vals)] * 3).  The non-canonical words are written into the
    value arrays directly: a CooCase holds canonical values only."""
    out = []

    def add(name, index_format, val_format, edit, code, msg, n=700):
        def build(index_format=index_format, val_format=val_format, edit=edit):
            case = count_case(n, n, n, index_format=index_format, val_format=val_format)
            patches = edit(case) or []
            arrays = case.arrays()
            for k, pos, raw in patches:
                arrays[k][2][pos] = np.frombuffer(int(raw).to_bytes(32, "little"), dtype=np.uint8)
            return case.dims(), arrays
        out.append((name, build, code, msg))

    nc, ncols = 37, 29 + 1 + 3
    add("bad_row", IDX_I64, C32, lambda c: _with(c, 1, 10, row=nc), INVALID_INDEX, MSG_ROW)
    add("bad_col", IDX_U32, I64, lambda c: _with(c, 2, 699, col=ncols), INVALID_INDEX, MSG_COL)
    add("bad_scalar", IDX_I32, C32, lambda c: [(0, 0, L)], INVALID_SCALAR, MSG_SCALAR)
    add("all_three_in_one_entry", IDX_I64, C32, lambda c: (_with(c, 0, 77, row=nc + 5, col=ncols + 5), [(0, 77, L + 1)])[1], INVALID_INDEX, MSG_ROW)
    add("col_and_scalar_in_one_entry", IDX_I64, C32, lambda c: (_with(c, 0, 77, col=ncols), [(0, 77, 2 ** 256 - 1)])[1], INVALID_INDEX, MSG_COL)
    add("positions_600_and_3", IDX_U64, C32, lambda c: (_with(c, 1, 600, row=nc), [(1, 3, L)])[1], INVALID_SCALAR, MSG_SCALAR)
    add("positions_3_and_600", IDX_U64, C32, lambda c: (_with(c, 1, 3, col=2 ** 40), [(1, 600, L)])[1], INVALID_INDEX, MSG_COL)
    add("scalar_in_A_before_row_in_C", IDX_I64, C32, lambda c: (_with(c, 2, 0, row=nc), [(0, 300, L)])[1], INVALID_SCALAR, MSG_SCALAR)
    add("minus_one_row_i32", IDX_I32, I64, lambda c: _with(c, 0, 256, row=-1), INVALID_INDEX, MSG_ROW)
    add("minus_one_col_i32", IDX_I32, I64, lambda c: _with(c, 0, 255, col=-1), INVALID_INDEX, MSG_COL)
    add("minus_one_row_i64", IDX_I64, I64, lambda c: _with(c, 2, 1, row=-1), INVALID_INDEX, MSG_ROW)
    add("minus_one_col_i64", IDX_I64, U64, lambda c: _with(c, 2, 1, col=-1), INVALID_INDEX, MSG_COL)
    add("int32_min_row", IDX_I32, I64, lambda c: _with(c, 1, 0, row=-2 ** 31), INVALID_INDEX, MSG_ROW)
    add("two_to_32_plus_3_row_u64", IDX_U64, I64, lambda c: _with(c, 0, 12, row=2 ** 32 + 3), INVALID_INDEX, MSG_ROW)
    add("two_to_32_plus_3_col_u64", IDX_U64, I64, lambda c: _with(c, 0, 12, col=2 ** 32 + 3), INVALID_INDEX, MSG_COL)
    add("two_to_63_row_u64", IDX_U64, I64, lambda c: _with(c, 1, 512, row=2 ** 63), INVALID_INDEX, MSG_ROW)
    add("two_to_63_col_u64", IDX_U64, I64, lambda c: _with(c, 1, 512, col=2 ** 63), INVALID_INDEX, MSG_COL)
    add("two_to_32_plus_3_row_i64", IDX_I64, I64, lambda c: _with(c, 2, 698, row=2 ** 32 + 3), INVALID_INDEX, MSG_ROW)
    add("two_to_32_plus_3_col_i64", IDX_I64, I64, lambda c: _with(c, 2, 698, col=2 ** 32 + 3), INVALID_INDEX, MSG_COL)
    add("u32_max_col", IDX_U32, I64, lambda c: _with(c, 0, 1, col=2 ** 32 - 1), INVALID_INDEX, MSG_COL)
    add("montgomery_word_equal_to_l", IDX_I64, M32, lambda c: [(2, 257, L)], INVALID_SCALAR, MSG_SCALAR)
    add("montgomery_word_all_ones", IDX_I64, M32, lambda c: [(0, 699, 2 ** 256 - 1)], INVALID_SCALAR, MSG_SCALAR)
    return out


def sequential_first_error(dims, arrays, val_formats):
    """the walk of Instance.new over the arrays as Python integers: (code, message) of the first defect, or None"""
    nc, nv, ni = dims
    for (rows, cols, vals), fmt in zip(arrays, val_formats):
        for i in range(len(rows)):
            if not 0 <= int(rows[i]) < nc:
                return INVALID_INDEX, MSG_ROW
            if not 0 <= int(cols[i]) < nv + 1 + ni:
                return INVALID_INDEX, MSG_COL
            if fmt in (C32, M32) and int.from_bytes(vals[i].tobytes(), "little") >= L:
                return INVALID_SCALAR, MSG_SCALAR
    return None
