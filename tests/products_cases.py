"""Shared by the tests of kept products (test_witness_products_host.py, test_gpu_products_patch_kernel.py, test_gpu_witness_products.py): the
pure-Python model of a patch — touched rows = rows with an entry of A, B or C in a changed column — the marker that stands for "not written", and
the change sets laid over the instances of sparse_cases.py.  A plain module like sparse_cases.py; nothing here is collected and nothing here calls
the library.  Columns are indices into z (2 * nvp of them: a caller's column c >= nv sits at c + nvp - nv, SparseCase.col_shifted)."""
import random

import numpy as np

import sparse_cases as sc

L = sc.L
# The marker fills the stale vectors: 32 bytes 0xa5 read as a word are above l, and every word a kernel stores is a canonical Montgomery word (< l)
MARKER_BYTE = 0xa5
MARKER_WORD = int.from_bytes(bytes([MARKER_BYTE]) * 32, "little")
assert MARKER_WORD >= L


def marker_rows(n):
    return np.full((n, 32), MARKER_BYTE, dtype=np.uint8)


def touched_rows(case, cols):
    """the model: ascending rows that hold an entry of A, B or C in one of the changed columns of z"""
    cols = set(int(c) for c in cols)
    return sorted({r for m in case.ents for r, c, _ in m if case.col_shifted(c) in cols})


def changed_z(case, z, cols, tag=0):
    """z with OTHER values at cols (never the value it holds), the same wherever it is built"""
    rng = random.Random(repr(("changed", case.name, tag, tuple(int(c) for c in cols))))
    out = list(z)
    for c in cols:
        out[int(c)] = (out[int(c)] + 1 + rng.randrange(L - 1)) % L
    return out


def failing_of(abc):
    a, b, c = abc
    return [r for r in range(len(a)) if a[r] * b[r] % L != c[r]]


def bitmap(rows, n):
    bits = np.zeros((n + 63) // 64, dtype=np.uint64)
    for r in rows:
        bits[r >> 6] |= np.uint64(1 << (r & 63))
    return bits


def columns_by_length(case, which):
    """[(list length, column of z)] over the LADDER of a transposed ladder case: the column whose by-column list in matrix `which` has that length"""
    places = sc.ladder_places(case.nv)
    by_len = {n: j for j, n in places.items()}
    assert sorted(by_len) == sorted(sc.LADDER)
    ln = case.lengths(by_col=True)[which]
    out = []
    for n in sc.LADDER:
        j = by_len[n]
        assert ln[case.col_shifted(j)] == n, (n, j, ln[case.col_shifted(j)])   # (the ladder's repeated pair and explicit zero sit in columns 11, 12: none of these)
        out.append((n, case.col_shifted(j)))
    return out


def columns_by_row_length(case, which):
    """[(row length, column of z)] over the LADDER of an untransposed ladder case: one column of the row of that length (taken from the row's list in
    matrix `which`, or from another matrix's where that list is empty)"""
    places = sc.ladder_places(case.nc)
    by_len = {n: r for r, n in places.items()}
    first = {}
    for k in (which, (which + 1) % 3, (which + 2) % 3):
        for r, c, _ in case.ents[k]:
            first.setdefault(r, case.col_shifted(c))
    return [(n, first[by_len[n]]) for n in sc.LADDER]


def edges_case():
    """256 constraints over 64 variables for the ends of the touched bitmap.  Columns 0 .. 5 carry the edges, the rest fill every row:
        0: rows 0, 63, 64 and N - 1 (A)          1: all 64 rows of word 2 (B)          2: no entry in A, B or C
        3: rows 10, 11 (A)   4: rows 10, 12 (B): the two meet in row 10               5: row 20 through A and through C"""
    nc, nv, ni = 256, 64, 2
    rng = random.Random("products-edges")
    ents = [[], [], []]
    for r in range(nc):
        ents[0].append((r, 8 + r % 40, rng.randrange(1, L)))
        ents[1].append((r, nv, rng.randrange(1, L)))               # the constant column
        ents[2].append((r, 8 + (r * 7) % 40, rng.randrange(1, L)))
    ents[0] += [(r, 0, rng.randrange(1, L)) for r in (0, 63, 64, nc - 1)]
    ents[1] += [(r, 1, rng.randrange(1, L)) for r in range(128, 192)]
    ents[0] += [(r, 3, rng.randrange(1, L)) for r in (10, 11)]
    ents[1] += [(r, 4, rng.randrange(1, L)) for r in (10, 12)]
    ents[0].append((20, 5, rng.randrange(1, L))); ents[2].append((20, 5, rng.randrange(1, L)))
    z = [rng.randrange(L) for _ in range(nv)] + [1] + [rng.randrange(L) for _ in range(ni)]
    z += [0] * (2 * nv - len(z))
    return sc.SparseCase("products-edges", nc, nv, ni, ents, z, [0] * nc, [0, 0, 0], "lane", False)


EDGE_CHANGES = {"rows 0, 63, 64, N - 1": ([0], [0, 63, 64, 255]), "a whole word": ([1], list(range(128, 192))), "none": ([2], []),
                "two columns meet in a row": ([3, 4], [10, 11, 12]), "one row through A and C": ([5], [20])}


def sat_changes(sat, case):
    """for the verdict transitions on a SatLadder case: one variable column (below nv) of A's list in each of a few rows — long rows, short rows, the
    ends of a word and the last row"""
    want = [r for r in (0, 5, 63, 64, 66, 127, 130, case.nc - 1) if r < case.nc]
    cols = {}
    for r, c, _ in sat.A:
        if r in want and c < case.nv and r not in cols:
            cols[r] = c
    return sorted(set(cols.values()))


def kernel_cases():
    """(case, [column lists]) for every instance and change set the kernel-level GPU test uses: the host test holds the model against
    SparseCase.multiply_vec on all of them"""
    for which in range(3):
        for mix in ("codes", "nocodes"):
            case = sc.ladder_case("lane", which, mix, transposed=True)
            yield case, [[c] for _, c in columns_by_length(case, which)]
            for layout in ("lane", "quad"):
                case = sc.ladder_case(layout, which, mix)
                yield case, [[c] for _, c in columns_by_row_length(case, which)]
    for mix in ("codes", "nocodes"):
        case = sc.column_quad_case(mix)
        yield case, [[0], [5, 6, 7, 900], list(range(64, 192))]
    case = edges_case()
    yield case, [cols for cols, _ in EDGE_CHANGES.values()]
    for layout, codes in (("lane", True), ("quad", False)):
        sat = sc.SatLadder(layout, codes)
        case = sat.with_failing([])
        yield case, [sat_changes(sat, case)]
    sat = sc.SatLadder("quad", False, 12, 8)
    case = sat.with_failing([])
    yield case, [[0, 3]]
