// The rule of otti_amd/csrc/coo_walk.h on the host, before any of it runs on a GPU: own main, the header alone, built by tests/host_build.py with the
// address and undefined-behaviour sanitizers.  Three parts:
//   1. coo_load_index over corner values in all four formats against the values written (128-bit compare, no narrowing);
//   2. coo_place over corner rows and columns around every bound and around 2^31, 2^32, 2^63, against the rule restated here in 128-bit integers;
//   3. the error key: random runs of three matrices with defects planted, judged entry by entry in a SCRAMBLED order with the smallest key kept (what
//      the device's one atomicMin word ends up holding), against a sequential walk over A, then B, then C written here that stops at the first
//      defect, row before column before scalar.
// Exit status 0 and "0 mismatches" on the last line, or every mismatch named.
#include "../otti_amd/csrc/coo_walk.h"
#include <stdio.h>
#include <stdint.h>
#include <algorithm>
#include <random>
#include <string>
#include <vector>

using namespace otti;
typedef __int128 i128;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_bad++; printf("MISMATCH %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// one index array of every format holding the same list of numbers (those the format can hold), and the numbers as written
struct IndexArrays {
    std::vector<uint32_t> u32; std::vector<int32_t> i32; std::vector<uint64_t> u64; std::vector<int64_t> i64;
};
static const void *base_of(const IndexArrays &a, int f) {
    return f == COO_IDX_U32 ? (const void *)a.u32.data() : f == COO_IDX_I32 ? (const void *)a.i32.data() : f == COO_IDX_U64 ? (const void *)a.u64.data() : (const void *)a.i64.data();
}
static uint64_t load(int f, const void *base, uint64_t i, bool &neg) {
    switch (f) {
    case COO_IDX_U32: return coo_load_index<COO_IDX_U32>(base, i, neg);
    case COO_IDX_I32: return coo_load_index<COO_IDX_I32>(base, i, neg);
    case COO_IDX_U64: return coo_load_index<COO_IDX_U64>(base, i, neg);
    default: return coo_load_index<COO_IDX_I64>(base, i, neg);
    }
}
// the number element i of format f's array stands for
static i128 written(const IndexArrays &a, int f, size_t i) {
    return f == COO_IDX_U32 ? (i128)a.u32[i] : f == COO_IDX_I32 ? (i128)a.i32[i] : f == COO_IDX_U64 ? (i128)a.u64[i] : (i128)a.i64[i];
}

static std::vector<i128> corner_numbers(uint64_t bound) {
    std::vector<i128> v = {0, 1, 2, 3, -1, -2, (i128)INT32_MAX, (i128)INT32_MAX + 1, (i128)INT32_MIN, (i128)UINT32_MAX, (i128)UINT32_MAX + 1, ((i128)1 << 32) + 3,
                           (i128)INT64_MAX, (i128)INT64_MIN, (i128)1 << 63, (i128)UINT64_MAX, ((i128)1 << 63) + 3, ((i128)1 << 40)};
    for (int d = -2; d <= 2; d++) { v.push_back((i128)bound + d); v.push_back(((i128)1 << 32) + (i128)bound + d); }
    return v;
}
static bool fits(int f, i128 x) {
    switch (f) {
    case COO_IDX_U32: return x >= 0 && x <= (i128)UINT32_MAX;
    case COO_IDX_I32: return x >= (i128)INT32_MIN && x <= (i128)INT32_MAX;
    case COO_IDX_U64: return x >= 0 && x <= (i128)UINT64_MAX;
    default: return x >= (i128)INT64_MIN && x <= (i128)INT64_MAX;
    }
}
static void push(IndexArrays &a, int f, i128 x) {
    switch (f) {
    case COO_IDX_U32: a.u32.push_back((uint32_t)x); break;
    case COO_IDX_I32: a.i32.push_back((int32_t)x); break;
    case COO_IDX_U64: a.u64.push_back((uint64_t)x); break;
    default: a.i64.push_back((int64_t)x); break;
    }
}

// the placement rule in 128-bit integers: the kind of the first defect, or COO_PLACED with the stored pair
static int place_ref(uint64_t nc, uint64_t nv, uint64_t ni, uint64_t nvp, i128 row, i128 col, bool scalar_refused, uint64_t &r, uint64_t &c) {
    if (row < 0 || row >= (i128)nc) return COO_KIND_ROW;
    if (col < 0 || col >= (i128)nv + 1 + (i128)ni) return COO_KIND_COL;
    if (scalar_refused) return COO_KIND_SCALAR;
    r = (uint64_t)row; c = (uint64_t)(col >= (i128)nv ? col + (i128)nvp - (i128)nv : col);
    return COO_PLACED;
}
static uint64_t next_pow2(uint64_t n) { uint64_t p = 1; while (p < n) p <<= 1; return p; }

static size_t check_loads_and_placement() {
    size_t cases = 0;
    const uint64_t dims[][3] = {{1, 3, 5}, {5, 5, 1}, {5, 8, 0}, {1, 0, 3}, {37, 29, 3}, {1u << 30, 1u << 30, (1u << 30) - 1}, {3, (1u << 30) - 1, 0}, {65536, 1, 65535}};
    for (const auto &d : dims) {
        const uint64_t nc = d[0], nv = d[1], ni = d[2], nvp = next_pow2(std::max(nv, ni + 1));
        const CooDims cd = coo_dims(nc, nv, ni, nvp);
        std::vector<i128> rows = corner_numbers(nc), cols = corner_numbers(nv + 1 + ni);
        for (i128 x : corner_numbers(nv)) cols.push_back(x);
        for (int f = 0; f < 4; f++) {
            IndexArrays ra, ca; std::vector<i128> rw, cw;
            for (i128 x : rows) if (fits(f, x)) { push(ra, f, x); rw.push_back(x); }
            for (i128 x : cols) if (fits(f, x)) { push(ca, f, x); cw.push_back(x); }
            for (size_t i = 0; i < rw.size(); i++) {
                bool rneg = false; const uint64_t r = load(f, base_of(ra, f), i, rneg);
                CHECK(written(ra, f, i) == rw[i], "format %d: array element %zu", f, i);
                CHECK(rneg == (rw[i] < 0) && (rneg || (i128)r == rw[i]), "format %d: load of %lld: %llu neg %d", f, (long long)rw[i], (unsigned long long)r, (int)rneg);
                for (size_t j = 0; j < cw.size(); j++) {
                    bool cneg = false; const uint64_t c = load(f, base_of(ca, f), j, cneg);
                    for (int refused = 0; refused < 2; refused++) {
                        uint32_t ro = 0xdeadbeef, co = 0xdeadbeef; uint64_t rr = 0, rc = 0;
                        const int got = coo_place(cd, r, rneg, c, cneg, refused != 0, ro, co), want = place_ref(nc, nv, ni, nvp, rw[i], cw[j], refused != 0, rr, rc);
                        CHECK(got == want, "format %d dims %llu %llu %llu row %lld col %lld: kind %d want %d", f, (unsigned long long)nc, (unsigned long long)nv,
                              (unsigned long long)ni, (long long)rw[i], (long long)cw[j], got, want);
                        if (got == COO_PLACED && want == COO_PLACED) CHECK(ro == rr && co == rc && rc < 2 * nvp, "format %d: placed (%u, %u) want (%llu, %llu)", f, ro, co,
                                                                           (unsigned long long)rr, (unsigned long long)rc);
                        if (got != COO_PLACED) CHECK(ro == 0xdeadbeef && co == 0xdeadbeef, "a refused entry wrote its outputs");
                        cases++;
                    }
                }
            }
        }
    }
    return cases;
}

struct Entry { i128 row, col; bool refused; };
// instance_new's walk: A, then B, then C, each in order, the first defect ends it; 0 and no message when there is none
static int sequential(uint64_t nc, uint64_t nv, uint64_t ni, const std::vector<Entry> m[3], const char *&what) {
    for (int k = 0; k < 3; k++)
        for (const Entry &e : m[k]) {
            if (e.row < 0 || e.row >= (i128)nc) { what = "row index out of range"; return -6; }
            if (e.col < 0 || e.col >= (i128)(nv + 1 + ni)) { what = "column index out of range"; return -6; }
            if (e.refused) { what = "non-canonical scalar in matrix"; return -5; }
        }
    what = ""; return 0;
}

static size_t check_key_order() {
    std::mt19937_64 rng(20240607);
    size_t runs = 0;
    for (int run = 0; run < 4000; run++) {
        const uint64_t nc = 1 + rng() % 40, nv = rng() % 40, ni = rng() % 8, nvp = next_pow2(std::max(nv, ni + 1));
        const CooDims cd = coo_dims(nc, nv, ni, nvp);
        const int f = (int)(rng() % 4);
        std::vector<Entry> m[3];
        const int n_defects = (int)(rng() % 5);               // 0: a clean run
        for (int k = 0; k < 3; k++) {
            const size_t n = rng() % 3 == 0 ? 0 : rng() % 600;
            for (size_t i = 0; i < n; i++) m[k].push_back(Entry{(i128)(rng() % nc), (i128)(rng() % (nv + 1 + ni)), false});
        }
        for (int dft = 0; dft < n_defects; dft++) {
            const int k = (int)(rng() % 3);
            if (m[k].empty()) continue;
            Entry &e = m[k][rng() % m[k].size()];
            const std::vector<i128> bad_rows = corner_numbers(nc), bad_cols = corner_numbers(nv + 1 + ni);
            const unsigned what = (unsigned)(rng() % 7) + 1;      // any mix of the three kinds in one entry
            if (what & 1) { i128 x; do x = bad_rows[rng() % bad_rows.size()]; while (!fits(f, x) || (x >= 0 && x < (i128)nc)); e.row = x; }
            if (what & 2) { i128 x; do x = bad_cols[rng() % bad_cols.size()]; while (!fits(f, x) || (x >= 0 && x < (i128)(nv + 1 + ni))); e.col = x; }
            if (what & 4) e.refused = true;
        }
        // the arrays in format f, every entry judged once in a scrambled order, the smallest key kept
        uint64_t key = kCooNoError;
        std::vector<std::pair<int, size_t>> order;
        IndexArrays ra[3], ca[3];
        for (int k = 0; k < 3; k++)
            for (size_t i = 0; i < m[k].size(); i++) { push(ra[k], f, m[k][i].row); push(ca[k], f, m[k][i].col); order.push_back({k, i}); }
        std::shuffle(order.begin(), order.end(), rng);
        for (const auto &o : order) {
            const int k = o.first; const size_t i = o.second;
            bool rneg, cneg; uint32_t ro, co;
            const uint64_t r = load(f, base_of(ra[k], f), i, rneg), c = load(f, base_of(ca[k], f), i, cneg);
            const int kind = coo_place(cd, r, rneg, c, cneg, m[k][i].refused, ro, co);
            if (kind != COO_PLACED) {
                const uint64_t mine = coo_key(k, i, kind);
                CHECK(mine != kCooNoError && coo_key_matrix(mine) == k && coo_key_position(mine) == i && coo_key_kind(mine) == kind, "key fields of (%d, %zu, %d)", k, i, kind);
                key = std::min(key, mine);
            }
        }
        const char *want_what = nullptr; const int want = sequential(nc, nv, ni, m, want_what);
        CHECK(coo_key_code(key) == want && std::string(coo_key_what(key)) == want_what, "run %d format %d: code %d \"%s\", the sequential walk says %d \"%s\"", run, f,
              coo_key_code(key), coo_key_what(key), want, want_what);
        runs++;
    }
    // the ends of the key's fields: the last position of the last matrix sorts below "no error", matrices before positions before kinds
    const uint64_t last = coo_key(2, kCooMaxEntries - 1, COO_KIND_SCALAR);
    CHECK(last < kCooNoError && coo_key_position(last) == kCooMaxEntries - 1 && coo_key_matrix(last) == 2, "the largest key");
    CHECK(coo_key(0, kCooMaxEntries - 1, COO_KIND_SCALAR) < coo_key(1, 0, COO_KIND_ROW), "matrix before position");
    CHECK(coo_key(1, 5, COO_KIND_SCALAR) < coo_key(1, 6, COO_KIND_ROW), "position before kind");
    CHECK(coo_key(1, 5, COO_KIND_ROW) < coo_key(1, 5, COO_KIND_COL) && coo_key(1, 5, COO_KIND_COL) < coo_key(1, 5, COO_KIND_SCALAR), "row < column < scalar");
    CHECK(coo_key_code(kCooNoError) == 0, "no error decodes to 0");
    return runs;
}

int main() {
    const size_t cases = check_loads_and_placement();
    const size_t runs = check_key_order();
    printf("%zu placements, %zu runs, %d mismatches\n", cases, runs, g_bad);
    return g_bad ? 1 : 0;
}
