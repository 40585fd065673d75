// The rule by which one (row, column, coefficient) triple of a caller's arrays becomes an entry of A, B or C (otti_instance_from_coo), written so
// that a device thread can run it: no HIP, no allocation, no exceptions, COO_HD functions over plain words, standard headers only.
// k_coo_ingest.hip runs it on the device, one thread per entry; tests/coo_walk_check.cpp runs the same functions on the host under the address and
// undefined-behaviour sanitizers and compares them with a sequential walk written there.
//
// Indices come in four formats (= OTTI_IDX_* of the C ABI).  coo_load_index widens one to 64 bits and says whether a signed one was negative;
// the bounds are judged on that 64-bit value BEFORE anything is narrowed, so 2^32 + 3 is out of range and never the index 3.
//
// Placement is instance_new's: row < num_cons, col < num_vars + 1 + num_inputs, and a column behind the variables (the constant 1, an input) moves
// up by the padding of the variable block, col + nvp - num_vars.
//
// Errors.  instance_new walks A, then B, then C and reports the FIRST defect it meets, within one entry the row before the column before the
// scalar; threads meet them in any order.  So a defect is a 64-bit key that sorts in that order, and the smallest key of a run (one atomicMin
// word on the device) names the error the host reports:
//     matrix (2 bits, at 34) | position in that matrix's arrays (32 bits, at 2: a matrix has fewer than 2^32 entries) | kind (2 bits)
//     kind 0: row out of range, 1: column out of range (both OTTI_ERR_INVALID_INDEX), 2: a coefficient >= l (OTTI_ERR_INVALID_SCALAR)
// kCooNoError (all ones) sorts behind every defect.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define COO_HD __host__ __device__ __forceinline__
#else
#define COO_HD inline
#endif

namespace otti {

enum CooIdxFormat { COO_IDX_U32 = 0, COO_IDX_I32 = 1, COO_IDX_U64 = 2, COO_IDX_I64 = 3 };   // = OTTI_IDX_* of the C ABI
constexpr size_t coo_index_bytes(int format) { return format == COO_IDX_U32 || format == COO_IDX_I32 ? 4 : 8; }

constexpr uint64_t kCooNoError = ~0ull;
constexpr uint64_t kCooMaxEntries = (uint64_t)1 << 32;        // entries of one matrix: a key names a position in 32 bits
enum CooKind { COO_KIND_ROW = 0, COO_KIND_COL = 1, COO_KIND_SCALAR = 2, COO_PLACED = 3 };
constexpr int kCooErrInvalidScalar = -5, kCooErrInvalidIndex = -6;   // = OTTI_ERR_INVALID_SCALAR, OTTI_ERR_INVALID_INDEX (asserted where both are seen)

// element i of an index array in format F, as 64 bits; neg: a signed index below zero (its 64 bits are then meaningless: it is out of range)
template <int F> COO_HD uint64_t coo_load_index(const void *base, uint64_t i, bool &neg) {
    if (F == COO_IDX_U32) { neg = false; return static_cast<const uint32_t *>(base)[i]; }
    if (F == COO_IDX_I32) { const int32_t x = static_cast<const int32_t *>(base)[i]; neg = x < 0; return (uint64_t)(uint32_t)x; }
    if (F == COO_IDX_U64) { neg = false; return static_cast<const uint64_t *>(base)[i]; }
    const int64_t x = static_cast<const int64_t *>(base)[i]; neg = x < 0; return (uint64_t)x;
}

// the caller's dimensions as the rule reads them: num_cols = num_vars + 1 + num_inputs, pad_shift = nvp - num_vars
struct CooDims { uint64_t num_cons, num_cols, num_vars, pad_shift; };
COO_HD CooDims coo_dims(uint64_t num_cons, uint64_t num_vars, uint64_t num_inputs, uint64_t nvp) {
    return CooDims{num_cons, num_vars + 1 + num_inputs, num_vars, nvp - num_vars};
}

// one entry judged: COO_PLACED with the stored row and the padded column, or the kind of its first defect (row, then column, then scalar)
COO_HD int coo_place(const CooDims &d, uint64_t row, bool row_neg, uint64_t col, bool col_neg, bool scalar_refused, uint32_t &row_out, uint32_t &col_out) {
    if (row_neg || row >= d.num_cons) return COO_KIND_ROW;
    if (col_neg || col >= d.num_cols) return COO_KIND_COL;
    if (scalar_refused) return COO_KIND_SCALAR;
    row_out = (uint32_t)row;
    col_out = (uint32_t)(col >= d.num_vars ? col + d.pad_shift : col);
    return COO_PLACED;
}

COO_HD uint64_t coo_key(int matrix, uint64_t position, int kind) { return ((uint64_t)matrix << 34) | (position << 2) | (uint64_t)kind; }
COO_HD int coo_key_matrix(uint64_t key) { return (int)(key >> 34); }
COO_HD uint64_t coo_key_position(uint64_t key) { return (key >> 2) & 0xffffffffull; }
COO_HD int coo_key_kind(uint64_t key) { return (int)(key & 3); }
COO_HD int coo_key_code(uint64_t key) {
    if (key == kCooNoError) return 0;
    return coo_key_kind(key) == COO_KIND_SCALAR ? kCooErrInvalidScalar : kCooErrInvalidIndex;
}
// instance_new's wording for the same defect
COO_HD const char *coo_key_what(uint64_t key) {
    if (key == kCooNoError) return "";
    const int kind = coo_key_kind(key);
    return kind == COO_KIND_ROW ? "row index out of range" : kind == COO_KIND_COL ? "column index out of range" : "non-canonical scalar in matrix";
}

}  // namespace otti
