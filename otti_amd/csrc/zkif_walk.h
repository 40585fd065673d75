// The bounds-checked reading of one zkInterface ConstraintSystem message body (zkif.cpp: Buf, Table::field / sub / vec, append_lc), written so that
// a device thread can run it: no HIP, no allocation, no exceptions, HD functions over (base, length, offset) only.  k_ingest.hip runs it on the
// device, one thread per constraint (count) and one per entry (emit); tests/zkif_walk_check.cpp runs the same functions on the host under the
// address and undefined-behaviour sanitizers and compares them with zkif_load + instance_new.
//
// Every load goes through zw_u32 / zw_u16 / zw_u8, which compare offset and length with the message's length BEFORE the address is formed; a load
// out of bounds records an error and yields 0.  No load assumes that its offset is aligned (the host reader's loads are memcpy): a value is
// composed from the 32-bit words that hold it, which ARE aligned by construction — `base` is 4-byte aligned (the device stages every message at a
// 16-byte aligned base) and readable up to its length rounded up to 4.
//
// Errors.  A sequential host run reports the FIRST defect it meets; threads meet them in any order.  So a defect is a 64-bit key that sorts in the
// order the host meets them, and the smallest key of a run (atomicMin on the device) names the error the host reports:
//     bit 63      0: a parse error (zkif_load), 1: a coefficient >= l (instance_new, which runs after the whole file has parsed)
//     parse:      row (30 bits) | matrix (2) | stage (1) | entry (29) | sub (1)
//                 stage 0: the tables and vectors of the combination (append_lc checks all of them before its first entry): OTTI_ERR_IO
//                 stage 1: entry e: sub 0 an undeclared variable id (OTTI_ERR_INVALID_INDEX), sub 1 a non-zero byte beyond the 32nd (OTTI_ERR_INVALID_SCALAR)
//     non-canonical: matrix (2 bits, at 61) | entry index within that matrix's list: OTTI_ERR_INVALID_SCALAR
// kZwNoError (all ones) sorts behind every defect.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "field.h"                                            // HD, and the conversion the callers apply to an emitted coefficient
#include "../../include/otti_spartan.h"

namespace otti {

constexpr uint64_t kZwNoError = ~0ull;
constexpr uint64_t kZwMaxRows = (uint64_t)1 << 30;            // rows a key can name (instance_new refuses more)
constexpr uint64_t kZwMaxEntries = (uint64_t)1 << 29;         // ids of one combination: 8 bytes each in a message of less than 4 GiB

HD uint64_t zw_key_parse(uint64_t row, int k, int stage, uint64_t entry, int sub) {
    return (row << 33) | ((uint64_t)k << 31) | ((uint64_t)stage << 30) | (entry << 1) | (uint64_t)sub;
}
HD uint64_t zw_key_noncanonical(int k, uint64_t index) { return ((uint64_t)1 << 63) | ((uint64_t)k << 61) | index; }
HD int zw_key_code(uint64_t key) {
    if (key == kZwNoError) return OTTI_OK;
    if (key >> 63) return OTTI_ERR_INVALID_SCALAR;
    if (!((key >> 30) & 1)) return OTTI_ERR_IO;
    return (key & 1) ? OTTI_ERR_INVALID_SCALAR : OTTI_ERR_INVALID_INDEX;
}

// one ConstraintSystem message: its body (after the size prefix), where its vector of constraint offsets starts and how many it holds, and the
// row of its first constraint.  The host's message walk fills this with its own checks done: vec_start + 4 * count <= size.
struct ZwMsg { const uint8_t *base; uint64_t size, vec_start, count, first_row; };

// a walk's state: the message and the smallest key met so far
struct Zw {
    const uint8_t *base; uint64_t n; uint64_t err;
    HD void fail(uint64_t key) { if (key < err) err = key; }
};

// ---- the accessors: [off, off + len) within [0, n), or the error `key` and 0
HD bool zw_chk(Zw &z, uint64_t off, uint64_t len, uint64_t key) {
    if (off > z.n || len > z.n - off) { z.fail(key); return false; }
    return true;
}
HD uint32_t zw_word(const Zw &z, uint64_t index) { return *reinterpret_cast<const uint32_t *>(z.base + 4 * index); }   // callers have checked the bytes they take from it
HD uint32_t zw_u32(Zw &z, uint64_t off, uint64_t key) {
    if (!zw_chk(z, off, 4, key)) return 0;
    const unsigned sh = (unsigned)(off & 3) * 8;
    const uint32_t lo = zw_word(z, off >> 2);
    if (!sh) return lo;
    return (lo >> sh) | (zw_word(z, (off >> 2) + 1) << (32 - sh));        // off + 3 is in bounds, so the next word starts in bounds
}
HD uint32_t zw_u8(Zw &z, uint64_t off, uint64_t key) {
    if (!zw_chk(z, off, 1, key)) return 0;
    return (zw_word(z, off >> 2) >> ((unsigned)(off & 3) * 8)) & 0xffu;
}
HD uint32_t zw_u16(Zw &z, uint64_t off, uint64_t key) {
    if (!zw_chk(z, off, 2, key)) return 0;
    const unsigned sh = (unsigned)(off & 3) * 8;
    const uint32_t lo = zw_word(z, off >> 2) >> sh;
    if (sh < 24) return lo & 0xffffu;
    return (lo | (zw_word(z, (off >> 2) + 1) << 8)) & 0xffffu;
}
HD uint64_t zw_u64(Zw &z, uint64_t off, uint64_t key) {
    if (!zw_chk(z, off, 8, key)) return 0;
    return (uint64_t)zw_u32(z, off, key) | ((uint64_t)zw_u32(z, off + 4, key) << 32);
}

// Table::field: the absolute position of field `id` of the table at pos, or 0 when it is absent.  ok = false: a load failed (recorded).
HD uint64_t zw_field(Zw &z, uint64_t pos, int id, uint64_t key, bool &ok) {
    const uint64_t before = z.err;
    const int64_t vt = (int64_t)pos - (int64_t)(int32_t)zw_u32(z, pos, key);
    if (z.err != before) { ok = false; return 0; }
    if (vt < 0) { z.fail(key); ok = false; return 0; }
    const uint32_t vsize = zw_u16(z, (uint64_t)vt, key);
    if (z.err != before) { ok = false; return 0; }
    const uint64_t slot = 4 + 2 * (uint64_t)id;
    if (slot + 2 > vsize) return 0;
    const uint32_t off = zw_u16(z, (uint64_t)vt + slot, key);
    if (z.err != before) { ok = false; return 0; }
    return off ? pos + off : 0;
}
// Table::vec: start and count of the vector in field `id`; false when the field is absent (start = count = 0)
HD bool zw_vec(Zw &z, uint64_t pos, int id, uint64_t key, uint64_t &start, uint64_t &count, bool &ok) {
    start = count = 0;
    const uint64_t f = zw_field(z, pos, id, key, ok);
    if (!ok || !f) return false;
    const uint64_t before = z.err;
    const uint64_t v = f + zw_u32(z, f, key);
    if (z.err != before) { ok = false; return false; }
    count = zw_u32(z, v, key);
    if (z.err != before) { ok = false; count = 0; return false; }
    start = v + 4;
    return true;
}

// one linear combination of one constraint as append_lc sees it: count entries (0: absent table, no ids — or refused, with the error recorded),
// ids at ids_start (8 bytes each), coefficients at vals_start (width bytes each)
struct ZwLc { uint64_t count, ids_start, vals_start, width; };

// combination k (0 A, 1 B, 2 C) of constraint i of message m, with every check append_lc and the tables above it make, in their order
HD ZwLc zw_lc(Zw &z, const ZwMsg &m, uint64_t i, int k) {
    ZwLc lc; lc.count = lc.ids_start = lc.vals_start = lc.width = 0;
    const uint64_t key = zw_key_parse(m.first_row + i, k, 0, 0, 0), before = z.err;
    bool ok = true;
    const uint64_t o = m.vec_start + 4 * i;
    const uint64_t bc = o + zw_u32(z, o, key);                          // the BilinearConstraint table
    if (z.err != before || !zw_chk(z, bc, 4, key)) return lc;
    const uint64_t f = zw_field(z, bc, k, key, ok);                     // Table::sub(k)
    if (!ok || !f) return lc;
    const uint64_t vars = f + zw_u32(z, f, key);
    if (z.err != before || !zw_chk(z, vars, 4, key)) return lc;
    uint64_t is, in, vs, vn;
    zw_vec(z, vars, 0, key, is, in, ok);
    if (!ok || !in) return lc;
    if (!zw_chk(z, is, in * 8, key)) return lc;
    const bool have = zw_vec(z, vars, 1, key, vs, vn, ok);
    if (!ok) return lc;
    if (!have || vn == 0 || vn % in) { z.fail(key); return lc; }
    if (!zw_chk(z, vs, vn, key)) return lc;
    lc.count = in; lc.ids_start = is; lc.vals_start = vs; lc.width = vn / in;
    return lc;
}

// THE element rule, for coefficients (zw_emit) and assigned values (zkif_wit_walk.h) alike: the w bytes at src as eight little-endian words — a
// narrower element zero-extended; of a wider one the first 32, any non-zero byte beyond them being the error key_tail.  val comes zeroed.
HD void zw_value(Zw &z, uint64_t src, uint64_t w, uint64_t key, uint64_t key_tail, uint32_t val[8]) {
    if (w >= 32) for (int j = 0; j < 8; j++) val[j] = zw_u32(z, src + 4 * j, key);
    else for (uint64_t b = 0; b < w; b++) val[b >> 2] |= zw_u8(z, src + b, key) << ((unsigned)(b & 3) * 8);
    if (w > 32) {
        uint32_t tail = 0;
        for (uint64_t b = 32; b < w; b++) tail |= zw_u8(z, src + b, key);
        if (tail) z.fail(key_tail);
    }
}

// ---- the two entry points
// COUNT: entries of (row, matrix) for the three matrices of constraint i
HD void zw_count(Zw &z, const ZwMsg &m, uint64_t i, uint32_t out[3]) {
    for (int k = 0; k < 3; k++) out[k] = (uint32_t)zw_lc(z, m, i, k).count;
}
// EMIT: entry e of combination k of constraint i: the variable id and the coefficient as eight little-endian words (32 canonical bytes: a narrower
// element zero-extended; of a wider one the first 32, any non-zero byte beyond them being the entry's stage-1 / sub-1 error).  The caller maps the
// id first (sub 0 sorts before sub 1, as append_lc looks the column up before it copies the value).  False: the combination does not hold entry e.
HD bool zw_emit(Zw &z, const ZwMsg &m, uint64_t i, int k, uint64_t e, uint64_t &id, uint32_t val[8]) {
    const ZwLc lc = zw_lc(z, m, i, k);
    for (int j = 0; j < 8; j++) val[j] = 0;
    id = 0;
    if (e >= lc.count) return false;
    const uint64_t key = zw_key_parse(m.first_row + i, k, 0, 0, 0);    // (cannot fail: zw_lc has checked both vectors whole)
    id = zw_u64(z, lc.ids_start + 8 * e, key);
    zw_value(z, lc.vals_start + e * lc.width, lc.width, key, zw_key_parse(m.first_row + i, k, 1, e, 1), val);
    return true;
}
// the column of a variable id (zkif.cpp ColOf::col, then instance_new's shift of the columns behind the variables by the padding), or the entry's
// stage-1 / sub-0 error and 0.  col_of: IdMap::col_of, n_ids entries, 0xffffffff = undeclared.
HD uint32_t zw_col(Zw &z, const uint32_t *col_of, uint64_t n_ids, uint64_t id, uint64_t num_vars, uint64_t pad_shift, uint64_t key_entry) {
    if (id >= n_ids || col_of[id] == 0xffffffffu) { z.fail(key_entry); return 0; }
    const uint32_t c = col_of[id];
    return c >= num_vars ? (uint32_t)(c + pad_shift) : c;
}

}  // namespace otti
