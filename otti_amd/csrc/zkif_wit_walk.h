// The bounds-checked reading of the Witness messages of a .wit.zkif file (zkif.cpp: read_variables, and the assignment loop of the loaders' frame),
// written as zkif_walk.h is: HD functions over (base, length, offset), no HIP, no allocation, no exceptions, every load through zw_u8 / zw_u32 /
// zw_u64.  k_wit_ingest.hip runs it on the device, one thread per assigned variable; tests/zkif_wit_walk_check.cpp runs the same functions on the
// host under the address and undefined-behaviour sanitizers and compares them with zkif_load.
//
// The host's message walk (zkif.cpp zkif_witness_with) has located the ids vector and the values vector of every message and checked that both lie
// within it, as it does for ZwMsg.
//
// Errors.  One 64-bit key per defect, sorting in the order the host pair (zkif_load, then the upload) meets them; the smallest names the error to
// report.  The top four bits are the step, the rest orders defects within it:
//     1  per Witness message in file order: (message << 33) | kind << 32 | element.  kind 0: the message's tables and vectors (OTTI_ERR_IO, found by
//        the host walk); kind 1: the first element wider than 32 bytes with a non-zero tail (OTTI_ERR_INVALID_SCALAR).  read_variables meets both
//        before the next message is looked at.
//     2  the frame's checks of the headers, the id map and the number of assigned variables (host; the code is the check's own)
//     3  0: an inputs file without values, 1: a witness message without values (host; OTTI_ERR_IO)
//     4  element e, in concatenated order, whose id is 0, an instance id or unknown (OTTI_ERR_INVALID_INDEX)
//     5  a variable assigned twice — with the count right, another is then not assigned at all, which is what the host says, and only behind
//        the whole list's step 4 (OTTI_ERR_IO)
//     6  0: a non-canonical public input (the upload's host check); 1 + e: the witness value of element e is >= l (OTTI_ERR_INVALID_SCALAR)
// kZwNoError sorts behind every defect.
#pragma once
#include "zkif_walk.h"

namespace otti {

enum { WW_MESSAGE = 1, WW_FRAME = 2, WW_NO_VALUES = 3, WW_INDEX = 4, WW_TWICE = 5, WW_SCALAR = 6 };
HD uint64_t ww_key(int step, uint64_t rest) { return ((uint64_t)step << 60) | rest; }
HD uint64_t ww_key_message(uint64_t message, int kind, uint64_t element) { return ww_key(WW_MESSAGE, (message << 33) | ((uint64_t)kind << 32) | element); }
HD int ww_key_step(uint64_t key) { return (int)(key >> 60); }
// the code of a key this reader or the host walk records (a step-2 defect carries its own code: zkif.cpp)
HD int ww_key_code(uint64_t key) {
    if (key == kZwNoError) return OTTI_OK;
    switch (ww_key_step(key)) {
    case WW_MESSAGE: return ((key >> 32) & 1) ? OTTI_ERR_INVALID_SCALAR : OTTI_ERR_IO;
    case WW_INDEX: return OTTI_ERR_INVALID_INDEX;
    case WW_SCALAR: return OTTI_ERR_INVALID_SCALAR;
    default: return OTTI_ERR_IO;
    }
}
constexpr uint64_t kWwMaxMessages = (uint64_t)1 << 27;        // messages a key can name (a message is at least 8 bytes: a file of 1 GiB of nothing else)

// one Witness message: its body, where its ids (8 bytes each) and values (stride bytes each) start, how many variables it assigns, and the place of
// its first one in the concatenated list.  width: the bytes of an element the reader has to look at — stride, unless the host walk has read the
// tails of a message of absurdly wide elements itself (kWwMaxWidth) and leaves 32.  The host walk has checked ids_start + 8 * count <= size and
// vals_start + stride * count <= size.
constexpr uint64_t kWwMaxWidth = 4096;                         // a thread reads an element's tail byte by byte: wider ones are the host walk's
struct WwMsg { const uint8_t *base; uint64_t size, ids_start, vals_start, count, width, stride, first; };

// assigned variable i of message m (the `message`-th Witness message of the file): its id, and its value by the element rule (zw_value)
HD void ww_elem(Zw &z, const WwMsg &m, uint64_t message, uint64_t i, uint64_t &id, uint32_t val[8]) {
    for (int j = 0; j < 8; j++) val[j] = 0;
    const uint64_t key = ww_key_message(message, 0, 0);               // (cannot fail: the host walk has checked both vectors whole)
    id = zw_u64(z, m.ids_start + 8 * i, key);
    zw_value(z, m.vals_start + i * m.stride, m.width, key, ww_key_message(message, 1, i), val);
}
// the column of a witness variable's id: id - 1 - (the instance ids below it) — ids are dense, so a binary search over the ni sorted instance ids
// serves — or the error `key` and 0xffffffff: id 0 (the constant), an instance id, or a column that is not below num_vars
HD uint32_t ww_col(Zw &z, const uint64_t *inst_sorted, uint64_t ni, uint64_t id, uint64_t num_vars, uint64_t key) {
    uint64_t lo = 0, hi = ni;                                          // the first instance id that is not below `id`
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (inst_sorted[mid] < id) lo = mid + 1; else hi = mid; }
    if (id == 0 || (lo < ni && inst_sorted[lo] == id) || id - 1 - lo >= num_vars) { z.fail(key); return 0xffffffffu; }
    return (uint32_t)(id - 1 - lo);
}

}  // namespace otti
