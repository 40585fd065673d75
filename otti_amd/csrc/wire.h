// The proofs' wire form (bincode, as upstream's serde derives it): a vector is a u64 count followed by its elements, a point its 32-byte
// encoding, a scalar the 32 bytes of its Montgomery limbs, little endian.  Writer and Reader are the two codecs; they expose the SAME method
// names on references, so wire.cpp writes each object's field order once, as a function template over the codec, and serialize() / parse()
// of NizkProof, SnarkProof and CompComm (spartan.h, snark.h) are that walk with one codec or the other.  Nothing outside wire.cpp knows the layout.
#pragma once
#include "spartan.h"
#include <string.h>

namespace otti {
namespace wire {

// the largest counts a reader accepts (it allocates for a count only after this check)
constexpr size_t kMaxVarRows = (size_t)1 << 20;              // comm_vars: rows of the witness commitment
constexpr size_t kMaxCommRows = (size_t)1 << 24;             // comm_derefs, comm_ops, comm_mem
constexpr size_t kMaxRounds = 64;                            // anything counted in sum-check rounds, layers or reduction steps
constexpr size_t kMaxRoundScalars = 4;                       // a round's DotProductProof::z

struct Writer {
    static constexpr bool reading = false;
    std::vector<uint8_t> b;
    void raw(const void *p, size_t n) { const uint8_t *q = (const uint8_t *)p; b.insert(b.end(), q, q + n); }
    void u64(const uint64_t &v) { uint64_t x = v; uint8_t t[8]; for (int i = 0; i < 8; i++) { t[i] = (uint8_t)x; x >>= 8; } raw(t, 8); }
    void pt(const CPoint &c) { raw(c.b, 32); }
    void fr(const Fr &x) { raw(x.v, 32); }                      // upstream serialises Scalar's Montgomery limbs
    size_t len(size_t have, size_t) { u64(have); return have; } // the count of a vector whose elements the walk writes itself
    void pts(const std::vector<CPoint> &v, size_t) { u64(v.size()); for (auto &c : v) pt(c); }
    void frs(const std::vector<Fr> &v, size_t) { u64(v.size()); for (auto &x : v) fr(x); }
    void frs_fixed(const Fr *v, size_t k) { u64(k); for (size_t i = 0; i < k; i++) fr(v[i]); }
    void expect(bool, const char *) {}
};

struct Reader {
    static constexpr bool reading = true;
    const uint8_t *p; size_t n, pos = 0;
    [[noreturn]] static void refuse(const char *msg) { throw Error(OTTI_ERR_MALFORMED_PROOF, msg); }
    void need(size_t k) { if (k > n - pos) refuse("proof truncated"); }
    void u64(uint64_t &x) { need(8); x = 0; for (int i = 7; i >= 0; i--) x = (x << 8) | p[pos + i]; pos += 8; }
    void pt(CPoint &c) { need(32); memcpy(c.b, p + pos, 32); pos += 32; }
    void fr(Fr &x) { need(32); memcpy(x.v, p + pos, 32); pos += 32; if (!fr_raw_is_canonical(x.v)) refuse("scalar out of range"); }
    size_t len(size_t, size_t max) { uint64_t k; u64(k); if (k > max) refuse("vector length out of range"); return (size_t)k; }
    void pts(std::vector<CPoint> &v, size_t max) { v.resize(len(0, max)); for (auto &c : v) pt(c); }
    void frs(std::vector<Fr> &v, size_t max) { v.resize(len(0, max)); for (auto &x : v) fr(x); }
    void frs_fixed(Fr *v, size_t k) { uint64_t have; u64(have); if (have != k) refuse("vector length"); for (size_t i = 0; i < k; i++) fr(v[i]); }
    void expect(bool ok, const char *msg) { if (!ok) refuse(msg); }
    bool at_end() const { return pos == n; }
};

}  // namespace wire
}  // namespace otti
