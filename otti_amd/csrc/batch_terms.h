// The group equations of a batch of proofs as one weighted sum (verify_batch.cpp): every check the verifier does not hash has the form
// sum_j s_j * P_j = identity, stated as a list of terms — a scalar with either a point, named by its 32-byte encoding, or a generator slot.  The
// verifiers state each equation as such a list and nothing else: the single verifier sums it (verify.h term_sum), the batch collects it.  An
// equation that fails leaves an error point E != identity; under independent uniform weights w the weighted sum  sum_k w_k E_k  is the identity
// with probability 1 / l only, whatever the E_k are: two defects cannot cancel unless they share a weight, which is why every equation of every
// proof has its own.  This header does the scalar side of that — it multiplies the weights in, merges the terms that name the same point
// and folds the generator terms into one scalar per slot — over the field type and the standard library alone, so a host compiler can run it
// without the group arithmetic (tests/verify_batch_check.cpp models a point by its discrete logarithm).
#pragma once
#include "field.h"
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

namespace otti {

typedef std::array<uint8_t, 32> BtKey;
struct BtTerm { Fr s; int32_t gen; BtKey key; };            // gen >= 0: generator slot `gen`; gen < 0: the point whose encoding is `key`
inline BtTerm bt_point(const Fr &s, const uint8_t enc[32]) { BtTerm t; t.s = s; t.gen = -1; memcpy(t.key.data(), enc, 32); return t; }
inline BtTerm bt_gen(const Fr &s, uint32_t slot) { BtTerm t; t.s = s; t.gen = (int32_t)slot; t.key.fill(0); return t; }
// one proof's equations in the order they arose: equation k is terms [eq[k], eq[k + 1])
struct BtEquations {
    std::vector<BtTerm> terms; std::vector<uint32_t> eq{0};
    void point(const Fr &s, const uint8_t enc[32]) { terms.push_back(bt_point(s, enc)); }
    void gen(const Fr &s, uint32_t slot) { terms.push_back(bt_gen(s, slot)); }
    void close() { eq.push_back((uint32_t)terms.size()); }   // the terms since the last close() are one equation (an empty one holds trivially)
    void equation(const std::vector<BtTerm> &e) { terms.insert(terms.end(), e.begin(), e.end()); close(); }
    size_t count() const { return eq.size() - 1; }
};
// one proof's equations under their weights: a scalar per distinct point, in the order of first appearance, and a scalar per generator slot
struct BtWeighted { std::vector<BtKey> keys; std::vector<Fr> point_s; std::vector<Fr> gen_s; std::vector<uint8_t> gen_used; };

struct BtKeyHash { size_t operator()(const BtKey &k) const { uint64_t h; memcpy(&h, k.data() + 8, 8); return (size_t)(h * 0x9e3779b97f4a7c15ULL); } };

// w: E.count() weights.  false (out is unspecified): a term names a generator slot >= ngens.
inline bool bt_weigh(const BtEquations &E, const Fr *w, size_t ngens, BtWeighted &out) {
    out.keys.clear(); out.point_s.clear(); out.gen_s.assign(ngens, fr_zero()); out.gen_used.assign(ngens, 0);
    std::unordered_map<BtKey, uint32_t, BtKeyHash> at; at.reserve(E.terms.size());
    for (size_t k = 0; k + 1 < E.eq.size(); k++)
        for (uint32_t i = E.eq[k]; i < E.eq[k + 1]; i++) {
            const BtTerm &t = E.terms[i]; const Fr s = fr_mul(w[k], t.s);
            if (t.gen >= 0) {
                if ((size_t)t.gen >= ngens) return false;
                out.gen_s[t.gen] = fr_add(out.gen_s[t.gen], s); out.gen_used[t.gen] = 1;
                continue;
            }
            auto ins = at.emplace(t.key, (uint32_t)out.keys.size());
            if (ins.second) { out.keys.push_back(t.key); out.point_s.push_back(s); }
            else out.point_s[ins.first->second] = fr_add(out.point_s[ins.first->second], s);
        }
    return true;
}
// the generator scalars of all proofs as one scalar per slot: total[i] += one[i]; returns how many slots any proof has used so far
inline size_t bt_fold_gens(std::vector<Fr> &total, std::vector<uint8_t> &used, const BtWeighted &one) {
    if (total.size() < one.gen_s.size()) { total.resize(one.gen_s.size(), fr_zero()); used.resize(one.gen_s.size(), 0); }
    for (size_t i = 0; i < one.gen_s.size(); i++) if (one.gen_used[i]) { total[i] = fr_add(total[i], one.gen_s[i]); used[i] = 1; }
    size_t n = 0; for (uint8_t u : used) n += u;
    return n;
}

}  // namespace otti
