// The group equations of a batch of proofs as one weighted sum (verify_batch.cpp): every check the verifier does not hash has the form
// sum_j s_j * P_j = identity, stated as a list of terms — a scalar with either a point, named by its 32-byte encoding, or a generator slot.  The
// verifiers state each equation as such a list and nothing else: the single verifier sums it (verify.h term_sum), the batch collects it.  An
// equation that fails leaves an error point E != identity; under independent uniform weights w the weighted sum  sum_k w_k E_k  is the identity
// with probability 1 / l only, whatever the E_k are: two defects cannot cancel unless they share a weight, which is why every equation of every
// proof has its own.  This header does the scalar side of that — it multiplies the weights in, merges the terms that name the same point
// and folds the generator terms into one scalar per slot — over the field type and the standard library alone, so a host compiler can run it
// without the group arithmetic (tests/verify_batch_check.cpp models a point by its discrete logarithm).  A list may also hold product-form runs
// over its handle's first generator slots (BtRun below; tests/batch_runs_check.cpp): only a collector that asked for them gets any.
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
// A product-form run: generator slots [0, 2^lg) of the list's handle, slot i with the scalar  c * prod_{t < lg, bit t of i set} f[t]  (bit 0 the least
// significant) — the closing equation of a log dot-product proof names n generators with scalars of this form (spartan_host.cpp
// dotproductlog_verify: f[t] is the squared challenge lg - 1 - t), so lg + 1 scalars stand for n terms.  eq: the equation the run belongs to.
struct BtRun { Fr c; uint32_t eq = 0; std::vector<Fr> f; size_t lg() const { return f.size(); } size_t slots() const { return (size_t)1 << f.size(); } };
// out[i] += the run's scalar of slot i, for i < 2^lg (out holds at least that many): the host reference of the device expansion (k_msm.hip k_gen_runs)
inline void bt_run_expand(const BtRun &r, Fr *out) {
    std::vector<Fr> s(r.slots()); s[0] = r.c;
    for (size_t t = 0; t < r.lg(); t++) for (size_t i = 0, k = (size_t)1 << t; i < k; i++) s[i + k] = fr_mul(s[i], r.f[t]);
    for (size_t i = 0; i < s.size(); i++) out[i] = fr_add(out[i], s[i]);
}
// one proof's equations in the order they arose: equation k is terms [eq[k], eq[k + 1]) and the runs that name k
struct BtEquations {
    std::vector<BtTerm> terms; std::vector<uint32_t> eq{0};
    std::vector<BtRun> runs; bool accept_runs = false;      // accept_runs: set by a collector that takes product-form runs; without it a site writes its generator terms out
    void run(const Fr &c, const Fr *f, size_t lg) { BtRun r; r.c = c; r.eq = (uint32_t)count(); r.f.assign(f, f + lg); runs.push_back(std::move(r)); }   // belongs to the equation that is open
    void point(const Fr &s, const uint8_t enc[32]) { terms.push_back(bt_point(s, enc)); }
    void gen(const Fr &s, uint32_t slot) { terms.push_back(bt_gen(s, slot)); }
    void close() { eq.push_back((uint32_t)terms.size()); }   // the terms since the last close() are one equation (an empty one holds trivially)
    void equation(const std::vector<BtTerm> &e) { terms.insert(terms.end(), e.begin(), e.end()); close(); }
    size_t count() const { return eq.size() - 1; }
};
// one proof's equations under their weights: a scalar per distinct point, in the order of first appearance, and a scalar per generator slot
// (the explicitly stated generator terms), and the runs with their coefficient under their equation's weight, factors as they were
struct BtWeighted { std::vector<BtKey> keys; std::vector<Fr> point_s; std::vector<Fr> gen_s; std::vector<uint8_t> gen_used; std::vector<BtRun> runs; };

struct BtKeyHash { size_t operator()(const BtKey &k) const { uint64_t h; memcpy(&h, k.data() + 8, 8); return (size_t)(h * 0x9e3779b97f4a7c15ULL); } };

// w: E.count() weights.  false (out is unspecified): a term names a generator slot >= ngens, or a run reaches past ngens or names no equation.
inline bool bt_weigh(const BtEquations &E, const Fr *w, size_t ngens, BtWeighted &out) {
    out.keys.clear(); out.point_s.clear(); out.gen_s.assign(ngens, fr_zero()); out.gen_used.assign(ngens, 0); out.runs.clear();
    for (const BtRun &r : E.runs) {
        if (r.eq >= E.count() || r.lg() >= 32 || r.slots() > ngens) return false;
        out.runs.push_back(r); out.runs.back().c = fr_mul(w[r.eq], r.c);
    }
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
