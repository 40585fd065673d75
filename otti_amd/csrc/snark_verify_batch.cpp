// Many SNARK proofs of one computation commitment verified as one randomised batch (snark.h snark_verify_batch).  Host code only: the staging is
// snark_verify_many's (snark_verify_staged), the device's sum is reached through a hook that prover.cpp sets, so the CPU rebuilds of the host sources
// compile this file as it is.
#include "snark.h"
#include "hostpar.h"
#include <atomic>
#include <thread>

namespace otti {

SnarkBatchSumHook g_snark_batch_sum_hook = nullptr;

namespace {
bool is_identity(const Pt &p) { return pt_eq(p, pt_identity()); }
// one proof of a chunk under its weights: the points of both lists as one set (an encoding both name stands twice, which the sum does not mind)
struct Weighed {
    SnarkCollected *col; BtWeighted w[2];                      // [0] over g.sat, [1] over g.eval
    std::vector<BtKey> keys; std::vector<Fr> point_s; std::vector<const BtRun *> runs[2];
};
// the sums on the host cores: a set's points are decoded once and kept for the localisation pass; a handle's scalars are its base with the runs expanded
struct HostSum {
    const Gens *g[2]; std::vector<std::vector<Pt>> pts; std::vector<uint8_t> bad;
    void decode(const SnarkBatchSet *sets, size_t n) {
        pts.resize(n); bad.assign(n, 0);
        const unsigned nt = (unsigned)std::min<size_t>({n, (size_t)16, (size_t)std::max(1u, std::thread::hardware_concurrency())});
        std::atomic<size_t> next{0};
        fan_out(nt, [&](unsigned) { for (size_t k; (k = next.fetch_add(1)) < n;) { pts[k].resize(sets[k].n); for (size_t i = 0; i < sets[k].n; i++) if (!pt_decode_fast(pts[k][i], sets[k].comp32 + 32 * i)) { pts[k][i] = pt_identity(); bad[k] = 1; } } });
    }
    Pt over_gens(const BatchGenSide &s, int h) const {
        const size_t n = g[h]->P.size();
        std::vector<Fr> sc(n, fr_zero());
        if (s.base) std::copy(s.base, s.base + n, sc.begin());
        for (size_t r = 0; r < s.nruns; r++) bt_run_expand(*s.runs[r], sc.data());
        return host_msm_wide(sc.data(), g[h]->P.data(), n);
    }
    Pt all(const SnarkBatchSet *sets, size_t n, const BatchGenSide total[2]) const {
        std::vector<Pt> P; std::vector<Fr> s;
        for (size_t k = 0; k < n; k++) { P.insert(P.end(), pts[k].begin(), pts[k].end()); s.insert(s.end(), sets[k].scalars, sets[k].scalars + sets[k].n); }
        return pt_add(host_msm_wide(s.data(), P.data(), P.size()), pt_add(over_gens(total[0], 0), over_gens(total[1], 1)));
    }
    Pt one(const SnarkBatchSet &set, size_t k) const { return pt_add(host_msm_wide(set.scalars, pts[k].data(), set.n), pt_add(over_gens(set.gen[0], 0), over_gens(set.gen[1], 1))); }
};
}  // namespace

void snark_verify_batch(const CompComm &comm, const SnarkGens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count, unsigned threads,
                        const uint8_t *seed32, int32_t *results, otti_verify_batch_info *info) {
    otti_verify_batch_info inf; memset(&inf, 0, sizeof inf);
    struct Report { otti_verify_batch_info *to, &from; ~Report() { if (to) *to = from; } } report{info, inf};
    if (!count) return;
    if (!threads) threads = kSnarkVerifyBatchThreads;
    inf.workers = (uint32_t)std::min<size_t>({(size_t)threads, (size_t)kVerifyManyMaxThreads, count});
    RandomTape tape(seed32);
    uint32_t sums_run = 0;
    const Gens *gs[2] = {g.sat.get(), g.eval.get()};
    const size_t ngens[2] = {gs[0]->P.size(), gs[1]->P.size()};
    auto single = [&](size_t item) {                                              // the single verifier decides, for its exact code
        inf.singles_rerun++;
        std::vector<Fr> inputs;
        int rc = item_inputs(items[item], comm.num_inputs, inputs);
        if (!rc) { try { rc = snark_verify(comm, inputs, g, tlabel, tlabel_len, items[item].proof, items[item].proof_len); } catch (const Error &e) { rc = e.code; } catch (...) { rc = OTTI_ERR_INTERNAL; } }
        results[item] = rc;
    };
    const SnarkChunkEnd chunk_end = [&](std::vector<SnarkCollected *> &done) {
        inf.live += (uint32_t)done.size();
        // ---- every equation of every collected proof under a weight of its own; the explicit generator terms folded per handle, the runs kept as they are
        std::vector<Weighed> in_sum; in_sum.reserve(done.size());
        std::vector<size_t> to_single;
        std::vector<Fr> base_total[2]; std::vector<uint8_t> base_used[2]; size_t run_slots[2] = {0, 0};
        for (SnarkCollected *c : done) {
            if (c->walk_code != OTTI_OK) { to_single.push_back(c->item); continue; }
            Weighed W; W.col = c;
            const size_t n0 = c->sat.count(), n1 = c->eval.count();
            const std::vector<Fr> w = tape.random_vector("weight", n0 + n1);
            if (!bt_weigh(c->sat, w.data(), ngens[0], W.w[0]) || !bt_weigh(c->eval, w.data() + n0, ngens[1], W.w[1])) { to_single.push_back(c->item); continue; }
            W.keys = W.w[0].keys; W.keys.insert(W.keys.end(), W.w[1].keys.begin(), W.w[1].keys.end());
            W.point_s = W.w[0].point_s; W.point_s.insert(W.point_s.end(), W.w[1].point_s.begin(), W.w[1].point_s.end());
            if (W.keys.empty()) { to_single.push_back(c->item); continue; }
            inf.equations += (uint32_t)(n0 + n1); inf.points += (uint32_t)W.keys.size();
            for (int h = 0; h < 2; h++) {
                bt_fold_gens(base_total[h], base_used[h], W.w[h]);
                for (const BtRun &r : W.w[h].runs) run_slots[h] = std::max(run_slots[h], r.slots());
            }
            in_sum.push_back(std::move(W));
        }
        for (Weighed &W : in_sum) for (int h = 0; h < 2; h++) { W.runs[h].clear(); for (const BtRun &r : W.w[h].runs) W.runs[h].push_back(&r); }   // in_sum no longer moves
        {   // how many generator slots of both handles the sum touches: a run covers [0, 2^lg), the explicit terms name theirs
            size_t n = 0;
            for (int h = 0; h < 2; h++) { n += run_slots[h]; for (size_t i = run_slots[h]; i < base_used[h].size(); i++) n += base_used[h][i]; }
            inf.gen_slots = std::max(inf.gen_slots, (uint32_t)n);
        }
        const size_t m = in_sum.size();
        if (m) {
            std::vector<SnarkBatchSet> sets(m); std::vector<const BtRun *> all_runs[2]; BatchGenSide total[2];
            for (size_t k = 0; k < m; k++) {
                Weighed &W = in_sum[k];
                sets[k].comp32 = W.keys[0].data(); sets[k].n = W.keys.size(); sets[k].scalars = W.point_s.data();
                for (int h = 0; h < 2; h++) {
                    sets[k].gen[h] = {W.w[h].gen_s.data(), W.runs[h].data(), W.runs[h].size()};
                    all_runs[h].insert(all_runs[h].end(), W.runs[h].begin(), W.runs[h].end());
                }
            }
            for (int h = 0; h < 2; h++) { base_total[h].resize(ngens[h], fr_zero()); total[h] = {base_total[h].data(), all_runs[h].data(), all_runs[h].size()}; }
            static_assert(sizeof(BtKey) == 32, "a proof's distinct points lie one behind the other as they are uploaded");
            std::vector<uint8_t> bad(m, 0); std::vector<Pt> sums(m);
            const char *where = getenv("OTTI_VERIFY_BATCH_SUM");                  // "host": the sum on the host cores whatever device there is (measurements, tests); read per call
            bool dev = g_snark_batch_sum_hook && !getenv("OTTI_VERIFY_HOST") && !(where && !strcmp(where, "host"));
            double ms = 0; Pt sum;
            if (dev) { try { dev = g_snark_batch_sum_hook(gs, sets.data(), m, total, false, &sum, bad.data(), &ms); } catch (...) { dev = false; } }
            HostSum host{{gs[0], gs[1]}, {}, {}};
            if (!dev) { host.decode(sets.data(), m); bad = host.bad; sum = host.all(sets.data(), m, total); ms = 0; }
            inf.on_device = dev; inf.sum_ms += ms;
            bool any_bad = false; for (uint8_t b : bad) any_bad |= b != 0;
            sums_run++;
            if (!any_bad && is_identity(sum)) { for (Weighed &W : in_sum) results[W.col->item] = OTTI_OK; }
            else {
                // ---- localisation: each proof's own sum, over what the first pass decoded
                inf.localise_passes++;
                bool again = dev;
                if (again) { double ms2 = 0; try { again = g_snark_batch_sum_hook(gs, sets.data(), m, total, true, sums.data(), bad.data(), &ms2); } catch (...) { again = false; } inf.sum_ms += ms2; }
                if (!again) {
                    if (dev) { host.decode(sets.data(), m); bad = host.bad; }    // the device let go between the passes
                    for (size_t k = 0; k < m; k++) sums[k] = host.one(sets[k], k);
                }
                for (size_t k = 0; k < m; k++) { if (!bad[k] && is_identity(sums[k])) results[in_sum[k].col->item] = OTTI_OK; else to_single.push_back(in_sum[k].col->item); }
            }
        }
        for (size_t item : to_single) single(item);
    };
    snark_verify_staged(comm, g, tlabel, tlabel_len, items, count, threads, results, &chunk_end);
    inf.accepted_first_pass = sums_run && !inf.localise_passes;                   // every chunk's sum was the identity
}

}  // namespace otti
