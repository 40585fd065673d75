// Many NIZK proofs of one instance verified as one randomised batch (spartan.h nizk_verify_batch).  Host code only: the batched evaluation of
// A, B, C and the device's sum are reached through hooks that prover.cpp sets, so the CPU rebuilds of the host sources compile this file as it is.
#include "spartan.h"
#include "verify.h"
#include "hostpar.h"
#include <atomic>
#include <memory>
#include <thread>

namespace otti {

BatchSumHook g_batch_sum_hook = nullptr;

namespace {
enum State { kWalk, kCollected, kSettled, kSingle };            // kSingle: the single verifier decides (rx / ry differ, or the proof's own sum fails)
struct Live : LiveProof {
    BtEquations sink; BtWeighted weighed; State state = kWalk;
    Fr evals[3]; bool have_evals = false;                       // A, B, C at the proof's point, once its walk has fetched them
};
// the walk of nizk_verify_parsed with the collecting sink: the code the walk itself met, or 0 with L.state set
int walk_one(const Instance &I, const Gens &g, const void *tlabel, size_t tlabel_len, Live &L, const InstEvalFetch *fetch) {
    try {
        const size_t N = I.num_cons, V = I.num_vars;
        Transcript tr(tlabel, tlabel_len);
        tr.append_protocol_name("Spartan NIZK proof");
        const InstEvalFetch keep([&](Fr out[3]) { (*fetch)(out); for (int j = 0; j < 3; j++) L.evals[j] = out[j]; L.have_evals = true; });
        if (!fetch) { I.evaluate(L.P.rx, L.P.ry, L.evals); L.have_evals = true; }
        std::vector<Fr> rx, ry;
        if (int rc = r1cs_verify_host(L.P, N, V, L.inputs, L.evals, g, tr, rx, ry, fetch ? &keep : nullptr, &L.sink)) return rc;
        bool same = true;
        for (size_t i = 0; i < rx.size(); i++) same &= fr_eq(rx[i], L.P.rx[i]);
        for (size_t i = 0; i < ry.size(); i++) same &= fr_eq(ry[i], L.P.ry[i]);
        L.state = same ? kCollected : kSingle;
        return OTTI_OK;
    } catch (const Error &e) { return e.code; }
    catch (...) { return OTTI_ERR_INTERNAL; }
}
bool is_identity(const Pt &p) { return pt_eq(p, pt_identity()); }
// the sums on the host cores: a set's points are decoded once and kept for the localisation pass
struct HostSum {
    const Gens &g; std::vector<std::vector<Pt>> pts; std::vector<uint8_t> bad;
    void decode(const BatchSumSet *sets, size_t n) {
        pts.resize(n); bad.assign(n, 0);
        const unsigned nt = (unsigned)std::min<size_t>({n, (size_t)16, (size_t)std::max(1u, std::thread::hardware_concurrency())});
        std::atomic<size_t> next{0};
        fan_out(nt, [&](unsigned) { for (size_t k; (k = next.fetch_add(1)) < n;) { pts[k].resize(sets[k].n); for (size_t i = 0; i < sets[k].n; i++) if (!pt_decode_fast(pts[k][i], sets[k].comp32 + 32 * i)) { pts[k][i] = pt_identity(); bad[k] = 1; } } });
    }
    Pt over_gens(const Fr *s, size_t ngens) const { return host_msm_wide(s, g.P.data(), ngens); }
    Pt all(const BatchSumSet *sets, size_t n, const Fr *gen_total, size_t ngens) const {
        std::vector<Pt> P; std::vector<Fr> s;
        for (size_t k = 0; k < n; k++) { P.insert(P.end(), pts[k].begin(), pts[k].end()); s.insert(s.end(), sets[k].scalars, sets[k].scalars + sets[k].n); }
        P.insert(P.end(), g.P.begin(), g.P.begin() + ngens); s.insert(s.end(), gen_total, gen_total + ngens);
        return host_msm_wide(s.data(), P.data(), P.size());
    }
    Pt one(const BatchSumSet &set, size_t k, size_t ngens) const { return pt_add(host_msm_wide(set.scalars, pts[k].data(), set.n), over_gens(set.gen_scalars, ngens)); }
};
}  // namespace

void nizk_verify_batch(const Instance &I, const Gens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count, unsigned threads,
                       const uint8_t *seed32, int32_t *results, otti_verify_batch_info *info) {
    otti_verify_batch_info inf; memset(&inf, 0, sizeof inf);
    struct Report { otti_verify_batch_info *to, &from; ~Report() { if (to) *to = from; } } report{info, inf};
    if (!count) return;
    const auto live = parse_items<Live>(I, items, count, results);
    const size_t n = live.size();
    inf.live = (uint32_t)n;
    if (!n) return;
    const char *rule = getenv("OTTI_VERIFY_BATCH_RULE");                      // "0", read per call: the routing below set aside (measurements, tests)
    if (n < kVerifyBatchMinLive && I.num_cons >= kVerifyBatchRouteMinCons && !(rule && !strcmp(rule, "0"))) {
        // one or two proofs of a large instance: nizk_verify_many's path is faster (profiles/verify_batch.md, rows K = 2), and its verdicts are these by contract
        std::vector<VerifyItem> sub(n); std::vector<int32_t> res(n, OTTI_ERR_INTERNAL);
        for (size_t k = 0; k < n; k++) sub[k] = items[live[k]->item];
        nizk_verify_many(I, g, tlabel, tlabel_len, sub.data(), n, threads, res.data());
        for (size_t k = 0; k < n; k++) results[live[k]->item] = res[k];
        inf.routed_to_many = 1; inf.workers = (uint32_t)std::min<size_t>(threads ? threads : kVerifyManyThreads, n);
        return;
    }
    // ---- the batched evaluation, queued on this thread before any worker starts (verify.h ManyEvals)
    std::vector<const NizkProof *> pts(n);
    for (size_t k = 0; k < n; k++) pts[k] = &live[k]->P;
    ManyEvals ev(I, std::move(pts));
    if (!threads) threads = kVerifyBatchThreads;
    const size_t nw = std::min<size_t>({(size_t)threads, (size_t)kVerifyManyMaxThreads, n});
    inf.workers = (uint32_t)nw;
    walk_proofs(ev, nw, [&](size_t k, const InstEvalFetch *fetch) {
        Live &L = *live[k];
        int rc;
        try { rc = walk_one(I, g, tlabel, tlabel_len, L, fetch); } catch (...) { rc = OTTI_ERR_INTERNAL; }
        if (rc) { L.state = kSettled; results[L.item] = rc; }
    });
    // ---- every equation of every collected proof under a weight of its own; the generator terms of all proofs folded into one scalar per slot
    const size_t ngens = g.P.size();
    RandomTape tape(seed32);
    std::vector<Live *> in_sum; std::vector<Fr> gen_total; std::vector<uint8_t> gen_used;
    for (auto &Lp : live) {
        Live &L = *Lp;
        if (L.state != kCollected) continue;
        const std::vector<Fr> w = tape.random_vector("weight", L.sink.count());
        if (!bt_weigh(L.sink, w.data(), ngens, L.weighed) || L.weighed.keys.empty()) { L.state = kSingle; continue; }
        inf.equations += (uint32_t)L.sink.count(); inf.points += (uint32_t)L.weighed.keys.size();
        inf.gen_slots = (uint32_t)bt_fold_gens(gen_total, gen_used, L.weighed);
        in_sum.push_back(&L);
    }
    const size_t m = in_sum.size();
    if (m) {
        std::vector<BatchSumSet> sets(m);
        for (size_t k = 0; k < m; k++) { const BtWeighted &W = in_sum[k]->weighed; sets[k] = {W.keys[0].data(), W.keys.size(), W.point_s.data(), W.gen_s.data()}; }
        static_assert(sizeof(BtKey) == 32, "a proof's distinct points lie one behind the other as they are uploaded");
        std::vector<uint8_t> bad(m, 0); std::vector<Pt> sums(m);
        const char *where = getenv("OTTI_VERIFY_BATCH_SUM");                  // "host": the sum on the host cores whatever device there is (measurements, tests); read per call
        bool dev = g_batch_sum_hook && !getenv("OTTI_VERIFY_HOST") && !(where && !strcmp(where, "host"));
        double ms = 0; Pt total;
        if (dev) { try { dev = g_batch_sum_hook(g, sets.data(), m, gen_total.data(), ngens, false, &total, bad.data(), &ms); } catch (...) { dev = false; } }
        HostSum host{g, {}, {}};
        if (!dev) { std::fill(bad.begin(), bad.end(), 0); host.decode(sets.data(), m); bad = host.bad; total = host.all(sets.data(), m, gen_total.data(), ngens); ms = 0; }
        inf.on_device = dev; inf.sum_ms = ms;
        bool any_bad = false; for (uint8_t b : bad) any_bad |= b != 0;
        if (!any_bad && is_identity(total)) { inf.accepted_first_pass = 1; for (Live *L : in_sum) results[L->item] = OTTI_OK; }
        else {
            // ---- localisation: each proof's own sum, over what the first pass decoded
            inf.localise_passes = 1;
            bool again = dev;
            if (again) { double ms2 = 0; try { again = g_batch_sum_hook(g, sets.data(), m, gen_total.data(), ngens, true, sums.data(), bad.data(), &ms2); } catch (...) { again = false; } inf.sum_ms += ms2; }
            if (!again) {
                if (dev) { host.decode(sets.data(), m); bad = host.bad; }        // the device let go between the passes
                for (size_t k = 0; k < m; k++) sums[k] = host.one(sets[k], k, ngens);
            }
            for (size_t k = 0; k < m; k++) { if (!bad[k] && is_identity(sums[k])) results[in_sum[k]->item] = OTTI_OK; else in_sum[k]->state = kSingle; }
        }
    }
    // ---- the single verifier settles the rest, with the values its walk has fetched
    for (auto &Lp : live) {
        Live &L = *Lp;
        if (L.state != kSingle) continue;
        inf.singles_rerun++;
        int rc;
        try { rc = nizk_verify_parsed(I, L.inputs, g, tlabel, tlabel_len, L.P, L.have_evals ? L.evals : nullptr, nullptr); }
        catch (const Error &e) { rc = e.code; } catch (...) { rc = OTTI_ERR_INTERNAL; }
        results[L.item] = rc;
    }
}

}  // namespace otti
