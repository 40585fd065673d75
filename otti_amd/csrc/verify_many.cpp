// Many NIZK proofs of one instance verified in one call (spartan.h nizk_verify_many).  Host code only: the batched evaluation of A, B, C at the
// proofs' points is reached through two hooks that prover.cpp sets, so the CPU rebuilds of the host sources compile this file as it is.
#include "spartan.h"
#include "verify.h"
#include <atomic>
#include <memory>
#include <thread>

namespace otti {

InstEvalManyBeginHook g_inst_eval_many_begin_hook = nullptr;
InstEvalManyNextHook g_inst_eval_many_next_hook = nullptr;

namespace {
struct Live { size_t item; std::vector<Fr> inputs; NizkProof P; };
int verify_one(const Instance &I, const Gens &g, const void *tlabel, size_t tlabel_len, const Live &L, const InstEvalFetch *fetch) {
    try { return nizk_verify_parsed(I, L.inputs, g, tlabel, tlabel_len, L.P, nullptr, fetch); }
    catch (const Error &e) { return e.code; }
    catch (...) { return OTTI_ERR_INTERNAL; }
}
}  // namespace

void nizk_verify_many(const Instance &I, const Gens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count, unsigned threads,
                      int32_t *results) {
    if (!count) return;
    // ---- parse and check, item by item, in the single path's order: the inputs' scalars, their count, the proof's bytes, its challenge lengths
    const size_t nrx = ilog2(I.num_cons), nry = ilog2(2 * I.num_vars);
    std::vector<std::unique_ptr<Live>> live; live.reserve(count);
    for (size_t i = 0; i < count; i++) {
        const VerifyItem &it = items[i];
        try {
            auto L = std::make_unique<Live>(); L->item = i;
            if (int rc = item_inputs(it, I.num_inputs, L->inputs)) { results[i] = rc; continue; }
            L->P = NizkProof::parse(it.proof, it.proof_len);
            if (L->P.rx.size() != nrx || L->P.ry.size() != nry) { results[i] = OTTI_ERR_VERIFY_INTERNAL; continue; }
            results[i] = OTTI_ERR_INTERNAL;                   // until its worker has written the verdict
            live.push_back(std::move(L));
        } catch (const Error &e) { results[i] = e.code; }
        catch (...) { results[i] = OTTI_ERR_INTERNAL; }
    }
    const size_t n = live.size();
    if (!n) return;
    // ---- the batched evaluation, queued on this thread before any worker starts (verify.h ManyEvals)
    std::vector<const NizkProof *> pts(n);
    for (size_t k = 0; k < n; k++) pts[k] = &live[k]->P;
    ManyEvals ev(I, std::move(pts));
    const bool queued = ev.queued;
    if (!threads) threads = kVerifyManyThreads;
    const size_t nw = std::min<size_t>({(size_t)threads, (size_t)kVerifyManyMaxThreads, n});
    if (nw <= 1) {
        // one worker: the calling thread, in the single path's order — the evaluation is collected where the first proof needs it
        for (size_t k = 0; k < n; k++) {
            const InstEvalFetch fetch([&ev, k](Fr out[3]) { ev.fetch_on_caller(k, out); });
            results[live[k]->item] = verify_one(I, g, tlabel, tlabel_len, *live[k], queued ? &fetch : nullptr);
        }
        ev.collect_rest();
        return;
    }
    // ---- workers take the live proofs in order, one at a time; each verdict goes to its own item's slot
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t k = next.fetch_add(1, std::memory_order_relaxed);
            if (k >= n) return;
            int rc;
            try {
                const InstEvalFetch fetch([&ev, k](Fr out[3]) { ev.fetch_on_worker(k, out); });
                rc = verify_one(I, g, tlabel, tlabel_len, *live[k], queued ? &fetch : nullptr);
            } catch (...) { rc = OTTI_ERR_INTERNAL; }
            results[live[k]->item] = rc;
        }
    };
    std::vector<std::thread> th; th.reserve(nw);
    struct Join { std::vector<std::thread> &th; ManyEvals &ev; ~Join() { ev.let_go(); for (auto &t : th) if (t.joinable()) t.join(); } } join{th, ev};
    for (size_t w = 0; w < nw; w++) {
        try { th.emplace_back(work); } catch (const std::system_error &) { break; }      // short of threads: those that started share the work
    }
    ev.collect_rest();
    if (th.empty()) work();
}

}  // namespace otti
