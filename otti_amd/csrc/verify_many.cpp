// Many NIZK proofs of one instance verified in one call (spartan.h nizk_verify_many).  Host code only: the batched evaluation of A, B, C at the
// proofs' points is reached through two hooks that prover.cpp sets, so the CPU rebuilds of the host sources compile this file as it is.
#include "spartan.h"
#include "verify.h"

namespace otti {

InstEvalManyBeginHook g_inst_eval_many_begin_hook = nullptr;
InstEvalManyNextHook g_inst_eval_many_next_hook = nullptr;

namespace {
int verify_one(const Instance &I, const Gens &g, const void *tlabel, size_t tlabel_len, const LiveProof &L, const InstEvalFetch *fetch) {
    try { return nizk_verify_parsed(I, L.inputs, g, tlabel, tlabel_len, L.P, nullptr, fetch); }
    catch (const Error &e) { return e.code; }
    catch (...) { return OTTI_ERR_INTERNAL; }
}
}  // namespace

void nizk_verify_many(const Instance &I, const Gens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count, unsigned threads,
                      int32_t *results) {
    if (!count) return;
    const auto live = parse_items<LiveProof>(I, items, count, results);
    const size_t n = live.size();
    if (!n) return;
    // ---- the batched evaluation, queued on this thread before any worker starts (verify.h ManyEvals)
    std::vector<const NizkProof *> pts(n);
    for (size_t k = 0; k < n; k++) pts[k] = &live[k]->P;
    ManyEvals ev(I, std::move(pts));
    if (!threads) threads = kVerifyManyThreads;
    // ---- workers take the live proofs in order, one at a time; each verdict goes to its own item's slot
    walk_proofs(ev, std::min<size_t>({(size_t)threads, (size_t)kVerifyManyMaxThreads, n}),
                [&](size_t k, const InstEvalFetch *fetch) { results[live[k]->item] = verify_one(I, g, tlabel, tlabel_len, *live[k], fetch); });
}

}  // namespace otti
