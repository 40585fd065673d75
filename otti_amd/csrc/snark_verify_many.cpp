// Many SNARK proofs of one computation commitment verified in one call (snark.h snark_verify_many), and the staging it shares with the randomised
// batch (snark_verify_staged; snark_verify_batch.cpp).  Host code only: the batched row sums are
// reached through one hook that prover.cpp sets, so the CPU rebuilds of the host sources compile this file as it is.
#include "snark.h"
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

namespace otti {

RowSumsManyHook g_row_sums_many_hook = nullptr;

namespace {
// one proof between parse and verdict: its transcript and the resumable evaluation-proof walk, parked between steps with its request out
struct Live {
    size_t item = 0; std::vector<Fr> inputs; SnarkProof S; std::vector<Fr> rx, ry;
    std::unique_ptr<Transcript> tr; std::unique_ptr<EvalProofVerifier> v;
    RowRequest req; RowAnswer ans; bool host_sum = true, alive = true;
    SnarkCollected col;                                       // snark_verify_batch: the group equations this walk stated instead of running
};
// The call's own threads: `extra` of them beside the calling thread, started once and parked on a condition variable between the phases;
// run(n, f) shares f(0 .. n) out among them and the caller and returns when all are done.  f does not throw.
class Crew {
public:
    explicit Crew(size_t extra) {
        for (size_t i = 0; i < extra; i++) { try { th_.emplace_back([this] { loop(); }); } catch (const std::system_error &) { break; } }   // short of threads: those that started share the work
    }
    ~Crew() { { std::lock_guard<std::mutex> lk(mu_); quit_ = true; } cv_.notify_all(); for (auto &t : th_) t.join(); }
    void run(size_t n, const std::function<void(size_t)> &f) {
        if (th_.empty() || n <= 1) { for (size_t k = 0; k < n; k++) f(k); return; }
        { std::lock_guard<std::mutex> lk(mu_); fn_ = &f; n_ = n; next_.store(0, std::memory_order_relaxed); gen_++; busy_ = th_.size(); }
        cv_.notify_all();
        take();
        std::unique_lock<std::mutex> lk(mu_); done_.wait(lk, [&] { return busy_ == 0; });
    }
private:
    std::mutex mu_; std::condition_variable cv_, done_; std::vector<std::thread> th_;
    const std::function<void(size_t)> *fn_ = nullptr; size_t n_ = 0, gen_ = 0, busy_ = 0; bool quit_ = false; std::atomic<size_t> next_{0};
    void take() { for (;;) { const size_t k = next_.fetch_add(1, std::memory_order_relaxed); if (k >= n_) return; (*fn_)(k); } }
    void loop() {
        size_t seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> lk(mu_); cv_.wait(lk, [&] { return quit_ || gen_ != seen; }); if (quit_) return; seen = gen_; }
            take();
            { std::lock_guard<std::mutex> lk(mu_); if (--busy_ == 0) done_.notify_one(); }
        }
    }
};
size_t chunk_size() {
    if (const char *e = getenv("OTTI_SNARK_VERIFY_CHUNK")) { const long v = atol(e); if (v >= 1 && v <= 4096) return (size_t)v; }
    return kSnarkVerifyManyChunk;
}
}  // namespace

void snark_verify_many(const CompComm &comm, const SnarkGens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count, unsigned threads,
                       int32_t *results) {
    snark_verify_staged(comm, g, tlabel, tlabel_len, items, count, threads, results, nullptr);
}
// The staging both callers share.  chunk_end == null: every proof runs its own group equations (snark_verify_many).  Otherwise (snark_verify_batch)
// a proof states them to two collecting sinks, one per generator handle, and the proofs of a chunk that walked to the end without a failure are
// handed to chunk_end on the calling thread, which owes their results; a proof that fails inside the evaluation proof is handed over too, marked,
// because the single verifier would have reported a failing sat equation first.
void snark_verify_staged(const CompComm &comm, const SnarkGens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count, unsigned threads,
                         int32_t *results, const SnarkChunkEnd *chunk_end) {
    if (!count) return;
    if (!threads) threads = kSnarkVerifyManyThreads;
    const bool collect = chunk_end != nullptr;
    const char *runs_env = collect ? getenv("OTTI_VERIFY_BATCH_RUNS") : nullptr;  // "0", read per collecting call: the closing equations' generator terms written out (measurements)
    const bool take_runs = !(runs_env && !strcmp(runs_env, "0"));
    const size_t chunk = chunk_size(), nw = std::min<size_t>({(size_t)threads, (size_t)kVerifyManyMaxThreads, count, chunk});
    Crew crew(nw - 1);
    const bool host_only = !g_row_sums_many_hook || getenv("OTTI_VERIFY_HOST") != nullptr;
    for (size_t c0 = 0; c0 < count; c0 += chunk) {
        const size_t c1 = std::min(count, c0 + chunk);
        // ---- parse and check, item by item, in the single path's order: the inputs' scalars, their count, the dimensions, the proof's bytes
        std::vector<std::unique_ptr<Live>> live; live.reserve(c1 - c0);
        for (size_t i = c0; i < c1; i++) {
            const VerifyItem &it = items[i];
            try {
                auto L = std::make_unique<Live>(); L->item = i;
                if (int rc = item_inputs(it, comm.num_inputs, L->inputs)) { results[i] = rc; continue; }
                if (comm.num_cons != g.num_cons || comm.num_vars != g.num_vars) { results[i] = OTTI_ERR_VERIFY_INTERNAL; continue; }
                L->S = SnarkProof::parse(it.proof, it.proof_len);
                results[i] = OTTI_ERR_INTERNAL;               // until a step has written the verdict
                live.push_back(std::move(L));
            } catch (const Error &e) { results[i] = e.code; }
            catch (...) { results[i] = OTTI_ERR_INTERNAL; }
        }
        // ---- one step of one proof; a failure is the proof's verdict and takes it out of the later passes
        auto step = [&](Live &L, int stage) {
            bool in_eval = false;                             // a failure from here on came after r1cs_verify_host would have run its deferred equations
            auto leave = [&](int code) {
                L.alive = false; L.v.reset(); L.tr.reset();
                if (collect && (code == OTTI_OK || in_eval)) { L.col.walk_code = code; return; }      // chunk_end settles it
                results[L.item] = code; L.col.settled = true;
            };
            try {
                if (stage == 0) {                             // everything snark_verify does before the evaluation proof, then its step 0
                    L.tr = std::make_unique<Transcript>(tlabel, tlabel_len);
                    L.tr->append_protocol_name("Spartan SNARK proof");
                    snark_append_comm(*L.tr, comm);
                    if (collect) { L.col.item = L.item; L.col.sat.accept_runs = L.col.eval.accept_runs = take_runs; }
                    if (int rc = r1cs_verify_host(L.S.r1cs, comm.num_cons, comm.num_vars, L.inputs, L.S.inst_evals, *g.sat, *L.tr, L.rx, L.ry, nullptr, collect ? &L.col.sat : nullptr)) { leave(rc); return; }
                    in_eval = true;
                    L.tr->append_scalar("Ar_claim", L.S.inst_evals[0]); L.tr->append_scalar("Br_claim", L.S.inst_evals[1]); L.tr->append_scalar("Cr_claim", L.S.inst_evals[2]);
                    L.v = std::make_unique<EvalProofVerifier>(L.S.eval, comm, L.rx, L.ry, L.S.inst_evals, g, *L.tr, 0, collect ? &L.col.eval : nullptr);
                    L.req = L.v->begin();
                    return;
                }
                in_eval = true;
                if (L.host_sum) {                             // the route does not change the verdict: the same sum, or the same failure
                    L.ans = RowAnswer();
                    try { L.ans.sum = row_sum_on_host(L.req.C, L.req.n, L.req.s, false); } catch (const VerifyFail &f) { L.ans.code = f.code; }
                }
                if (stage == 1) L.req = L.v->after_derefs(L.ans);
                else if (stage == 2) L.req = L.v->after_ops(L.ans);
                else { L.v->after_mem(L.ans); leave(OTTI_OK); }
            } catch (const VerifyFail &f) { leave(f.code); }
            catch (const Error &e) { leave(e.code); }
            catch (...) { leave(OTTI_ERR_INTERNAL); }
        };
        std::vector<Live *> now; now.reserve(live.size());
        for (auto &L : live) now.push_back(L.get());
        for (int stage = 0; stage <= 3 && !now.empty(); stage++) {
            if (stage > 0) {
                // ---- the seam: every proof still alive has named its sum; those of at least kRowSumDeviceMin points go to the device in one pass
                std::vector<Live *> dev; std::vector<RowRequest> req;
                for (Live *L : now) { L->host_sum = true; if (!host_only && L->req.n >= kRowSumDeviceMin) { dev.push_back(L); req.push_back(L->req); } }
                if (!dev.empty()) {
                    std::vector<RowAnswer> ans(dev.size());
                    bool ok = false;
                    try { ok = g_row_sums_many_hook(comm, req.data(), req.size(), ans.data()); } catch (...) { ok = false; }
                    if (ok) for (size_t k = 0; k < dev.size(); k++) { dev[k]->ans = ans[k]; dev[k]->host_sum = false; }
                }
            }
            crew.run(now.size(), [&](size_t k) { step(*now[k], stage); });
            std::vector<Live *> next;
            for (Live *L : now) if (L->alive) next.push_back(L);
            now.swap(next);
        }
        if (collect) {
            std::vector<SnarkCollected *> done;
            for (auto &L : live) if (!L->col.settled) done.push_back(&L->col);
            if (!done.empty()) (*chunk_end)(done);
        }
    }
}

}  // namespace otti
