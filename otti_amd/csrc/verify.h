// The host verifiers' toolkit, defined in spartan_host.cpp: what NIZK::verify, SNARK::verify (snark_host.cpp) and the two batched verifiers
// (verify_many.cpp, snark_verify_many.cpp) are all built from.
#pragma once
#include "spartan.h"
#include "cpu_relax.h"
#include "batch_terms.h"
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <system_error>
#include <thread>
#include <vector>

namespace otti {

struct VerifyFail { int code; };
Pt dec(const CPoint &c);                                     // throws VerifyFail{OTTI_ERR_VERIFY_DECOMPRESS}
void require(bool ok);                                       // throws VerifyFail{OTTI_ERR_VERIFY_INTERNAL}
Pt host_msm_wide(const Fr *sc, const Pt *pts, size_t n);
// sum_i s[i] * decode(C[i]) over the row commitments of a polynomial commitment (PolyEvalProof::verify's C_LZ).  Construct it as soon as
// the commitments are known (with a device their decompression starts right away, spartan.h RowSumBeginHook), call finish() when the
// scalars are; without a device, or when it declines, both steps run on the host cores inside finish().  Throws VerifyFail.
struct RowSum {
    RowSumJob *job = nullptr; const CPoint *C; size_t n;
    RowSum(const CPoint *C_, size_t n_);
    RowSum(const RowSum &) = delete; RowSum &operator=(const RowSum &) = delete;
    ~RowSum();
    Pt finish(const Fr *s);
};
// The same equations stated instead of run: each site that hands a check to Deferred below also knows it as a term list  sum_j s_j P_j = identity
// (batch_terms.h), and a Deferred built over a TermSink takes that list and no closure — nothing is decoded, multiplied or compared on the walk.
// verify_batch.cpp sums the lists of many proofs under random weights in one multi-scalar multiplication.
struct TermSink : BtEquations {
    using BtEquations::point;
    void point(const Fr &s, const CPoint &c) { BtEquations::point(s, c.b); }
};
// Group equations that do not feed the transcript — most of the verifier's arithmetic: per sum-check round two checks with a
// variable-base scalar multiplication each — are handed to a few background threads AS THEY ARISE, while the calling thread walks on
// through the rounds (whose hashed commitments are the sequential path); finish() drains what is left and reports the first failure — the
// failing check that was handed over EARLIEST, whichever thread found its failure first: a proof with several defects gets one code, the same in
// every run and beside any number of other verifiers (verify_many.cpp holds its results against the single verifier's, code for code).
// Lock-free: the producer fills a slot and bumps `count`; workers claim slots with a compare-exchange on `next`.
class Deferred {
public:
    // workers < 0: the default rule below.  0: no threads at all — everything handed over runs in finish(), on the thread that calls it (a proof
    // parked between the steps of snark_verify_many owns no thread); the failure reported is the same either way.
    explicit Deferred(int workers = -1) {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        unsigned nw = hw >= 12 ? 6 : hw >= 6 ? hw - 3 : 0;                // beside the caller and its spinning helpers (pool.h)
        if (const char *e = getenv("OTTI_VERIFY_THREADS")) { int v = atoi(e); if (v >= 0 && v <= 32) nw = (unsigned)v; }
        if (workers >= 0) nw = (unsigned)workers;
        try { for (unsigned i = 0; i < nw; i++) th_.emplace_back([this] { work(false); }); } catch (const std::system_error &) {}
    }
    // collecting: no threads, no closures — the sites state their checks to `s` (nullptr: the default rule above, as Deferred())
    explicit Deferred(TermSink *s) : Deferred(s ? 0 : -1) { sink = s; }
    TermSink *sink = nullptr;
    Deferred(const Deferred &) = delete; Deferred &operator=(const Deferred &) = delete;
    ~Deferred() { closing_.store(true, std::memory_order_release); for (auto &t : th_) t.join(); }
    void push_back(std::function<void()> f) {
        const size_t c = count_.load(std::memory_order_relaxed);
        if (c >= kSlots) { run_one(f, kSlots); return; }                          // (never in practice: two checks per round, at most 2 x 64 rounds + a few)
        items_[c] = std::move(f);
        count_.store(c + 1, std::memory_order_release);
    }
    void finish() {                                                       // throws VerifyFail
        closing_.store(true, std::memory_order_release);
        work(true);
        for (auto &t : th_) t.join();
        th_.clear();
        if (const uint64_t f = first_.load()) throw VerifyFail{(int)(int32_t)(uint32_t)f};
    }
private:
    static constexpr size_t kSlots = 512;
    std::function<void()> items_[kSlots];
    std::atomic<size_t> count_{0}, next_{0};
    std::atomic<bool> closing_{false};
    std::atomic<uint64_t> first_{0};                                      // 0: no failure; else (slot + 1) << 32 | code of the failure in the lowest slot
    std::vector<std::thread> th_;
    void failed(size_t slot, int code) {
        const uint64_t mine = ((uint64_t)(slot + 1) << 32) | (uint32_t)code;
        uint64_t cur = first_.load(std::memory_order_relaxed);
        while ((cur == 0 || mine < cur) && !first_.compare_exchange_weak(cur, mine, std::memory_order_acq_rel)) {}
    }
    void run_one(const std::function<void()> &f, size_t slot) {
        try { f(); } catch (const VerifyFail &e) { failed(slot, e.code); } catch (...) { failed(slot, (int)OTTI_ERR_VERIFY_INTERNAL); }
    }
    void work(bool until_empty) {
        for (;;) {
            size_t i = next_.load(std::memory_order_relaxed);
            if (i < count_.load(std::memory_order_acquire)) { if (next_.compare_exchange_weak(i, i + 1, std::memory_order_acq_rel)) run_one(items_[i], i); continue; }
            if (until_empty || closing_.load(std::memory_order_acquire)) { if (next_.load() >= count_.load(std::memory_order_acquire)) return; continue; }
            cpu_relax();
        }
    }
};
void dotproductlog_verify(const DotProductProofLog &pf, size_t n, const Gens &g, const PcView &v, Transcript &tr, const Fr *a, const CPoint &Cx, const CPoint &Cy, Deferred *later = nullptr);
// RowSum's host path alone: decompression and Pippenger on the host cores.  wide: striped over up to 16 threads of its own (the single verifier);
// otherwise on the calling thread alone (snark_verify_many's workers are the parallelism there).  Throws VerifyFail{OTTI_ERR_VERIFY_DECOMPRESS}.
Pt row_sum_on_host(const CPoint *C, size_t n, const Fr *s, bool wide);

// R1CSProof::verify, shared by both modes: `tr` already carries the caller's protocol name; returns 0 and the challenges the transcript produced.
// sink: the group equations that feed nothing hashed are stated to it as term lists and NOT checked here (0 then says: the walk met no failure).
int r1cs_verify_host(const NizkProof &P, size_t N, size_t V, const std::vector<Fr> &inputs, const Fr inst_evals[3], const Gens &g, Transcript &tr,
                     std::vector<Fr> &rx, std::vector<Fr> &ry, const InstEvalFetch *fetch = nullptr, TermSink *sink = nullptr);

// What both batched verifiers check of an item before they parse its proof, in the single path's order: the arguments, the inputs' scalars
// (inputs32 are canonical bytes: a scalar >= l is OTTI_ERR_INVALID_SCALAR, as the C entry reports it), their count.  0: `inputs` is filled.
inline int item_inputs(const VerifyItem &it, size_t num_inputs, std::vector<Fr> &inputs) {
    if (!it.proof || (it.ninputs && !it.inputs32)) return OTTI_ERR_BAD_ARG;
    inputs.resize(it.ninputs);
    for (size_t j = 0; j < it.ninputs; j++) if (!fr_from_bytes(inputs[j], it.inputs32 + 32 * j)) return OTTI_ERR_INVALID_SCALAR;
    if (it.ninputs != num_inputs) return OTTI_ERR_INVALID_NUM_INPUTS;
    return OTTI_OK;
}

// The evaluation of A, B, C at the points of many proofs of one instance, as both batched NIZK verifiers use it (verify_many.cpp, verify_batch.cpp):
// queued by the constructing thread through the hooks of spartan.h when the instance has at least 4096 constraints and a device is present — the
// rule of the single path — and collected by that thread tile by tile; the workers wait for their proof's tile.  Where nothing was queued, or the
// device lets go of the batch, a proof is evaluated on the host by whoever asks for it.
struct ManyEvals {
    const Instance &I; const std::vector<const NizkProof *> pts; bool queued = false;
    std::mutex mu; std::condition_variable cv;
    size_t done = 0; bool failed = false;                     // triples of proofs [0, done) hold their values; failed: the rest evaluate on the host
    std::vector<Fr> triples;                                  // 3 per proof
    ManyEvals(const Instance &I_, std::vector<const NizkProof *> pts_) : I(I_), pts(std::move(pts_)) {
        if (I.num_cons >= 4096 && g_inst_eval_many_begin_hook && g_inst_eval_many_next_hook) { try { queued = g_inst_eval_many_begin_hook(I, pts); } catch (...) { queued = false; } }
        if (queued) triples.resize(3 * pts.size()); else failed = true;
    }
    void publish(size_t d, bool f) { { std::lock_guard<std::mutex> lk(mu); done = d; failed = f; } cv.notify_all(); }
    bool wait(size_t k) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return done > k || failed; }); return done > k; }
    void collect_next() {                                     // on the constructing thread: one more tile's values, published
        long d = -1;
        try { d = g_inst_eval_many_next_hook(reinterpret_cast<Fr (*)[3]>(triples.data())); } catch (...) { d = -1; }
        if (d < 0 || (size_t)d <= done) publish(done, true); else publish((size_t)d, false);
    }
    void collect_rest() { while (!failed && done < pts.size()) collect_next(); }   // proofs that failed before their closing step: the queued work still has to drain
    void let_go() { if (done * 3 < triples.size() && !failed) publish(done, true); }   // no more tiles will come: waiting workers evaluate on the host
    void take(size_t k, Fr out[3]) const { for (int j = 0; j < 3; j++) out[j] = triples[3 * k + j]; }
    void on_host(size_t k, Fr out[3]) const { I.evaluate(pts[k]->rx, pts[k]->ry, out); }
    void fetch_on_worker(size_t k, Fr out[3]) { if (wait(k)) take(k, out); else on_host(k, out); }
    void fetch_on_caller(size_t k, Fr out[3]) {               // the constructing thread walks the proofs itself: the evaluation is collected where proof k needs it
        while (!failed && done <= k) collect_next();
        if (done > k) take(k, out); else on_host(k, out);
    }
};

}  // namespace otti
