// The host verifiers' toolkit, defined in spartan_host.cpp: what NIZK::verify, SNARK::verify (snark_host.cpp) and the batched verifiers
// (verify_many.cpp, verify_batch.cpp, snark_verify_many.cpp) are all built from.
#pragma once
#include "spartan.h"
#include "cpu_relax.h"
#include "batch_terms.h"
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
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
// A group equation that feeds nothing hashed is stated ONCE, as a term list  sum_j s_j P_j = identity  (batch_terms.h): a scalar with a point, named
// by its 32-byte encoding, or with a generator slot of g.P.  Deferred::equation below either runs the list (term_sum, then the identity test) or,
// built over a BtEquations, appends it and runs nothing — verify_batch.cpp sums the lists of many proofs under random weights in one
// multi-scalar multiplication.  A list owns its encodings: nothing it names has to outlive the site that stated it.
inline BtTerm term(const Fr &s, const CPoint &c) { return bt_point(s, c.b); }
inline BtTerm term(const Fr &s, uint32_t slot) { return bt_gen(s, slot); }
// the sum of n terms, in one host_msm.  Throws VerifyFail: OTTI_ERR_VERIFY_DECOMPRESS for an encoding that does not decode,
// OTTI_ERR_VERIFY_INTERNAL for a slot past g.P
Pt term_sum(const BtTerm *t, size_t n, const Gens &g);
inline void require_identity(const Pt &sum) { require(pt_eq(sum, pt_identity())); }
// Group equations that do not feed the transcript — most of the verifier's arithmetic: per sum-check round two checks with a
// small multi-scalar multiplication each — are handed to a few background threads AS THEY ARISE, while the calling thread walks on
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
    // collecting: no threads, and equation() appends to `s` instead of running (nullptr: the default rule above, as Deferred())
    explicit Deferred(BtEquations *s) : Deferred(s ? 0 : -1) { sink = s; }
    BtEquations *sink = nullptr;
    Deferred(const Deferred &) = delete; Deferred &operator=(const Deferred &) = delete;
    ~Deferred() { closing_.store(true, std::memory_order_release); for (auto &t : th_) t.join(); }
    // one group equation, one slot: the job owns the list
    void equation(const Gens &g, std::vector<BtTerm> e) {
        if (sink) { sink->equation(e); return; }
        push_back([gp = &g, e = std::move(e)] { require_identity(term_sum(e.data(), e.size(), *gp)); });
    }
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
// the sigma protocols' verifiers (nizk/mod.rs): the transcript part runs, the group equations go to `later`
void knowledge_verify(const KnowledgeProof &pf, const Gens &g, Transcript &tr, const CPoint &C, Deferred &later);
void equality_verify(const EqualityProof &pf, const Gens &g, Transcript &tr, const CPoint &C1, const CPoint &C2, Deferred &later);
void product_verify(const ProductProof &pf, const Gens &g, Transcript &tr, const CPoint &X, const CPoint &Y, const CPoint &Z, Deferred &later);
void dotproduct_verify(const DotProductProof &pf, const Gens &g, const GensView &gn, Transcript &tr, const Fr *a, size_t n, const CPoint &Cx, const CPoint &Cy, Deferred &later);
// a_point: the lg n coordinates `a` is the eq table of, when it is one (a collector that takes runs then needs neither `a` nor the n scalars s)
void dotproductlog_verify(const DotProductProofLog &pf, size_t n, const Gens &g, const PcView &v, Transcript &tr, const Fr *a, const CPoint &Cx, const CPoint &Cy, Deferred *later = nullptr,
                          const Fr *a_point = nullptr);
Fr dotproductlog_a_hat(const Fr *r, const Fr *ch2, size_t lg, const Fr &allinv);     // <eq_evals_host(r, lg), s> in closed form: ch2 the squared challenges, allinv = s[0]
// RowSum's host path alone: decompression and Pippenger on the host cores.  wide: striped over up to 16 threads of its own (the single verifier);
// otherwise on the calling thread alone (snark_verify_many's workers are the parallelism there).  Throws VerifyFail{OTTI_ERR_VERIFY_DECOMPRESS}.
Pt row_sum_on_host(const CPoint *C, size_t n, const Fr *s, bool wide);

// R1CSProof::verify, shared by both modes: `tr` already carries the caller's protocol name; returns 0 and the challenges the transcript produced.
// sink: the group equations that feed nothing hashed are stated to it as term lists and NOT checked here (0 then says: the walk met no failure).
int r1cs_verify_host(const NizkProof &P, size_t N, size_t V, const std::vector<Fr> &inputs, const Fr inst_evals[3], const Gens &g, Transcript &tr,
                     std::vector<Fr> &rx, std::vector<Fr> &ry, const InstEvalFetch *fetch = nullptr, BtEquations *sink = nullptr);

// What both batched verifiers check of an item before they parse its proof, in the single path's order: the arguments, the inputs' scalars
// (inputs32 are canonical bytes: a scalar >= l is OTTI_ERR_INVALID_SCALAR, as the C entry reports it), their count.  0: `inputs` is filled.
inline int item_inputs(const VerifyItem &it, size_t num_inputs, std::vector<Fr> &inputs) {
    if (!it.proof || (it.ninputs && !it.inputs32)) return OTTI_ERR_BAD_ARG;
    inputs.resize(it.ninputs);
    for (size_t j = 0; j < it.ninputs; j++) if (!fr_from_bytes(inputs[j], it.inputs32 + 32 * j)) return OTTI_ERR_INVALID_SCALAR;
    if (it.ninputs != num_inputs) return OTTI_ERR_INVALID_NUM_INPUTS;
    return OTTI_OK;
}
// How both batched NIZK verifiers open: parse and check, item by item, in the single path's order — the inputs' scalars, their count, the proof's
// bytes, its challenge lengths.  An item that fails has its code in results[]; the others come back live (Live: LiveProof or a struct derived
// from it), in the items' order, with OTTI_ERR_INTERNAL as their result until they are settled.
struct LiveProof { size_t item; std::vector<Fr> inputs; NizkProof P; };
template <class Live> std::vector<std::unique_ptr<Live>> parse_items(const Instance &I, const VerifyItem *items, size_t count, int32_t *results) {
    const size_t nrx = ilog2(I.num_cons), nry = ilog2(2 * I.num_vars);
    std::vector<std::unique_ptr<Live>> live; live.reserve(count);
    for (size_t i = 0; i < count; i++) {
        const VerifyItem &it = items[i];
        try {
            auto L = std::make_unique<Live>(); L->item = i;
            if (int rc = item_inputs(it, I.num_inputs, L->inputs)) { results[i] = rc; continue; }
            L->P = NizkProof::parse(it.proof, it.proof_len);
            if (L->P.rx.size() != nrx || L->P.ry.size() != nry) { results[i] = OTTI_ERR_VERIFY_INTERNAL; continue; }
            results[i] = OTTI_ERR_INTERNAL;
            live.push_back(std::move(L));
        } catch (const Error &e) { results[i] = e.code; }
        catch (...) { results[i] = OTTI_ERR_INTERNAL; }
    }
    return live;
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
// walk(k, fetch) for every proof k of `ev`, each once; fetch is null where nothing was queued.  Up to nw workers take the proofs in order by an atomic
// counter while the calling thread, which constructed `ev`, collects its tiles; short of threads, those that started share the work.  nw <= 1:
// the calling thread alone, in the single path's order — the evaluation is collected where the first proof needs it.  walk must not throw.
template <class Walk> void walk_proofs(ManyEvals &ev, size_t nw, Walk &&walk) {
    const size_t n = ev.pts.size();
    if (nw <= 1) {
        for (size_t k = 0; k < n; k++) {
            const InstEvalFetch fetch([&ev, k](Fr out[3]) { ev.fetch_on_caller(k, out); });
            walk(k, ev.queued ? &fetch : nullptr);
        }
        ev.collect_rest();
        return;
    }
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t k; (k = next.fetch_add(1, std::memory_order_relaxed)) < n;) {
            const InstEvalFetch fetch([&ev, k](Fr out[3]) { ev.fetch_on_worker(k, out); });
            walk(k, ev.queued ? &fetch : nullptr);
        }
    };
    std::vector<std::thread> th; th.reserve(nw);
    struct Join { std::vector<std::thread> &th; ManyEvals &ev; ~Join() { ev.let_go(); for (auto &t : th) if (t.joinable()) t.join(); } } join{th, ev};
    for (size_t w = 0; w < nw; w++) { try { th.emplace_back(work); } catch (const std::system_error &) { break; } }
    ev.collect_rest();
    if (th.empty()) work();
}

}  // namespace otti
