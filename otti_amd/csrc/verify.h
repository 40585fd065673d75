// The host verifiers' toolkit, defined in spartan_host.cpp: what NIZK::verify, SNARK::verify (snark_host.cpp) and the two batched verifiers
// (verify_many.cpp, snark_verify_many.cpp) are all built from.
#pragma once
#include "spartan.h"
#include "cpu_relax.h"
#include <algorithm>
#include <atomic>
#include <functional>
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

// R1CSProof::verify, shared by both modes: `tr` already carries the caller's protocol name; returns 0 and the challenges the transcript produced
int r1cs_verify_host(const NizkProof &P, size_t N, size_t V, const std::vector<Fr> &inputs, const Fr inst_evals[3], const Gens &g, Transcript &tr,
                     std::vector<Fr> &rx, std::vector<Fr> &ry, const InstEvalFetch *fetch = nullptr);

// What both batched verifiers check of an item before they parse its proof, in the single path's order: the arguments, the inputs' scalars
// (inputs32 are canonical bytes: a scalar >= l is OTTI_ERR_INVALID_SCALAR, as the C entry reports it), their count.  0: `inputs` is filled.
inline int item_inputs(const VerifyItem &it, size_t num_inputs, std::vector<Fr> &inputs) {
    if (!it.proof || (it.ninputs && !it.inputs32)) return OTTI_ERR_BAD_ARG;
    inputs.resize(it.ninputs);
    for (size_t j = 0; j < it.ninputs; j++) if (!fr_from_bytes(inputs[j], it.inputs32 + 32 * j)) return OTTI_ERR_INVALID_SCALAR;
    if (it.ninputs != num_inputs) return OTTI_ERR_INVALID_NUM_INPUTS;
    return OTTI_OK;
}

}  // namespace otti
