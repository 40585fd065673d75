// Many witnesses of one instance proved in one call (device.h nizk_prove_many; the contract: include/otti_spartan.h otti_nizk_prove_many).
// Everything a proof computes before its first challenge depends on the witness alone: the unblinded row sums of its commitment and Az, Bz, Cz.
// The calling thread forms both for a chunk of witnesses in joint passes — the FRONT HALF: one fixed-base MSM launch over the witnesses' rows side by
// side, one walk over the matrices per tile of four witnesses (k_sparse.hip dev_spmv3_many) — and hands each proof a ProveFront, which
// r1cs_prove_device reads where it reads a witness's kept rows and kept products.  The sequential halves run on the library's own workers, one
// proof at a time each, exactly as nizk_prove_resident runs them: the bytes cannot differ, since the row sums are the same group elements (they
// are compressed after the blind's term is added) and the products the same canonical words.
#include "device.h"
#include "prove_many_plan.h"
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <mutex>
#include <thread>

namespace otti {

// Front-half buffers of the calling thread's context: grow-only, reused chunk by chunk — a chunk's are written again only after its proofs are done.
struct ProveManyScratch {
    DevBuf<Fr> z_il, stage, abc, seg_partial;                 // the tile's interleaved vectors; the row jobs' scalars side by side; 3 N per witness lacking products
    DevBuf<Pt> rows;                                          // L per witness lacking rows
    std::vector<hipEvent_t> ev;                               // three per step: before staging, before the pass, behind it
    hipEvent_t event(size_t i) {
        while (ev.size() <= i) { hipEvent_t e; OTTI_HIP(hipEventCreate(&e)); ev.push_back(e); }
        return ev[i];
    }
    template <class T> static void grow(DevCtx &c, DevBuf<T> &b, size_t n) {
        if (b.n >= n) return;
        OTTI_HIP(hipStreamSynchronize(c.stream));             // nothing queued may still read what is replaced
        b.alloc(n);
    }
};

namespace {
// OTTI_PROVE_MANY_GB, read per call: the front half's byte budget (default 8; 0: no front half).  OTTI_PROVE_MANY_FRONT=0 switches it off for A/B runs.
uint64_t front_budget() {
    if (const char *e = getenv("OTTI_PROVE_MANY_FRONT")) if (e[0] == '0' && !e[1]) return 0;
    double gb = 8.0;
    if (const char *e = getenv("OTTI_PROVE_MANY_GB")) { char *end = nullptr; const double v = strtod(e, &end); if (end != e && v >= 0) gb = v; }
    return (uint64_t)(gb * 1073741824.0);
}
struct Geometry { size_t N, V, L, R; };
Geometry geometry(const Instance &I, const Gens &g) {
    const size_t V = I.num_vars, ell = ilog2(V), L = (size_t)1 << (ell / 2), R = (size_t)1 << (ell - ell / 2);
    if (g.num_vars_padded != V || g.R != R) throw Error(OTTI_ERR_BAD_ARG, "generators were made for a different instance size");
    return {I.num_cons, V, L, R};
}
// THE front-half rule: which of the two things are formed jointly at all.  Measured, profiles/prove_many.md (tools/prove_many_probe.py, K = 16, 2^12 /
// 2^16 / 2^20, device-event time of the joint pass over that of the 16 single passes, each beyond the singles' own spread):
//   products  row-per-quad layout (compiled circuits) 0.94 / 0.90 / 0.88: joint.  Row-per-lane layout (one entry per row and matrix) 1.21 / 1.09 /
//             2.38 — putting the vectors side by side costs more than a walk over so few entries saves: such an instance takes the singles.
//   rows      0.09 - 0.12 / 0.24 - 0.32 / 0.67 - 0.87: joint wherever measured.  But at 2^20 what the joint job saves on the device is less than what
//             it loses on the host: a single proof sums its rows and forms its products BEHIND its own tape draws, the front half stands in front
//             of the first proof — sixteen proofs on one thread took 53.0 ms against 44.6 ms for sixteen single calls (compiler-like: 54.7 against
//             49.9) and tied with a caller's pool at four threads and more.  So the front half stops at the largest size at which it was measured
//             to win, 2^16 variables; between 2^16 and 2^20 nothing was measured.
// A witness the rule leaves out is planned as one that has the thing already: its proof forms it, as a single proof does.  Bytes do not depend on it.
// OTTI_PROVE_MANY_RULE=0, read per call, sets the rule aside (everything the plan allows is joint): how the figures above are measured again.
constexpr size_t kProveManyMaxVars = (size_t)1 << 16;
struct FrontRule { bool rows, products; };
FrontRule front_rule(const Instance &I, const Geometry &G) {
    if (const char *e = getenv("OTTI_PROVE_MANY_RULE")) if (e[0] == '0' && !e[1]) return {true, true};
    const bool size_ok = G.V <= kProveManyMaxVars;
    return {size_ok, size_ok && I.dev->by_row.quad()};
}
// One chunk's front half queued on c.stream: the row jobs first (a proof reads its rows first), then the tiles.  front[i] of every witness in a
// job / tile receives its pointers, need[i] the number of steps that must have completed before proof i may start; behind step s the event
// S.event(3 s + 2) is recorded.  Returns the number of steps.  Throws with nothing of front / need to be relied on (the caller clears them).
template <class ZOf>
size_t queue_front(DevCtx &c, ProveManyScratch &S, Instance &I, Gens &g, const Geometry &G, const PmChunk &ch, ZOf z_of, ProveFront *front, size_t *need,
                   otti_prove_many_info &info) {
    const DeviceCsrSet &m = I.dev->by_row;
    size_t np = 0, nr = 0;
    for (const PmTile &t : ch.tiles) np += t.wit.size();
    for (const PmRowJob &j : ch.jobs) nr += j.wit.size();
    if (np) { S.grow(c, S.z_il, kProveManyTile * 2 * G.V); S.grow(c, S.abc, np * 3 * G.N); if (m.n_seg) S.grow(c, S.seg_partial, 3 * kProveManyTile * m.n_seg); }
    if (nr) { S.grow(c, S.stage, nr * G.V); S.grow(c, S.rows, nr * G.L); }
    size_t step = 0, r0 = 0, p0 = 0;
    for (const PmRowJob &j : ch.jobs) {
        const size_t n = j.wit.size();
        OTTI_HIP(hipEventRecord(S.event(3 * step), c.stream));
        for (size_t a = 0; a < n; a++)      // the variable halves side by side: row i of witness a is row a L + i of the joint job
            OTTI_HIP(hipMemcpyAsync(S.stage.p + (r0 + a) * G.V, z_of(j.wit[a]), G.V * sizeof(Fr), hipMemcpyDeviceToDevice, c.stream));
        OTTI_HIP(hipEventRecord(S.event(3 * step + 1), c.stream));
        const MsmJob job{.dense = S.stage.p + r0 * G.V, .n_dense = G.R, .rows = n * G.L, .mode = MSM_KEEP, .sparse = j.sparse, .keep_dst = S.rows.p + r0 * G.L};
        if (info.row_jobs < 4) info.row_kernel[info.row_jobs] = (int32_t)dev_msm_plan(c, *g.dev, job).kernel;
        dev_msm_rows(c, *g.dev, job);
        OTTI_HIP(hipEventRecord(S.event(3 * step + 2), c.stream));
        for (size_t a = 0; a < n; a++) { front[j.wit[a]].rows = S.rows.p + (r0 + a) * G.L; need[j.wit[a]] = step + 1; }
        r0 += n; step++; info.row_jobs++;
    }
    for (const PmTile &t : ch.tiles) {
        const int nt = (int)t.wit.size();
        OTTI_HIP(hipEventRecord(S.event(3 * step), c.stream));
        SpmvManyOut out{};
        for (int a = 0; a < nt; a++) {
            dev_interleave_slot(c, z_of(t.wit[a]), 2 * G.V, S.z_il.p, a);
            for (int k = 0; k < 3; k++) out.o[k][a] = S.abc.p + ((p0 + a) * 3 + k) * G.N;
        }
        OTTI_HIP(hipEventRecord(S.event(3 * step + 1), c.stream));
        dev_spmv3_many(c, m, S.z_il.p, nt, out, S.seg_partial.p);
        OTTI_HIP(hipEventRecord(S.event(3 * step + 2), c.stream));
        for (int a = 0; a < nt; a++) { for (int k = 0; k < 3; k++) front[t.wit[a]].abc[k] = out.o[k][a]; need[t.wit[a]] = step + 1; }
        p0 += (size_t)nt; step++; info.product_tiles++;
    }
    return step;
}
// device-event times of a chunk's steps, once they have completed: [0] staging + interleave, [1] row sums, [2] products
void add_front_ms(ProveManyScratch &S, const PmChunk &ch, size_t steps, otti_prove_many_info &info) {
    for (size_t s = 0; s < steps; s++) {
        float a = 0, b = 0;
        if (hipEventElapsedTime(&a, S.ev[3 * s], S.ev[3 * s + 1]) != hipSuccess || hipEventElapsedTime(&b, S.ev[3 * s + 1], S.ev[3 * s + 2]) != hipSuccess) continue;
        info.front_ms[0] += a; info.front_ms[s < ch.jobs.size() ? 1 : 2] += b;
    }
}
otti_prove_many_info empty_info() { otti_prove_many_info i{}; for (int32_t &k : i.row_kernel) k = -1; return i; }
}  // namespace

void nizk_prove_many(Instance &I, Gens &g, const void *tlabel, size_t tlabel_len, const ProveManyItem *items, size_t count, unsigned threads,
                     std::vector<uint8_t> *proofs, int32_t *results, ProveTimings *tm, otti_prove_many_info &info) {
    info = empty_info();
    if (!count) return;
    const Geometry G = geometry(I, g);
    DevCtx &c = DevCtx::get();
    ensure_device_objects(I, g);
    if (!c.prove_many) c.prove_many = new ProveManyScratch();
    ProveManyScratch &S = *c.prove_many;
    // ---- per item, what the single call would refuse before it touches the device; such an item takes no part in the front half
    const FrontRule rule = front_rule(I, G);
    std::vector<PmWitness> pw(count);
    std::vector<char> refused(count, 0);
    for (size_t i = 0; i < count; i++) {
        const DeviceWitness &w = *items[i].wit;
        if (w.z.n != 2 * G.V) { results[i] = OTTI_ERR_INVALID_NUM_VARS; refused[i] = 1; }
        else if (w.inputs.size() != I.num_inputs) { results[i] = OTTI_ERR_INVALID_NUM_INPUTS; refused[i] = 1; }
        else results[i] = OTTI_ERR_INTERNAL;                  // until its worker has written the outcome
        pw[i].has_rows = refused[i] || !rule.rows || w.rows_kept_for(g); pw[i].has_products = refused[i] || !rule.products || w.products_kept_for(I);
        pw[i].sparse = w.small_fraction > kSparseWitness;
    }
    const PmPlan plan = prove_many_plan(count, G.N, G.V, G.L, G.R, pw.data(), front_budget());
    info.chunks = (uint32_t)plan.chunks.size();
    if (!threads) threads = kProveManyThreads;
    const size_t nw = std::min<size_t>({(size_t)threads, (size_t)kProveManyMaxThreads, count});

    // ---- what the calling thread hands the workers.  A worker starts proof i only after the launches that write i's front buffers have COMPLETED:
    // the calling thread synchronises with the event behind the step and then publishes the item under the mutex (a host publish behind an event
    // synchronise, as verify.h's ManyEvals::publish does it), so the worker's stream needs no event of another context to wait on.  With one
    // thread everything is on one stream, whose order does the same.
    struct Shared {
        std::mutex mu; std::condition_variable cv;
        std::vector<char> go;                                 // item i's front record is final: its proof may start
        std::vector<size_t> chunk_left;                       // proofs of chunk k still to finish (its buffers are theirs until then)
        size_t next = 0;
    } sh;
    std::vector<ProveFront> front(count);
    std::vector<size_t> need(count, 0), chunk_of(count, 0);
    sh.go.assign(count, 1); sh.chunk_left.resize(plan.chunks.size());
    for (size_t k = 0; k < plan.chunks.size(); k++) {
        const PmChunk &ch = plan.chunks[k];
        sh.chunk_left[k] = ch.count;
        for (size_t i = ch.first; i < ch.first + ch.count; i++) chunk_of[i] = k;
        for (const PmRowJob &j : ch.jobs) for (uint32_t i : j.wit) sh.go[i] = 0;      // waits for its steps; everybody else may start at once
        for (const PmTile &t : ch.tiles) for (uint32_t i : t.wit) sh.go[i] = 0;
    }
    std::atomic<uint32_t> rows_used{0}, prods_used{0};
    auto prove_item = [&](size_t i) {
        if (!refused[i]) {
            {   std::unique_lock<std::mutex> lk(sh.mu); sh.cv.wait(lk, [&] { return sh.go[i] != 0; }); }
            const ProveFront f = front[i];
            try {
                ProveTimings t{};
                proofs[i] = nizk_prove_resident(I, *items[i].wit, g, tlabel, tlabel_len, items[i].seed32, &t, nullptr, &f);
                if (tm) tm[i] = t;
                results[i] = OTTI_OK;
                if (f.rows) rows_used.fetch_add(1, std::memory_order_relaxed);
                if (f.abc[0]) prods_used.fetch_add(1, std::memory_order_relaxed);
            } catch (const Error &e) { results[i] = e.code; proofs[i].clear(); }
            catch (...) { results[i] = OTTI_ERR_INTERNAL; proofs[i].clear(); }
        }
        { std::lock_guard<std::mutex> lk(sh.mu); sh.chunk_left[chunk_of[i]]--; }
        sh.cv.notify_all();
    };
    auto take = [&](size_t limit) -> long {                  // the next item below `limit`, or -1
        std::lock_guard<std::mutex> lk(sh.mu);
        return sh.next < limit ? (long)sh.next++ : -1;
    };
    std::vector<std::thread> th;
    struct Join {                                             // on every way out: whoever still waits is let go without a front, and joined
        std::vector<std::thread> &th; Shared &sh; std::vector<ProveFront> &front;
        ~Join() {
            { std::lock_guard<std::mutex> lk(sh.mu); for (size_t i = 0; i < sh.go.size(); i++) if (!sh.go[i]) { front[i] = ProveFront{}; sh.go[i] = 1; } }
            sh.cv.notify_all();
            for (auto &t : th) if (t.joinable()) t.join();
        }
    } join{th, sh, front};
    th.reserve(nw);
    for (size_t w = 1; w < nw; w++) {
        try { th.emplace_back([&] { for (long i; (i = take(count)) >= 0;) prove_item((size_t)i); }); }
        catch (const std::system_error &) { break; }          // short of threads: those that started share the work
    }
    info.workers = (uint32_t)th.size() + 1;
    const bool alone = th.empty();

    for (size_t k = 0; k < plan.chunks.size(); k++) {
        const PmChunk &ch = plan.chunks[k];
        size_t steps = 0;
        if (!ch.jobs.empty() || !ch.tiles.empty()) {
            // the buffers are still those of the chunks before: their proofs have to be done (alone, they are: this thread ran them)
            if (k) { std::unique_lock<std::mutex> lk(sh.mu); sh.cv.wait(lk, [&] { for (size_t j = 0; j < k; j++) if (sh.chunk_left[j]) return false; return true; }); }
            bool ok = true;
            try { steps = queue_front(c, S, I, g, G, ch, [&](uint32_t i) { return (const Fr *)items[i].wit->z.p; }, front.data(), need.data(), info); }
            catch (...) { ok = false; }
            if (!ok) {
                // a front half that gave up (HBM short, say) is no error: the chunk's proofs form their own rows and products, as single proofs do
                (void)hipStreamSynchronize(c.stream);
                (void)hipGetLastError();
                info.front_failed++;
                std::lock_guard<std::mutex> lk(sh.mu);
                for (size_t i = ch.first; i < ch.first + ch.count; i++) { front[i] = ProveFront{}; sh.go[i] = 1; }
                steps = 0;
            } else if (alone) {
                std::lock_guard<std::mutex> lk(sh.mu);
                for (size_t i = ch.first; i < ch.first + ch.count; i++) sh.go[i] = 1;
            } else {
                // proofs of the first steps start while the later ones are summed
                for (size_t s = 0; s < steps; s++) {
                    OTTI_HIP(hipEventSynchronize(S.ev[3 * s + 2]));
                    { std::lock_guard<std::mutex> lk(sh.mu); for (size_t i = ch.first; i < ch.first + ch.count; i++) if (!sh.go[i] && need[i] <= s + 1) sh.go[i] = 1; }
                    sh.cv.notify_all();
                }
            }
            sh.cv.notify_all();
        }
        for (long i; (i = take(ch.first + ch.count)) >= 0;) prove_item((size_t)i);
        if (steps) {
            if (alone) OTTI_HIP(hipStreamSynchronize(c.stream));
            add_front_ms(S, ch, steps, info);
        }
    }
    for (auto &t : th) t.join();
    th.clear();
    info.rows_from_front = rows_used.load(); info.products_from_front = prods_used.load();
}

void prove_front_staged(Instance &I, Gens &g, const Fr *const *zs, const int32_t *small, size_t K, Pt *rows, Fr *const abc[3], otti_prove_many_info &info) {
    info = empty_info();
    if (!K) return;
    const Geometry G = geometry(I, g);
    DevCtx &c = DevCtx::get();
    ensure_device_objects(I, g);
    if (!c.prove_many) c.prove_many = new ProveManyScratch();
    ProveManyScratch &S = *c.prove_many;
    std::vector<PmWitness> pw(K);
    const FrontRule rule = front_rule(I, G);
    for (size_t i = 0; i < K; i++) { pw[i].sparse = small[i] != 0; pw[i].has_rows = !rule.rows; pw[i].has_products = !rule.products; }
    const PmPlan plan = prove_many_plan(K, G.N, G.V, G.L, G.R, pw.data(), front_budget());
    info.chunks = (uint32_t)plan.chunks.size(); info.workers = 1;
    std::vector<ProveFront> front(K); std::vector<size_t> need(K, 0);
    for (const PmChunk &ch : plan.chunks) {
        const size_t steps = queue_front(c, S, I, g, G, ch, [&](uint32_t i) { return zs[i]; }, front.data(), need.data(), info);
        for (size_t i = ch.first; i < ch.first + ch.count; i++) {
            // what the plan leaves to a proof is formed as the proof forms it, so the caller's arrays are whole
            if (front[i].rows) { OTTI_HIP(hipMemcpyAsync(rows + i * G.L, front[i].rows, G.L * sizeof(Pt), hipMemcpyDeviceToDevice, c.stream)); info.rows_from_front++; }
            else dev_msm_rows(c, *g.dev, {.dense = zs[i], .n_dense = G.R, .rows = G.L, .mode = MSM_KEEP, .sparse = pw[i].sparse, .keep_dst = rows + i * G.L});
            if (front[i].abc[0]) { for (int k = 0; k < 3; k++) OTTI_HIP(hipMemcpyAsync(abc[k] + i * G.N, front[i].abc[k], G.N * sizeof(Fr), hipMemcpyDeviceToDevice, c.stream)); info.products_from_front++; }
            else dev_spmv3(c, I.dev->by_row, zs[i], abc[0] + i * G.N, abc[1] + i * G.N, abc[2] + i * G.N, false, nullptr);
        }
        OTTI_HIP(hipStreamSynchronize(c.stream));
        add_front_ms(S, ch, steps, info);
    }
}

}  // namespace otti
