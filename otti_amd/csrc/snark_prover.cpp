// SNARK mode on the MI355X: SNARK::prove = R1CSProof (prover.cpp, the NIZK device path) + R1CSEvalProof.  Follows upstream libspartan
// src/lib.rs, src/r1csinstance.rs, src/sparse_mlpoly.rs step for step [RECALL]; see snark.h.
// SNARK::encode / attach are in snark_encode.cpp, the product circuits and their batched sum-check in snark_pc.cpp.
//
// Data flow of R1CSEvalProof: the dense representation of A, B, C (addresses, timestamps, values: 16 N + 2 M field elements) and the
// two generator window tables stay in HBM; per proof the device builds eq(rx), eq(ry), dereferences them by address (6 N elements, committed
// with the bulk MSM), hashes 12 operation vectors and 4 memory vectors into product circuits (about 24 N + 8 M elements with all layers),
// and plays the layered sum-checks: every round is ONE launch over all tables of the batch (fold by the previous challenge + this round's
// sums, pcbatch_prove), the last rounds of every layer on the host; the host only hashes four scalars per round (this sum-check is
// not zero-knowledge: no commitments on the sequential path).  The three closing polynomial-evaluation proofs reuse the log-size dot-product prover of NIZK mode.
#include "snark_prover.h"
#include <sched.h>
#include "pool.h"
#include <thread>
#include <condition_variable>
#include <mutex>

namespace otti {

namespace {
// PolyEvalProof::prove(poly, None, r, Zr, None, gens, ..) on a polynomial resident in HBM
// chunks (optional): the bound's chunk sums over eq of the left point's variables a .. (dev_poly_bound_chunks, computed ahead of time: the point's first
// a variables are the last to be drawn) — the bound is then a 2^a-row one over them
DotProductProofLog polyeval_prove_plain(DevCtx &c, Gens &gens, const PcSet &s, const Fr *Z, const std::vector<Fr> &r, const Fr &Zr, Transcript &tr, RandomTape &tape,
                                        const Fr *chunks = nullptr, size_t a_first = 0) {
    if (r.size() != s.num_vars) throw Error(OTTI_ERR_INTERNAL, "evaluation point of the wrong length");
    tr.append_protocol_name("polynomial evaluation proof");
    const size_t lv = s.num_vars / 2, lgR = ilog2(s.R);
    SnarkScratch &W = snark_workspace(c);
    Fr *Lv = W.get(SS_PE0 + 0, s.L), *Rv = W.get(SS_PE0 + 1, s.R), *LZ = W.get(SS_PE0 + 2, s.R), *a = W.get(SS_PE0 + 3, s.R), *sbuf = W.get(SS_PE0 + 4, s.R),
       *b2 = W.get(SS_PE0 + 5, s.R), *s2 = W.get(SS_PE0 + 6, s.R), *rows = W.get(SS_PE0 + 7, 2 * s.R), *extras = W.get(SS_PE0 + 8, 4 * (lgR + 1)),
       *eqs = W.get(SS_PE0 + 9, 5 * 4096), *bound = W.get(SS_PE0 + 10, 64 * s.R);
    if (chunks) {
        dev_eq_evals2(c, r.data(), a_first, Lv, r.data() + lv, s.num_vars - lv, Rv, eqs);
        dev_poly_bound(c, chunks, (size_t)1 << a_first, s.R, Lv, LZ, bound);
    } else {
        dev_eq_evals2(c, r.data(), lv, Lv, r.data() + lv, s.num_vars - lv, Rv, eqs);
        dev_poly_bound(c, Z, s.L, s.R, Lv, LZ, bound);
    }
    const PcView pv = {s.h_n, s.g1, s.h1, s.R};
    const PeBufs pb = {LZ, Rv, a, sbuf, b2, s2, rows, extras};
    CPoint Cy;
    return dplog_prove_device(c, *gens.dev, gens, pv, pb, fr_zero(), &Zr, fr_zero(), Cy, tr, tape);
}

// ---- the row half of the derefs commitment, ahead of time.  The dereferenced polynomial is [eq(rx) at the row addresses of A, B, C |
// eq(ry) at the column addresses | zeros]: its first 3 N / R commitment rows depend on rx alone, which the R1CS proof fixes at the end
// of its FIRST sum-check — and everything the proof does after that (sigma protocols, second sum-check, evaluation proof: ~2 ms at 2^20)
// is a chain of latency-bound rounds that leaves the chip idle.  A helper thread with a device context of its own therefore sums those
// rows meanwhile (3.2 ms of the chip's multiplier), on a stream confined to 192 of the 256 CUs (hipExtStreamCreateWithCUMask) so that the rounds keep
// CUs to themselves — a fixed-base MSM workgroup holds its CU for ~2 ms, and without the mask a round's kernel waits for one to end;
// the column half is committed by the proving thread once ry is known, both launches sharing the chip.
struct RowsAhead {
    Gens &gens; const Fr *Z; size_t R, rows;
    std::thread th; std::mutex mu; std::condition_variable cv; int stage = 0;      // 1: the rows' scalars are on their way (ev recorded), -1: cancelled
    hipEvent_t ev = nullptr; std::vector<CPoint> C; std::exception_ptr err; bool done = false;
    RowsAhead(Gens &g, const Fr *Z_, size_t R_, size_t rows_) : gens(g), Z(Z_), R(R_), rows(rows_) {
        OTTI_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        th = std::thread([this] { run(); });
    }
    ~RowsAhead() { { std::lock_guard<std::mutex> lk(mu); if (stage == 0) stage = -1; } cv.notify_all(); if (th.joinable()) th.join(); if (ev) (void)hipEventDestroy(ev); }
    bool recorded = false;
    void record(hipStream_t producer) { OTTI_HIP(hipEventRecord(ev, producer)); recorded = true; }   // the scalars are complete once `producer` reaches this point
    void release() {                                              // start summing (after record)
        if (!recorded) return;
        { std::lock_guard<std::mutex> lk(mu); if (stage == 0) stage = 1; }
        cv.notify_all();
    }
    std::vector<CPoint> take() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done; });
        if (err) std::rethrow_exception(err);
        return std::move(C);
    }
    static hipStream_t masked_stream() { return bulk_masked_stream(); }   // k_context.hip: ONE CU-masked stream for the process
    void run() {
        try {
            {   // created inside the prover's session: give back the affinity the session narrowed (this thread waits on the GPU, it does not belong on the helpers' cores)
                cpu_set_t all; CPU_ZERO(&all); for (int i = 0; i < CPU_SETSIZE; i++) CPU_SET(i, &all);
                (void)sched_setaffinity(0, sizeof all, &all);
            }
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return stage != 0; }); if (stage < 0) { done = true; cv.notify_all(); return; } }
            DevCtx &hc = DevCtx::get();                           // this thread's own context: its own MSM partials, point buffers, stream
            hipStream_t own = hc.stream, ms = masked_stream();
            struct Restore { DevCtx &c; hipStream_t s; ~Restore() { c.stream = s; } } restore{hc, own};
            if (ms) hc.stream = ms;
            const bool trace = getenv("OTTI_TRACE") != nullptr; const double t_go = now_ms();
            OTTI_HIP(hipStreamWaitEvent(hc.stream, ev, 0));
            dev_msm_rows(hc, *gens.dev, {.dense = Z, .n_dense = R, .rows = rows});
            const double t_queued = now_ms();
            // (polled, not hipStreamSynchronize: a blocking wait in this thread was seen to hold up the proving thread's launches for as long as it lasted)
            if (!getenv("OTTI_DEREFS_SYNC")) while (hipStreamQuery(hc.stream) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(50));
            hc.sync();
            if (trace) fprintf(stderr, "[otti] rows ahead: %zu rows on %s: queued in %.3f ms, summed %.3f ms after the release\n", rows, ms ? "the CU-masked stream" : "an ordinary second stream (no CU mask)", t_queued - t_go, now_ms() - t_go);
            std::vector<CPoint> out(rows); memcpy(out.data(), hc.h_points, 32 * rows);
            std::lock_guard<std::mutex> lk(mu); C = std::move(out); done = true;
        } catch (...) {
            // whatever was queued on the (shared) masked stream may still be using this context's buffers: drain it before the context goes back to the pool
            if (hipStream_t ms = masked_stream()) (void)hipStreamSynchronize(ms);
            std::lock_guard<std::mutex> lk(mu); err = std::current_exception(); done = true;
        }
        cv.notify_all();
    }
};

// ================================================================================================ SNARK::prove
// work queued on the second stream uses this context's buffers: an exception on the way to the hash layer must not let the context go back to the pool under it
struct SideDrain { DevCtx &c; bool pending = false; ~SideDrain() { if (pending && c.ev_side) (void)hipEventSynchronize(c.ev_side); } };

// One proof in progress: what the stages of SNARK::prove share.  The stages are member functions in proof order (prove() is the sequence).
struct SnarkRun {
    const double t_start = now_ms(); const bool trace = getenv("OTTI_TRACE") != nullptr; double t_lap = now_ms();
    DevCtx &c; Instance &I; DeviceWitness &wit; SnarkGens &g; ShardComm *const sh; SideDrain &side_drain;
    const DeviceDecomm &d; const size_t N, M, H, nm;
    Transcript tr; RandomTape tape; SnarkProof S; EvalProof &E = S.eval; SnarkTimings T{};
    SnarkScratch &W = snark_workspace(c);
    Fr *mem_rx, *mem_ry, *eqs, *derefs, *partials;
    size_t rows_half = 0; std::unique_ptr<RowsAhead> rows_job; bool rows_queued = false;        // the derefs commitment's row half, ahead of time
    std::vector<Fr> dotp_evals = std::vector<Fr>(6), ops_evals = std::vector<Fr>(12), mem_evals = std::vector<Fr>(4), rand_ops, rand_mem;
    int pcG = 1, pcR = 0; ShardComm *pc_sh = nullptr; Circuits ops, mem; DotpTables D;          // the product circuits and how they are split over the ranks
    bool hash_fused = false, hash_ahead = false, hash_evals_queued = false; Fr *chunks_d = nullptr, *chunks_o = nullptr;
    SnarkRun(DevCtx &c_, Instance &I_, CompComm &comm, DeviceWitness &wit_, SnarkGens &g_, const void *tlabel, size_t tlabel_len, const uint8_t *seed32, ShardComm *sh_, SideDrain &sd)
        : c(c_), I(I_), wit(wit_), g(g_), sh(sh_), side_drain(sd), d(*comm.dec), N(d.N), M(d.M), H(N / 2), nm(ilog2(M)), tr(tlabel, tlabel_len), tape(seed32) {
        ensure_gens_device(*g.eval);
        if (wit.z.n != 2 * I.num_vars || wit.inputs.size() != I.num_inputs) throw Error(OTTI_ERR_BAD_ARG, "witness belongs to another instance");
        tr.append_protocol_name("Spartan SNARK proof");
        snark_append_comm(tr, comm);
        mem_rx = W.get(SS_MEM_RX, M); mem_ry = W.get(SS_MEM_RY, M); eqs = W.get(SS_EQS, 5 * 4096); derefs = W.get(SS_DEREFS, (size_t)8 * N); partials = W.get(SS_PARTIALS, kSnarkPartials);
    }
    void lap(const char *what) { if (!trace) return; c.sync(); const double t = now_ms(); fprintf(stderr, "[otti] snark_prove %-34s %.3f ms\n", what, t - t_lap); t_lap = t; }
    Fr *drow(int k) const { return derefs + (size_t)k * N; }
    Fr *dcol(int k) const { return derefs + (size_t)(3 + k) * N; }
    std::vector<Fr> equalized(const std::vector<Fr> &r) const {          // zeros in FRONT of the shorter point
        if (r.size() > nm) throw Error(OTTI_ERR_INTERNAL, "memory size does not match the evaluation point");
        std::vector<Fr> e(nm - r.size(), fr_zero()); e.insert(e.end(), r.begin(), r.end()); return e;
    }
    // ---- 1. the R1CS proof with its hooks
    // dense.deref, row side: row_ops_val[k][i] = eq(rx)[row_addr[k][i]] — queued the moment rx is final (R1csHooks), and with it the row half
    // of the derefs commitment on the helper's stream (RowsAhead above); the column side follows after the R1CS proof
    void queue_rows(const std::vector<Fr> &rx) {
        const std::vector<Fr> rxe = equalized(rx);
        dev_eq_evals(c, rxe.data(), nm, mem_rx, eqs);
        for (int k = 0; k < 3; k++) dev_gather(c, mem_rx, d.row_addr[k].p, drow(k), N);
        if (rows_job) rows_job->record(c.stream);
        rows_queued = true;
    }
    void r1cs_proof() {
        rows_half = g.derefs.R ? 3 * N / g.derefs.R : 0;
        static const bool ahead_env = [] { const char *e = getenv("OTTI_DEREFS_AHEAD"); return !(e && e[0] == '0'); }();
        const bool ahead = !sh && ahead_env && c.armed_ok() && c.num_cu >= 128 && N >= ((size_t)1 << 14) && rows_half >= 64 && rows_half * g.derefs.R == 3 * N && 2 * rows_half <= g.derefs.L;
        if (ahead) rows_job.reset(new RowsAhead(*g.eval, derefs, g.derefs.R, rows_half));
        // the helper starts once the second sum-check is past its bandwidth-bound rounds: those want the whole chip (confined to the CUs the
        // helper leaves free they took 3.2 ms instead of 0.75), the short rounds after them and the evaluation proof do not
        R1csHooks hooks; hooks.on_rx = [this](const std::vector<Fr> &rx) { queue_rows(rx); }; hooks.on_idle = [this] { if (rows_job) rows_job->release(); };
        ProveTimings pt{}; r1cs_prove_device(I, wit, *g.sat, tr, tape, S.r1cs, pt, sh, ahead ? &hooks : nullptr); for (int k = 0; k < 6; k++) T.ms[k] = pt.ms[k];
        lap("r1cs proof");
    }
    // ---- 2. dereference and inst.evaluate
    // inst.evaluate(rx, ry) is not computed by a sparse product of its own: M(rx, ry) = sum_i val_i eq(rx)[row_i] eq(ry)[col_i] is exactly
    // the dot product of the dereferenced vectors the evaluation proof needs anyway (its two halves are E.dotp_left / dotp_right below),
    // so the eq tables, the gathers and one launch of six sums come first and serve both.
    void deref_and_evaluate() {
        const std::vector<Fr> &rx = S.r1cs.rx, &ry = S.r1cs.ry;
        if (((size_t)1 << std::max(rx.size(), ry.size())) != M) throw Error(OTTI_ERR_INTERNAL, "memory size does not match the evaluation point");
        const std::vector<Fr> rye = equalized(ry);
        if (!rows_queued) queue_rows(rx);
        if (rows_job) rows_job->release();
        dev_eq_evals(c, rye.data(), nm, mem_ry, eqs);
        // comb = merge(rows, cols), zero-padded to 8 N
        OTTI_HIP(hipMemsetAsync(derefs + 6 * N, 0, 2 * N * sizeof(Fr), c.stream));
        lap("allocations, eq tables");
        for (int k = 0; k < 3; k++) dev_gather(c, mem_ry, d.col_addr[k].p, dcol(k), N);
        AbcList A; A.n = 6;
        for (int k = 0; k < 3; k++) for (int half = 0; half < 2; half++) { A.A[2 * k + half] = drow(k) + half * H; A.B[2 * k + half] = dcol(k) + half * H; A.C[2 * k + half] = d.part(4, k) + half * H; }
        dev_sum3(c, A, H, partials, kSumSlot + 40);
        c.sync();
        for (int i = 0; i < 6; i++) dotp_evals[i] = c.h_results[kSumSlot + 40 + i];
        for (int k = 0; k < 3; k++) S.inst_evals[k] = fr_add(dotp_evals[2 * k], dotp_evals[2 * k + 1]);
        lap("deref gathers, inst.evaluate");
        tr.append_scalar("Ar_claim", S.inst_evals[0]); tr.append_scalar("Br_claim", S.inst_evals[1]); tr.append_scalar("Cr_claim", S.inst_evals[2]);
        // ---- R1CSEvalProof::prove -> SparseMatPolyEvalProof::prove
        tr.append_protocol_name("Sparse polynomial evaluation proof");
    }
    // ---- 3. the derefs commitment, by one of three routes
    void zero_comm_derefs() { E.comm_derefs.assign(g.derefs.L, CPoint{}); for (auto &z : E.comm_derefs) memset(z.b, 0, 32); }      // the identity compresses to 32 zero bytes
    // the helper's rows ahead: the column half (and nothing for the zero rows) on this stream, beside what is left of the helper's row half
    void derefs_rows_ahead() {
        dev_msm_rows(c, *g.eval->dev, {.dense = derefs + (size_t)3 * N, .n_dense = g.derefs.R, .rows = rows_half});
        c.sync();
        zero_comm_derefs();
        memcpy(E.comm_derefs[rows_half].b, c.h_points, 32 * rows_half);
        const std::vector<CPoint> head = rows_job->take();
        memcpy(E.comm_derefs[0].b, head[0].b, 32 * rows_half);
        rows_job.reset();
    }
    // one proof over several GPUs: the commitment's rows are independent MSMs over the same generators, so every rank sums a block of
    // them and the 32-byte results are gathered (rank order = row order), as the witness commitment of the R1CS proof is.  Only the
    // rows that can be non-zero are dealt out (the polynomial ends in 2 N zeros: their rows are the identity).
    void derefs_rows_over_ranks() {
        const size_t Lr = g.derefs.L, Rr = g.derefs.R, nzr = std::min(Lr, (6 * N + Rr - 1) / Rr), world = (size_t)sh->world();
        const size_t per = (nzr + world - 1) / world, r0 = std::min(nzr, per * (size_t)sh->rank()), mine = std::min(per, nzr - r0);
        if (per * 32 > ShardComm::kSlotBytes) throw Error(OTTI_ERR_BAD_ARG, "derefs commitment: too many rows per rank for the exchange");
        ensure_gens_device(*g.eval);
        std::vector<CPoint> block(per); for (auto &z : block) memset(z.b, 0, 32);
        if (mine) {
            dev_msm_rows(c, *g.eval->dev, {.dense = derefs + r0 * Rr, .n_dense = Rr, .rows = mine});
            c.sync();
            memcpy(block[0].b, c.h_points, 32 * mine);
        }
        std::vector<CPoint> all(per * world);
        sh->allgather(block.data(), per * 32, all.data());
        zero_comm_derefs();
        memcpy(E.comm_derefs[0].b, all[0].b, 32 * nzr);              // rank k's block starts at row k * per: contiguous up to nzr
    }
    void commit_derefs() {
        if (rows_job) derefs_rows_ahead();
        else if (sh && sh->world() > 1) derefs_rows_over_ranks();
        else E.comm_derefs = commit_poly(c, *g.eval, derefs, g.derefs, 0);      // plain.  Values of eq tables: uniform field elements
        tr.append_message("derefs_commitment", "begin_derefs_commitment", 23);
        append_poly_commitment(tr, "comm_poly_row_col_ops_val", E.comm_derefs);
        tr.append_message("derefs_commitment", "end_derefs_commitment", 21);
        lap("derefs commitment");
    }
    // ---- 4. PolyEvalNetwork::new: hash layers -> product circuits.  ops: row reads A,B,C; row writes; col reads; col writes.  mem: row init, row audit, col init, col audit.
    // One proof over several GPUs: the product circuits (hash layer, product layers, the large rounds of the two batched sum-checks — the
    // bandwidth-bound part of this stage) are split by residue classes of the element index; circuits too small for that run on every rank alike.
    void build_circuits() {
        const std::vector<Fr> r_mem_check = tr.challenge_vector("challenge_r_hash", 2);
        pcG = (sh && sh->world() > 1 && sh->world() <= 16 && N >= (size_t)64 * sh->world() && M >= (size_t)64 * sh->world()) ? sh->world() : 1;
        pcR = pcG > 1 ? sh->rank() : 0;
        pc_sh = pcG > 1 ? sh : nullptr;
        ops.init(12, N, W, SS_OPS, pcG, pcR); mem.init(4, M, W, SS_MEMC, pcG, pcR);
        lap("circuit allocations");
        for (int k = 0; k < 3; k++) {
            dev_hash_ops(c, d.part(0, k), drow(k), d.part(1, k), ops.input(k), ops.input(3 + k), N, r_mem_check[0], r_mem_check[1], pcG, pcR);
            dev_hash_ops(c, d.part(2, k), dcol(k), d.part(3, k), ops.input(6 + k), ops.input(9 + k), N, r_mem_check[0], r_mem_check[1], pcG, pcR);
        }
        dev_hash_mem(c, mem_rx, d.comb_mem.p, mem.input(0), mem.input(1), M, r_mem_check[0], r_mem_check[1], pcG, pcR);
        dev_hash_mem(c, mem_ry, d.comb_mem.p + M, mem.input(2), mem.input(3), M, r_mem_check[0], r_mem_check[1], pcG, pcR);
        lap("hash layer kernels");
        ops.build(c); mem.build(c);
        if (pc_sh) { ops.gather_small(c, *pc_sh); mem.gather_small(c, *pc_sh); }
        if (pc_sh && trace) fprintf(stderr, "[otti] snark_prove product circuits split by residue classes over %d ranks (rank %d: %zu of %zu operations, %zu of %zu memory cells)\n", pcG, pcR, ops.n_dev, N, mem.n_dev, M);
        lap("product layers");
    }
    // ---- 5. the dot-product circuits and the circuits' outputs (PolyEvalNetworkProof::prove / ProductLayerProof::prove begin here)
    void circuit_outputs() {
        // the dot-product circuits: halves of (row_ops_val, col_ops_val, val) per matrix — copies, because the sum-check folds them in place
        Fr *const dotp = W.get(SS_DOTP, (size_t)9 * N);
        D.len = H / (size_t)pcG; D.n = 6;
        for (int k = 0; k < 3; k++) {
            Fr *base = dotp + (size_t)3 * k * N;
            const Fr *src[3] = {drow(k), dcol(k), d.part(4, k)};
            for (int t = 0; t < 3; t++) {
                if (pc_sh)                                            // this rank's residue class of every half: element e = element e G + rk of the half
                    for (int half = 0; half < 2; half++) dev_gather_strided(c, src[t] + half * H, (size_t)pcG, (size_t)pcR, base + (size_t)t * N + half * H, D.len);
                else OTTI_HIP(hipMemcpyAsync(base + (size_t)t * N, src[t], N * sizeof(Fr), hipMemcpyDeviceToDevice, c.stream));
            }
            for (int half = 0; half < 2; half++) { D.l[2 * k + half] = base + half * H; D.r[2 * k + half] = base + N + half * H; D.w[2 * k + half] = base + 2 * N + half * H; }
        }
        tr.append_protocol_name("Sparse polynomial evaluation proof");
        tr.append_protocol_name("Sparse polynomial product layer proof");
        if (pc_sh) {   // circuit outputs, sharded: the top layers are on the host (Circuits::small)
            for (int i = 0; i < 12; i++) ops_evals[i] = fr_mul(ops.small[ops.nl - 1][i].first[0], ops.small[ops.nl - 1][i].second[0]);
            for (int i = 0; i < 4; i++) mem_evals[i] = fr_mul(mem.small[mem.nl - 1][i].first[0], mem.small[mem.nl - 1][i].second[0]);
        } else {   // circuit outputs (left * right of the top layer); the dot-product claims were summed above
            PtrList pick; pick.n = 0;
            for (int i = 0; i < 12; i++) { pick.p[pick.n++] = ops.left(i, ops.nl - 1); pick.p[pick.n++] = ops.right(i, ops.nl - 1); }
            for (int i = 0; i < 4; i++) { pick.p[pick.n++] = mem.left(i, mem.nl - 1); pick.p[pick.n++] = mem.right(i, mem.nl - 1); }
            dev_pick0(c, pick, kSumSlot);
            c.sync();
            for (int i = 0; i < 12; i++) ops_evals[i] = fr_mul(c.h_results[kSumSlot + 2 * i], c.h_results[kSumSlot + 2 * i + 1]);
            for (int i = 0; i < 4; i++) mem_evals[i] = fr_mul(c.h_results[kSumSlot + 24 + 2 * i], c.h_results[kSumSlot + 24 + 2 * i + 1]);
        }
        E.eval_row.init = mem_evals[0]; E.eval_row.audit = mem_evals[1]; E.eval_col.init = mem_evals[2]; E.eval_col.audit = mem_evals[3];
        for (int k = 0; k < 3; k++) { E.eval_row.read[k] = ops_evals[k]; E.eval_row.write[k] = ops_evals[3 + k]; E.eval_col.read[k] = ops_evals[6 + k]; E.eval_col.write[k] = ops_evals[9 + k]; }
        append_evals4(tr, E.eval_row, false); append_evals4(tr, E.eval_col, true);
        for (int k = 0; k < 3; k++) {
            E.dotp_left[k] = dotp_evals[2 * k]; E.dotp_right[k] = dotp_evals[2 * k + 1];
            tr.append_scalar("claim_eval_dotp_left", E.dotp_left[k]); tr.append_scalar("claim_eval_dotp_right", E.dotp_right[k]);
            if (!fr_eq(fr_add(E.dotp_left[k], E.dotp_right[k]), S.inst_evals[k])) throw Error(OTTI_ERR_INTERNAL, "sparse polynomial evaluation does not match its dot-product circuits");
        }
    }
    // ---- 6. the two batched proofs; 7. the hash layer's evaluations
    // The hash layer's work that depends on rand_ops alone.  The two evaluation proofs' points are [3 or 4 challenges drawn later | rand_ops] and a
    // committed vector is one CHUNK of rows of its polynomial's matrix, so ONE pass over the 21 vectors gives both the chunk sums of the proofs' bounds
    // (dev_poly_bound_chunks: P_c[j] = sum_i' eq(rand_ops[0 .. rest))[i'] v_c[i' R + j]) and, as dot products of length R with eq(rand_ops[rest ..]),
    // the 21 evaluations v_c(rand_ops) themselves — instead of a pass for the evaluations (with an eq table of N elements) and one per bound (3.1 GB
    // -> 1.6 GB at 2^20: hash layer 3.11 -> 2.9 ms).  OTTI_HASH_FUSED=0: the separate passes as before.  OTTI_HASH_AHEAD=1: that pass queued on a second
    // stream when rand_ops comes out, beside the memory circuits' sum-check (hash layer 2.9 -> 2.6 ms, but those rounds lose 0.1-0.35 ms — more than
    // that inside bench.py's SNARK leg, whatever CU mask the second stream has: profiles/r4_hash_layer_ab.txt; off by default).
    void batched_proofs() {
        static const bool hash_fused_env = [] { const char *e = getenv("OTTI_HASH_FUSED"); return !(e && e[0] == '0'); }();
        static const bool hash_ahead_env = [] { const char *e = getenv("OTTI_HASH_AHEAD"); return e && e[0] == '1'; }();
        const size_t lgN = ilog2(N);
        hash_fused = hash_fused_env && g.derefs.num_vars == lgN + 3 && g.ops.num_vars == lgN + 4 && g.derefs.num_vars / 2 > 3 && g.ops.num_vars / 2 > 4 && g.derefs.L * g.derefs.R == 8 * N && g.ops.L * g.ops.R == 16 * N;
        hash_ahead = hash_fused && hash_ahead_env && !sh && c.side_stream();
        lap("dotp copies, circuit outputs");
        prove_circuits();
    }
    bool queue_hash_evals() {                                   // on c.stream; false (chunks_* null) when the bounds' geometry does not allow the chunked form
        const size_t lgN = ilog2(N), lv_d = g.derefs.num_vars / 2, lv_o = g.ops.num_vars / 2, rest_d = lv_d - 3, rest_o = lv_o - 4;
        Fr *tab_d = W.get(SS_AHEAD + 2, (size_t)1 << rest_d), *tab_o = W.get(SS_AHEAD + 3, (size_t)1 << rest_o), *rv_d = W.get(SS_AHEAD + 4, g.derefs.R), *rv_o = W.get(SS_AHEAD + 5, g.ops.R);
        Fr *bound = W.get(SS_PE0 + 10, 64 * std::max(g.derefs.R, g.ops.R));
        chunks_d = W.get(SS_AHEAD, 8 * g.derefs.R); chunks_o = W.get(SS_AHEAD + 1, 16 * g.ops.R);
        dev_eq_evals2(c, rand_ops.data(), rest_d, tab_d, rand_ops.data(), rest_o, tab_o, eqs);
        if (!dev_poly_bound_chunks(c, derefs, g.derefs.L, g.derefs.R, tab_d, (size_t)1 << rest_d, chunks_d, bound) ||
            !dev_poly_bound_chunks(c, d.comb_ops.p, g.ops.L, g.ops.R, tab_o, (size_t)1 << rest_o, chunks_o, bound)) { chunks_d = chunks_o = nullptr; return false; }
        dev_eq_evals2(c, rand_ops.data() + rest_d, lgN - rest_d, rv_d, rand_ops.data() + rest_o, lgN - rest_o, rv_o, eqs);
        PtrList Ld, Lo; Ld.n = 0; Lo.n = 0;
        for (int k = 0; k < 6; k++) Ld.p[Ld.n++] = chunks_d + (size_t)k * g.derefs.R;            // = drow(0..2), dcol(0..2)
        for (int k = 0; k < 15; k++) Lo.p[Lo.n++] = chunks_o + (size_t)k * g.ops.R;              // = d.part(p, k), p = 0..4
        dev_dot_many(c, rv_d, Ld, g.derefs.R, partials, kHashEvalSlot);
        dev_dot_many(c, rv_o, Lo, g.ops.R, partials, kHashEvalSlot + 6);
        return true;
    }
    void prove_circuits() {
        Fr *const pyr = W.get(SS_PYR, 2 * 8192);
        const bool tail_allowed = !sh;                          // (also where the circuits were too small to be split: see snark_prove_resident)
        E.proof_ops = pcbatch_prove(c, ops, ops_evals, &D, dotp_evals, tr, pyr, rand_ops, tail_allowed, pc_sh);
        lap("batched proof: ops");
        // rand_ops is out.  OTTI_HASH_AHEAD=1: the hash layer's rand_ops-only work to a second stream now (after the memory circuits' first launches)
        const std::function<void()> queue_hash_ahead = [&] {
            hipStream_t own = c.stream;
            struct Restore { DevCtx &c; hipStream_t s; ~Restore() { c.stream = s; } } restore{c, own};
            c.stream = c.side_stream();
            hash_evals_queued = queue_hash_evals();
            OTTI_HIP(hipEventRecord(c.ev_side, c.stream));
            side_drain.pending = true;
        };
        E.proof_mem = pcbatch_prove(c, mem, mem_evals, nullptr, {}, tr, pyr, rand_mem, tail_allowed, pc_sh, hash_ahead ? &queue_hash_ahead : nullptr);
        lap("batched proof: mem");
    }
    // HashLayerProof::prove((rand_mem, rand_ops)): evaluations at rand_ops of the six dereferenced vectors and the fifteen committed ones, at
    // rand_mem of the two audit vectors.  The 21 by one of three routes: fused and ahead on the side stream, fused, separate
    void hash_layer_evals() {
        tr.append_protocol_name("Sparse polynomial hash layer proof");
        Fr *const Em = W.get(SS_EM, M);
        if (hash_ahead) {                                       // queued on the second stream when rand_ops came out
            OTTI_HIP(hipEventSynchronize(c.ev_side));
            OTTI_HIP(hipStreamWaitEvent(c.stream, c.ev_side, 0));
            side_drain.pending = false;
        } else if (hash_fused) hash_evals_queued = queue_hash_evals();
        if (!hash_evals_queued) {                               // separate: an eq table of N elements and a pass of its own
            Fr *const Eo = W.get(SS_EO, N);
            dev_eq_evals(c, rand_ops.data(), rand_ops.size(), Eo, eqs);
            PtrList Lo; Lo.n = 0;
            for (int k = 0; k < 3; k++) Lo.p[Lo.n++] = drow(k);
            for (int k = 0; k < 3; k++) Lo.p[Lo.n++] = dcol(k);
            for (int p = 0; p < 5; p++) for (int k = 0; k < 3; k++) Lo.p[Lo.n++] = d.part(p, k);
            dev_dot_many(c, Eo, Lo, N, partials, kSumSlot + 8);
        }
        const int es = hash_evals_queued ? kHashEvalSlot : kSumSlot + 8;
        dev_eq_evals(c, rand_mem.data(), rand_mem.size(), Em, eqs);
        PtrList Lm; Lm.n = 2; Lm.p[0] = d.comb_mem.p; Lm.p[1] = d.comb_mem.p + M;
        dev_dot_many(c, Em, Lm, M, partials, kSumSlot);
        c.sync();                                               // one synchronise for the 21 + 2 evaluations
        for (int k = 0; k < 3; k++) {
            E.h_deref_row[k] = c.h_results[es + k]; E.h_deref_col[k] = c.h_results[es + 3 + k];
            E.h_row_addr[k] = c.h_results[es + 6 + k]; E.h_row_read_ts[k] = c.h_results[es + 9 + k];
            E.h_col_addr[k] = c.h_results[es + 12 + k]; E.h_col_read_ts[k] = c.h_results[es + 15 + k]; E.h_val[k] = c.h_results[es + 18 + k];
        }
        E.h_row_audit = c.h_results[kSumSlot]; E.h_col_audit = c.h_results[kSumSlot + 1];
        lap("hash layer evaluations");
    }
    // ---- 8. the three evaluation proofs
    Fr joint(std::vector<Fr> ev, const char *label_evals, const char *label_ch, const char *label_joint, const std::vector<Fr> &rand, std::vector<Fr> &r_joint) {
        tr.append_scalars(label_evals, ev.data(), ev.size());
        std::vector<Fr> ch = tr.challenge_vector(label_ch, ilog2(ev.size()));
        const Fr j = reduce_evals(ev, ch);
        r_joint = ch; r_joint.insert(r_joint.end(), rand.begin(), rand.end());
        tr.append_scalar(label_joint, j);
        return j;
    }
    void eval_proofs() {
        std::vector<Fr> ev_d(8, fr_zero()), ev_o(16, fr_zero()), rj;
        for (int k = 0; k < 3; k++) { ev_d[k] = E.h_deref_row[k]; ev_d[3 + k] = E.h_deref_col[k]; }
        for (int k = 0; k < 3; k++) { ev_o[k] = E.h_row_addr[k]; ev_o[3 + k] = E.h_row_read_ts[k]; ev_o[6 + k] = E.h_col_addr[k]; ev_o[9 + k] = E.h_col_read_ts[k]; ev_o[12 + k] = E.h_val[k]; }
        tr.append_protocol_name("Derefs evaluation proof");      // DerefsEvalProof::prove
        Fr j = joint(ev_d, "evals_ops_val", "challenge_combine_n_to_one", "joint_claim_eval", rand_ops, rj);
        E.pe_derefs = polyeval_prove_plain(c, *g.eval, g.derefs, derefs, rj, j, tr, tape, chunks_d, 3);
        lap("polyeval derefs");
        j = joint(ev_o, "claim_evals_ops", "challenge_combine_n_to_one", "joint_claim_eval_ops", rand_ops, rj);
        E.pe_ops = polyeval_prove_plain(c, *g.eval, g.ops, d.comb_ops.p, rj, j, tr, tape, chunks_o, 4);
        lap("polyeval ops");
        j = joint({E.h_row_audit, E.h_col_audit}, "claim_evals_mem", "challenge_combine_two_to_one", "joint_claim_eval_mem", rand_mem, rj);
        E.pe_mem = polyeval_prove_plain(c, *g.eval, g.mem, d.comb_mem.p, rj, j, tr, tape);
        lap("polyeval mem");
    }
    std::vector<uint8_t> prove(SnarkTimings *tm) {
        r1cs_proof();
        double t0 = now_ms();
        deref_and_evaluate(); commit_derefs();
        T.ms[6] = now_ms() - t0; t0 = now_ms();
        build_circuits(); circuit_outputs(); batched_proofs();
        T.ms[7] = now_ms() - t0; t0 = now_ms();
        hash_layer_evals(); eval_proofs();
        T.ms[8] = now_ms() - t0;
        std::vector<uint8_t> out = S.serialize();
        T.ms[9] = now_ms() - t_start;
        OTTI_HIP(hipStreamSynchronize(c.stream));
        KStats::get().flush();
        if (tm) *tm = T;
        return out;
    }
};

std::vector<uint8_t> snark_prove_resident_once(Instance &I, CompComm &comm, DeviceWitness &wit, SnarkGens &g, const void *tlabel, size_t tlabel_len,
                                               const uint8_t *seed32, SnarkTimings *tm, ShardComm *sh) {
    DevCtx &c = DevCtx::get();
    ActiveProof active;
    // first-use HIP objects are made BEFORE the session narrows this thread's affinity to its helpers' L3 group (pool.h hold_caller): a thread
    // the runtime starts while making them would inherit the narrowed mask for good
    if (!sh && c.num_cu >= 128) (void)bulk_masked_stream();
    if (!sh && getenv("OTTI_HASH_AHEAD")) (void)c.side_stream();
    SpinPool::Session pool_session;
    if (!comm.dec) throw Error(OTTI_ERR_BAD_ARG, "this computation commitment carries no decommitment (it was parsed from bytes): SNARK::prove needs the one SNARK::encode returned");
    if (I.num_cons != comm.num_cons || I.num_vars != comm.num_vars || I.num_inputs != comm.num_inputs) throw Error(OTTI_ERR_BAD_ARG, "commitment belongs to another instance");
    SideDrain side_drain{c};
    return SnarkRun(c, I, comm, wit, g, tlabel, tlabel_len, seed32, sh, side_drain).prove(tm);
}
}  // namespace

std::vector<uint8_t> snark_prove_gpu(Instance &I, CompComm &comm, const uint8_t *vars32, size_t nvars, const std::vector<Fr> &inputs, SnarkGens &g,
                                     const void *tlabel, size_t tlabel_len, const uint8_t *seed32, SnarkTimings *tm) {
    if (I.num_cons != comm.num_cons || I.num_vars != comm.num_vars || I.num_inputs != comm.num_inputs) throw Error(OTTI_ERR_BAD_ARG, "commitment belongs to another instance");
    check_comm_generation(I, comm);
    DeviceWitness wit(I, vars32, nvars, inputs);                 // uploaded (and checked for canonical scalars) inside the call
    return snark_prove_resident(I, comm, wit, g, tlabel, tlabel_len, seed32, tm);
}
std::vector<uint8_t> snark_prove_resident(Instance &I, CompComm &comm, DeviceWitness &wit, SnarkGens &g, const void *tlabel, size_t tlabel_len,
                                          const uint8_t *seed32, SnarkTimings *tm, ShardComm *sh) {
    check_comm_generation(I, comm);                           // before any device work
    // (sharded: every rank of a node sees the same device conditions or none does — a rank that alone repeated its proof would leave the
    // others waiting in the exchange — so the persistent tail, which can time out, is not used at all there)
    if (sh) return snark_prove_resident_once(I, comm, wit, g, tlabel, tlabel_len, seed32, tm, sh);
    try { return snark_prove_resident_once(I, comm, wit, g, tlabel, tlabel_len, seed32, tm, nullptr); }
    catch (const TailTimeout &e) {
        // the persistent tail's grid was not resident as a whole (the GPU is shared, partitioned or CU-masked): a proof is a function of its
        // inputs and the tape seed, so proving again — with a launch per round from now on — gives the bytes the first attempt would have given
        if (pc_set_tail_timed_out()) throw;
        fprintf(stderr, "[otti] notice: %s; SNARK::prove repeats the proof with one launch per sum-check round, and this process keeps doing so\n", e.what());
        return snark_prove_resident_once(I, comm, wit, g, tlabel, tlabel_len, seed32, tm, nullptr);
    }
}

}  // namespace otti
