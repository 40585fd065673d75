// SNARK::encode and attach on the MI355X: the dense representation of A, B, C (addresses, timestamps, values: 16 N + 2 M field elements)
// built in HBM and committed with the bulk MSM.  Follows upstream libspartan src/r1csinstance.rs, src/sparse_mlpoly.rs; see snark.h.
#include "snark_prover.h"
#include "value_rows.h"
#include <thread>

namespace otti {

namespace {
// upstream pads 0 / 1 constraints with explicit zero entries (row i, column num_vars): the length of matrix k's entry list with them
size_t padded_len(const Instance &I, int k) { return (I.given_cons < 2 && I.num_cons > I.nnz[k]) ? I.num_cons : I.nnz[k]; }
// sizes of the dense representation of I: N operations per matrix, M memory cells
void decomm_dims(const Instance &I, size_t &N, size_t &M) {
    size_t nz = 0; for (int k = 0; k < 3; k++) nz = std::max(nz, padded_len(I, k));
    N = next_pow2(std::max<size_t>(nz, 2)); M = (size_t)1 << std::max(ilog2(I.num_cons), ilog2(2 * I.num_vars));
}
void check_gens_fit(const Instance &I, const SnarkGens &g, size_t N, size_t M) {
    if (I.num_cons != g.num_cons || I.num_vars != g.num_vars) throw Error(OTTI_ERR_BAD_ARG, "SNARK generators were made for a different instance size");
    if (ilog2(16 * N) != g.ops.num_vars || ilog2(2 * M) != g.mem.num_vars) throw Error(OTTI_ERR_BAD_ARG, "SNARK generators were made for a different number of non-zero entries");
}
bool same_points(const std::vector<CPoint> &a, const std::vector<CPoint> &b) { return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), 32 * a.size())); }
struct EncodeLaps {
    DevCtx &c; const bool on = getenv("OTTI_TRACE") != nullptr; double t_lap = now_ms();
    explicit EncodeLaps(DevCtx &c_) : c(c_) {}
    void operator()(const char *what) { if (!on) return; c.sync(); const double t = now_ms(); fprintf(stderr, "[otti] snark_encode %-34s %.3f ms\n", what, t - t_lap); t_lap = t; }
};
// OTTI_DECOMM_HOST=1 (A/B): the address / timestamp scans as sequential host loops over u32 lists, their results uploaded list by list
void decomm_fill_host(DevCtx &c, const Instance &I, DeviceDecomm *dec, EncodeLaps &lap) {
    const size_t N = dec->N, M = dec->M;
    std::vector<uint32_t> addr[2][3], read_ts[2][3], audit[2];
    for (int k = 0; k < 3; k++) {
        const SparseMat &m = I.mat(k);
        addr[0][k].assign(N, 0); addr[1][k].assign(N, 0);
        for (size_t i = 0; i < m.val.size(); i++) { addr[0][k][i] = m.row[i]; addr[1][k][i] = m.col[i]; }
        for (size_t i = m.val.size(); i < padded_len(I, k); i++) { addr[0][k][i] = (uint32_t)i; addr[1][k][i] = (uint32_t)I.num_vars; }
    }
    auto scan_side = [&](int side) {                          // AddrTimestamps::new: audit_ts is shared by the three matrices
        audit[side].assign(M, 0);
        for (int k = 0; k < 3; k++) {
            read_ts[side][k].resize(N);
            for (size_t i = 0; i < N; i++) read_ts[side][k][i] = audit[side][addr[side][k][i]]++;
        }
    };
    { std::thread other(scan_side, 1); scan_side(0); other.join(); }
    lap("address / timestamp scans (host)");
    DevBuf<uint32_t> tmp(std::max(N, M));
    OTTI_HIP(hipMemsetAsync(dec->comb_ops.p + 12 * N, 0, 4 * N * sizeof(Fr), c.stream));      // values (zero-padded) and the unused sixteenth part
    for (int k = 0; k < 3; k++) {
        OTTI_HIP(hipMemcpyAsync(dec->row_addr[k].p, addr[0][k].data(), N * 4, hipMemcpyHostToDevice, c.stream));
        OTTI_HIP(hipMemcpyAsync(dec->col_addr[k].p, addr[1][k].data(), N * 4, hipMemcpyHostToDevice, c.stream));
        dev_u32_to_fr(c, dec->row_addr[k].p, dec->part(0, k), N); dev_u32_to_fr(c, dec->col_addr[k].p, dec->part(2, k), N);
        for (int side = 0; side < 2; side++) {
            OTTI_HIP(hipMemcpyAsync(tmp.p, read_ts[side][k].data(), N * 4, hipMemcpyHostToDevice, c.stream));
            dev_u32_to_fr(c, tmp.p, dec->part(2 * side + 1, k), N);
            OTTI_HIP(hipStreamSynchronize(c.stream));     // tmp is reused (the copies come from pageable memory: nothing to overlap with)
        }
        if (!I.mat(k).val.empty()) OTTI_HIP(hipMemcpyAsync(dec->part(4, k), I.mat(k).val.data(), I.mat(k).val.size() * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
    }
    for (int side = 0; side < 2; side++) {
        OTTI_HIP(hipMemcpyAsync(tmp.p, audit[side].data(), M * 4, hipMemcpyHostToDevice, c.stream));
        dev_u32_to_fr(c, tmp.p, dec->comb_mem.p + (size_t)side * M, M);
        OTTI_HIP(hipStreamSynchronize(c.stream));
    }
    lap("uploads + expansion to field elements");
}
// what both device fills end with: the timestamps by dev_addr_timestamps straight into comb_ops / comb_mem (timed by events when traced)
void decomm_finish_device(DevCtx &c, DeviceDecomm *dec, AddrTs &a, EncodeLaps &lap) {
    for (int side = 0; side < 2; side++) a.audit_fr[side] = dec->comb_mem.p + (size_t)side * dec->M;
    lap("entry lists: upload + expansion");
    if (lap.on) OTTI_HIP(hipEventRecord(c.ev0, c.stream));
    dev_addr_timestamps(c, a);                                // returns with the stream idle: the caller's staging lists may go
    if (lap.on) {
        float ms = 0; OTTI_HIP(hipEventRecord(c.ev1, c.stream)); OTTI_HIP(hipEventSynchronize(c.ev1)); OTTI_HIP(hipEventElapsedTime(&ms, c.ev0, c.ev1));
        fprintf(stderr, "[otti] snark_encode %-34s %.3f ms\n", "dev_addr_timestamps (events)", (double)ms);
    }
    lap("address / timestamp sort (device)");
}
// the device path: the instance's entry lists go up once (u32 addresses, values), everything else is made in HBM
void decomm_fill_device(DevCtx &c, const Instance &I, DeviceDecomm *dec, EncodeLaps &lap) {
    const size_t N = dec->N;
    AddrTs a; a.sides = 2; a.N = N; a.M = dec->M;
    std::vector<uint32_t> extra[2][3];                        // the padding entries
    OTTI_HIP(hipMemsetAsync(dec->comb_ops.p + 12 * N, 0, 4 * N * sizeof(Fr), c.stream));      // values (zero-padded) and the unused sixteenth part
    for (int k = 0; k < 3; k++) {
        const SparseMat &m = I.mat(k); const size_t nv = m.val.size(), len = padded_len(I, k);
        for (size_t i = nv; i < len; i++) { extra[0][k].push_back((uint32_t)i); extra[1][k].push_back((uint32_t)I.num_vars); }
        a.len[k] = (uint32_t)len;
        uint32_t *dst[2] = {dec->row_addr[k].p, dec->col_addr[k].p}; const uint32_t *src[2] = {m.row.data(), m.col.data()};
        for (int side = 0; side < 2; side++) {
            if (len < N) OTTI_HIP(hipMemsetAsync(dst[side] + len, 0, (N - len) * 4, c.stream));
            if (nv) OTTI_HIP(hipMemcpyAsync(dst[side], src[side], nv * 4, hipMemcpyHostToDevice, c.stream));
            if (len > nv) OTTI_HIP(hipMemcpyAsync(dst[side] + nv, extra[side][k].data(), (len - nv) * 4, hipMemcpyHostToDevice, c.stream));
            dev_u32_to_fr(c, dst[side], dec->part(2 * side, k), N);
            a.addr[side][k] = dst[side]; a.ts_fr[side][k] = dec->part(2 * side + 1, k);
        }
        if (nv) OTTI_HIP(hipMemcpyAsync(dec->part(4, k), m.val.data(), nv * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
    }
    decomm_finish_device(c, dec, a, lap);
}
// the same from the entry lists a device ingest keeps in HBM (DeviceInstance::ent): one launch writes addresses, their field elements and the
// values of all three matrices, padding included — nothing crosses PCIe and Instance::mat() is never asked
bool decomm_entries_resident(const Instance &I) {
    // (only a device ingest keeps lists, and its `dev` is set before the instance is shared: no other instance's `dev`, which a prover
    // thread may be setting right now, is looked at)
    if (!I.ingested_on_device || !I.dev || I.nnz[0] + I.nnz[1] + I.nnz[2] == 0) return false;
    for (int k = 0; k < 3; k++) if (I.dev->ent[k].n != I.nnz[k]) return false;
    return true;
}
void decomm_fill_from_entries(DevCtx &c, const Instance &I, DeviceDecomm *dec, EncodeLaps &lap) {
    const size_t N = dec->N;
    const std::shared_ptr<DeviceInstance> d = I.dev;          // (kept alive across the launches)
    AddrTs a; a.sides = 2; a.N = N; a.M = dec->M;
    DecommFill f{};
    OTTI_HIP(hipMemsetAsync(dec->comb_ops.p + 15 * N, 0, N * sizeof(Fr), c.stream));          // the unused sixteenth part
    for (int k = 0; k < 3; k++) {
        const size_t len = padded_len(I, k);
        a.len[k] = (uint32_t)len;
        f.m[k] = DecommFillMat{d->ent[k].row.p, d->ent[k].col.p, d->ent[k].val.p, dec->row_addr[k].p, dec->col_addr[k].p, dec->part(0, k), dec->part(2, k),
                               dec->part(4, k), I.nnz[k], len, (uint32_t)I.num_vars};
        a.addr[0][k] = dec->row_addr[k].p; a.addr[1][k] = dec->col_addr[k].p;
        for (int side = 0; side < 2; side++) a.ts_fr[side][k] = dec->part(2 * side + 1, k);
    }
    dev_decomm_fill(c, f, 3, N);
    decomm_finish_device(c, dec, a, lap);
}
// MultiSparseMatPolynomialAsDense in HBM: what SNARK::encode keeps as the decommitment and what attach rebuilds
std::shared_ptr<DeviceDecomm> build_decomm(DevCtx &c, const Instance &I, size_t N, size_t M, EncodeLaps &lap) {
    auto dec = std::make_shared<DeviceDecomm>(); dec->N = N; dec->M = M;
    dec->comb_ops.alloc(16 * N); dec->comb_mem.alloc(2 * M);
    for (int k = 0; k < 3; k++) { dec->row_addr[k].alloc(N); dec->col_addr[k].alloc(N); }
    static const bool host_scans = [] { const char *e = getenv("OTTI_DECOMM_HOST"); return e && e[0] == '1'; }();
    if (host_scans) decomm_fill_host(c, I, dec.get(), lap);
    else if (decomm_entries_resident(I)) decomm_fill_from_entries(c, I, dec.get(), lap);
    else decomm_fill_device(c, I, dec.get(), lap);
    return dec;
}
}  // namespace

std::unique_ptr<CompComm> snark_encode_gpu(Instance &I, SnarkGens &g) {
    DevCtx &c = DevCtx::get();
    size_t N, M; decomm_dims(I, N, M); check_gens_fit(I, g, N, M);
    EncodeLaps lap(c);
    auto dec = build_decomm(c, I, N, M, lap);
    auto cc = std::make_unique<CompComm>();
    cc->num_cons = I.num_cons; cc->num_vars = I.num_vars; cc->num_inputs = I.num_inputs; cc->num_ops = N; cc->num_mem_cells = M;
    cc->comm_ops = commit_poly(c, *g.eval, dec->comb_ops.p, g.ops);          // SparseMatPolynomial::multi_commit: comb_ops.commit(gens_ops, None), comb_mem.commit(gens_mem, None)
    lap("commit comb_ops (+ window table)");
    cc->comm_mem = commit_poly(c, *g.eval, dec->comb_mem.p, g.mem);
    lap("commit comb_mem");
    cc->dec = dec; cc->dec_gen = I.value_gen;
    return cc;
}

void snark_attach_gpu(Instance &I, CompComm &cc, SnarkGens &g, bool verify) {
    size_t N, M; decomm_dims(I, N, M);
    if (I.num_cons != cc.num_cons || I.num_vars != cc.num_vars || I.num_inputs != cc.num_inputs || N != cc.num_ops || M != cc.num_mem_cells)
        throw Error(OTTI_ERR_BAD_ARG, "the computation commitment was made for an instance of other dimensions");
    check_gens_fit(I, g, N, M);
    if (cc.dec) return;
    DevCtx &c = DevCtx::get();
    EncodeLaps lap(c);
    auto dec = build_decomm(c, I, N, M, lap);
    if (verify) {
        if (!same_points(commit_poly(c, *g.eval, dec->comb_ops.p, g.ops), cc.comm_ops)) throw Error(OTTI_ERR_BAD_ARG, "attach: comm_ops recomputed from this instance differs from the stored commitment");
        lap("verify comm_ops (+ window table)");
        if (!same_points(commit_poly(c, *g.eval, dec->comb_mem.p, g.mem), cc.comm_mem)) throw Error(OTTI_ERR_BAD_ARG, "attach: comm_mem recomputed from this instance differs from the stored commitment");
        lap("verify comm_mem");
    }
    cc.dec = dec; cc.dec_gen = I.value_gen;
}

void snark_revalue_gpu(Instance &I, CompComm &cc, SnarkGens &g) {
    size_t N, M; decomm_dims(I, N, M);
    if (!cc.dec) throw Error(OTTI_ERR_BAD_ARG, "revalue: this computation commitment carries no decommitment (encode it, or attach the instance first)");
    if (I.num_cons != cc.num_cons || I.num_vars != cc.num_vars || I.num_inputs != cc.num_inputs || N != cc.num_ops || M != cc.num_mem_cells || cc.dec->N != N || cc.dec->M != M)
        throw Error(OTTI_ERR_BAD_ARG, "the computation commitment was made for an instance of other dimensions");
    check_gens_fit(I, g, N, M);
    if (cc.comm_ops.size() != g.ops.L) throw Error(OTTI_ERR_BAD_ARG, "the computation commitment was made for other generators");
    DevCtx &c = DevCtx::get();
    EncodeLaps lap(c);
    DeviceDecomm &dec = *cc.dec;
    // ---- the values alone: entries [0, nnz) of part(4, k); what lies behind them is upstream's zero padding and stays
    const bool resident = decomm_entries_resident(I);
    const std::shared_ptr<DeviceInstance> d = resident ? I.dev : nullptr;
    for (int k = 0; k < 3; k++) {
        if (!I.nnz[k]) continue;
        if (resident) OTTI_HIP(hipMemcpyAsync(dec.part(4, k), d->ent[k].val.p, I.nnz[k] * sizeof(Fr), hipMemcpyDeviceToDevice, c.stream));
        else OTTI_HIP(hipMemcpyAsync(dec.part(4, k), I.mat(k).val.data(), I.nnz[k] * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
    }
    lap("revalue: values into comb_ops");
    // ---- the rows of comm_ops that meet them, as one block of independent row sums
    const ValueRows vr = comm_value_rows(N, g.ops.L, g.ops.R);
    const size_t rows = vr.r1 - vr.r0;
    ensure_gens_device(*g.eval);
    const Fr *Z = dec.comb_ops.p + vr.r0 * g.ops.R;
    const bool sparse = dev_small_fraction(c, Z, rows * g.ops.R) > kSparseWitness;
    dev_msm_rows(c, *g.eval->dev, {.dense = Z, .n_dense = g.ops.R, .rows = rows, .sparse = sparse});
    c.sync();
    memcpy(cc.comm_ops[vr.r0].b, c.h_points, 32 * rows);
    lap("revalue: value rows of comm_ops");
    { std::lock_guard<std::mutex> lk(cc.row_cache_mu); cc.row_cache.reset(); }
    cc.dec_gen = I.value_gen;
}

}  // namespace otti
