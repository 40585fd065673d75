// Kernel-level and device-pointer entries of libottispartan (otti_k_*, otti_kd_*, otti_dev_*, otti_bench_*, otti_stats_*, otti_lanes_*): what the tests and
// the measurement tools call, one launch function at a time.  The ABI that embedders call is in capi.cpp.
#include "capi_common.h"

namespace {
struct Staged {                      // host Montgomery bytes -> device buffer
    DevBuf<Fr> d;
    Staged(DevCtx &c, const uint8_t *h, size_t n) : d(std::max<size_t>(1, n)) { if (n) OTTI_HIP(hipMemcpyAsync(d.p, h, n * sizeof(Fr), hipMemcpyHostToDevice, c.stream)); }
};
void download(DevCtx &c, uint8_t *h, const Fr *d, size_t n) { if (n) OTTI_HIP(hipMemcpyAsync(h, d, n * sizeof(Fr), hipMemcpyDeviceToHost, c.stream)); }
struct KTimer {
    DevCtx &c; float *out;
    KTimer(DevCtx &c_, float *o) : c(c_), out(o) { if (out) OTTI_HIP(hipEventRecord(c.ev0, c.stream)); }
    void stop() { if (out) { OTTI_HIP(hipEventRecord(c.ev1, c.stream)); OTTI_HIP(hipEventSynchronize(c.ev1)); OTTI_HIP(hipEventElapsedTime(out, c.ev0, c.ev1)); } }
};
// the two eq pyramids over m variables exactly as nizk_prove_resident lays them out (lo: last min(m,12) variables, hi: the ones before)
struct EqPyramids {
    DevBuf<Fr> buf; size_t n_lo = 0, n_hi = 0;
    EqPyramids(DevCtx &c, const Fr *tau, size_t m) : buf(8192 + 16384) {
        n_lo = std::min<size_t>(m, 12); n_hi = m - n_lo;
        dev_eq_pyramid2(c, tau + n_hi, n_lo, buf.p, tau, n_hi, n_hi ? buf.p + 8192 : nullptr);
    }
    EqSrc top() const {                                      // E over all m variables
        EqSrc e; const size_t m = n_lo + n_hi;
        if (m <= n_lo) { e.hi = nullptr; e.lo = buf.p + (((size_t)1 << m) - 1); e.lo_bits = 0; }
        else { e.hi = buf.p + 8192 + (((size_t)1 << n_hi) - 1); e.lo = buf.p + (((size_t)1 << n_lo) - 1); e.lo_bits = (int)n_lo; }
        return e;
    }
};
std::vector<Fr> fr_load_vec(const uint8_t *p, size_t n) { std::vector<Fr> v(n + 1); for (size_t i = 0; i < n; i++) v[i] = fr_load(p + 32 * i); return v; }
// Run the library's launch functions on a caller's stream for the duration of one call.  The launches share the context's scratch
// (round partials, arrival counters, MSM partials, result slots), so work enqueued on one stream must not overlap work on another:
// entering, the caller's stream waits for everything the context's own stream has been given; leaving, the context's own stream
// waits for what was just enqueued — two calls on different caller streams are thereby ordered through the context's stream.
struct StreamScope {
    DevCtx &c; hipStream_t old;
    void order(hipStream_t after, hipStream_t before) {
        if (!c.ev_order) OTTI_HIP(hipEventCreateWithFlags(&c.ev_order, hipEventDisableTiming));
        OTTI_HIP(hipEventRecord(c.ev_order, before)); OTTI_HIP(hipStreamWaitEvent(after, c.ev_order, 0));
    }
    StreamScope(DevCtx &c_, void *s) : c(c_), old(c_.stream) { if (s && (hipStream_t)s != old) { order((hipStream_t)s, old); c.stream = (hipStream_t)s; } }
    ~StreamScope() { if (c.stream != old) { hipStream_t mine = c.stream; c.stream = old; try { order(old, mine); } catch (...) {} } }
};
bool pow2(size_t x) { return x && !(x & (x - 1)); }
struct StagedPc {
    std::unique_ptr<Staged> a, b, cc; PcList L; size_t nC = 0;
    StagedPc(DevCtx &c, const uint8_t *A, const uint8_t *B, const uint8_t *C, const uint8_t *has_C, size_t ninst, size_t len) {
        for (size_t y = 0; y < ninst; y++) nC += has_C[y] ? 1 : 0;
        a = std::make_unique<Staged>(c, A, ninst * len); b = std::make_unique<Staged>(c, B, ninst * len); cc = std::make_unique<Staged>(c, C, nC * len);
        L.n = (int)ninst; size_t k = 0;
        for (size_t y = 0; y < ninst; y++) { L.A[y] = a->d.p + y * len; L.B[y] = b->d.p + y * len; L.C[y] = has_C[y] ? cc->d.p + (k++) * len : nullptr; }
    }
};
void check_pc_list(const uint8_t *A, const uint8_t *B, const uint8_t *C, const uint8_t *has_C, size_t ninst, size_t len) {
    if (ninst < 1 || ninst > (size_t)kMaxInst) throw Error(OTTI_ERR_BAD_ARG, "a batch has 1 .. kMaxInst instances");
    if (!A || !B || !has_C) throw Error(OTTI_ERR_BAD_ARG, "null argument");
    if (!pow2(len)) throw Error(OTTI_ERR_BAD_ARG, "table length must be a power of two");
    for (size_t y = 0; y < ninst; y++) if (has_C[y] && !C) throw Error(OTTI_ERR_BAD_ARG, "an instance with a third table, but no third tables");
}
}  // namespace

extern "C" {

int32_t otti_k_fr_op(int32_t op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Staged A(c, a, n), B(c, b, n); DevBuf<Fr> O(std::max<size_t>(1, n));
        KTimer t(c, ms); dev_fr_op(c, op, A.d.p, B.d.p, O.p, n); t.stop();
        download(c, out, O.p, n); c.sync(); return OTTI_OK;
    });
}
// GF(2^255-19) in the device's three forms and the point formulas built on them (k_curve_ops.hip), on a caller's operands
int32_t otti_k_fp_op(int32_t form, int32_t op, const uint8_t *a, const uint8_t *b, const uint8_t *cc, const uint8_t *d, size_t n, uint8_t *out, uint32_t *limbs, float *ms) {
    return guarded([&] {
        if (form < FPFORM_FP8 || form > FPFORM_F10 || op < 0 || op >= FPOP_COUNT) throw Error(OTTI_ERR_BAD_ARG, "unknown form or operation");
        if (form == FPFORM_F9 && (op == FPOP_SQR || op == FPOP_POW22523 || op == FPOP_MUL_F_E)) throw Error(OTTI_ERR_BAD_ARG, "the nine-limb form has no such operation (no square, no power; 2a - b is normalised before it is multiplied)");
        if (n && (!a || !b || !cc || !d || !out || !limbs)) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (!n) return OTTI_OK;
        DevCtx &c = DevCtx::get();
        DevBuf<Fp> in(4 * n), o(n); DevBuf<uint32_t> lm(n * kFpOpLimbStride);
        const uint8_t *src[4] = {a, b, cc, d};
        for (int k = 0; k < 4; k++) OTTI_HIP(hipMemcpyAsync(in.p + k * n, src[k], n * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
        OTTI_HIP(hipMemsetAsync(lm.p, 0, n * kFpOpLimbStride * sizeof(uint32_t), c.stream));
        KTimer t(c, ms); dev_fp_op(c, form, op, in.p, in.p + n, in.p + 2 * n, in.p + 3 * n, o.p, lm.p, n); t.stop();
        OTTI_HIP(hipMemcpyAsync(out, o.p, n * sizeof(Fp), hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipMemcpyAsync(limbs, lm.p, n * kFpOpLimbStride * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
        c.sync(); return OTTI_OK;
    });
}
// GF(l) in nine limbs (fr9.h, fold9) on a caller's operands: words or raw limbs in, as the operation demands (device.h Fr9Op)
int32_t otti_k_fr9_op(int32_t op, const void *a, const void *b, const void *cc, size_t n, uint8_t *out, uint32_t *limbs, float *ms) {
    return guarded([&] {
        if (op < 0 || op >= FR9OP_COUNT) throw Error(OTTI_ERR_BAD_ARG, "unknown operation");
        if (n && (!a || !b || !cc || !out || !limbs)) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (n > ((size_t)1 << 24)) throw Error(OTTI_ERR_BAD_ARG, "more than 2^24 cases");
        if (!n) return OTTI_OK;
        DevCtx &c = DevCtx::get();
        const int nw = fr9_op_words_in(op), nl = fr9_op_limbs_in(op);
        const size_t lbytes = n * kFr9OpLimbs * sizeof(uint32_t);
        DevBuf<Fr> w(3 * n), o(n); DevBuf<uint32_t> l(2 * n * kFr9OpLimbs), lm(n * kFr9OpLimbs);
        const void *src[3] = {a, b, cc};
        for (int k = 0; k < nw; k++) OTTI_HIP(hipMemcpyAsync(w.p + k * n, src[k], n * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
        for (int k = 0; k < nl; k++) OTTI_HIP(hipMemcpyAsync(l.p + k * n * kFr9OpLimbs, src[k], lbytes, hipMemcpyHostToDevice, c.stream));
        OTTI_HIP(hipMemsetAsync(o.p, 0, n * sizeof(Fr), c.stream));
        OTTI_HIP(hipMemsetAsync(lm.p, 0, lbytes, c.stream));
        KTimer t(c, ms); dev_fr9_op(c, op, w.p, w.p + n, w.p + 2 * n, l.p, l.p + n * kFr9OpLimbs, o.p, lm.p, n); t.stop();
        OTTI_HIP(hipMemcpyAsync(out, o.p, n * sizeof(Fr), hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipMemcpyAsync(limbs, lm.p, lbytes, hipMemcpyDeviceToHost, c.stream));
        c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_pt_op(int32_t op, const uint8_t *P, const uint8_t *Q, int32_t neg, uint32_t k, size_t n, uint8_t *out, uint32_t *limbs, uint32_t *bad, float *ms) {
    return guarded([&] {
        if (op < 0 || op >= PTOP_COUNT) throw Error(OTTI_ERR_BAD_ARG, "unknown operation");
        if (n && (!P || !out)) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (n > ((size_t)1 << 20) || k > 4096) throw Error(OTTI_ERR_BAD_ARG, "more than 2^20 cases, or a chain of more than 4096 additions");
        if (bad) *bad = 0;
        if (!n) return OTTI_OK;
        DevCtx &c = DevCtx::get();
        if (op == PTOP_DECODE) {                                   // P: n encodings; out: n Niels entries
            if (!bad) throw Error(OTTI_ERR_BAD_ARG, "null argument");
            DevBuf<uint8_t> in(32 * n); DevBuf<Niels> o(n); DevBuf<unsigned> cnt(1);
            OTTI_HIP(hipMemcpyAsync(in.p, P, 32 * n, hipMemcpyHostToDevice, c.stream));
            OTTI_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned), c.stream));
            KTimer t(c, ms); dev_decode_niels(c, in.p, n, o.p, cnt.p); t.stop();
            OTTI_HIP(hipMemcpyAsync(out, o.p, n * sizeof(Niels), hipMemcpyDeviceToHost, c.stream));
            OTTI_HIP(hipMemcpyAsync(bad, cnt.p, sizeof(unsigned), hipMemcpyDeviceToHost, c.stream));
            c.sync(); return OTTI_OK;
        }
        DevBuf<Pt> p(n);
        OTTI_HIP(hipMemcpyAsync(p.p, P, n * sizeof(Pt), hipMemcpyHostToDevice, c.stream));
        if (op == PTOP_ENCODE) {                                   // Q: n addends, or NULL; out: n encodings
            DevBuf<Pt> q(n); DevBuf<uint8_t> o(32 * n);
            if (Q) OTTI_HIP(hipMemcpyAsync(q.p, Q, n * sizeof(Pt), hipMemcpyHostToDevice, c.stream));
            KTimer t(c, ms); dev_encode_points(c, p.p, n, o.p, Q ? q.p : nullptr); t.stop();
            OTTI_HIP(hipMemcpyAsync(out, o.p, 32 * n, hipMemcpyDeviceToHost, c.stream));
            c.sync(); return OTTI_OK;
        }
        if (!Q || !limbs) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        const bool q_is_point = op == PTOP_P10_ADD || op == PTOP_Q10_ADD;
        const size_t qbytes = n * (q_is_point ? sizeof(Pt) : sizeof(Niels)), nl = n * 4 * kFpOpLimbStride;
        DevBuf<uint8_t> q(qbytes); DevBuf<Pt> o(n); DevBuf<uint32_t> lm(nl);
        OTTI_HIP(hipMemcpyAsync(q.p, Q, qbytes, hipMemcpyHostToDevice, c.stream));
        OTTI_HIP(hipMemsetAsync(lm.p, 0, nl * sizeof(uint32_t), c.stream));
        KTimer t(c, ms); dev_pt_op(c, op, p.p, q.p, neg != 0, k, n, o.p, lm.p); t.stop();
        OTTI_HIP(hipMemcpyAsync(out, o.p, n * sizeof(Pt), hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipMemcpyAsync(limbs, lm.p, nl * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
        c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_addr_timestamps(const uint32_t *h_addr3, size_t N, size_t M, uint32_t *h_read_ts3, uint32_t *h_audit, float *ms) {
    return guarded([&] {
        if (!h_addr3 || !h_read_ts3 || !h_audit || N < 1 || M < 1 || N > ((size_t)1 << 28) || M > ((size_t)1 << 31)) throw Error(OTTI_ERR_BAD_ARG, "address timestamps: null argument, or N outside 1 .. 2^28, or M outside 1 .. 2^31");
        AddrTs a; a.sides = 1; a.N = N; a.M = M;
        for (size_t i = 0; i < 3 * N; i++) if (h_addr3[i] >= M) throw Error(OTTI_ERR_BAD_ARG, "address timestamps: an address is not below M");
        for (int k = 0; k < 3; k++) { size_t len = N; while (len && h_addr3[k * N + len - 1] == 0) len--; a.len[k] = (uint32_t)len; }   // the closed-form tail: trailing entries at address 0
        DevCtx &c = DevCtx::get();
        DevBuf<uint32_t> addr(3 * N), ts(3 * N), audit(M);
        OTTI_HIP(hipMemcpyAsync(addr.p, h_addr3, 3 * N * 4, hipMemcpyHostToDevice, c.stream));
        for (int k = 0; k < 3; k++) { a.addr[0][k] = addr.p + k * N; a.ts_u32[0][k] = ts.p + k * N; }
        a.audit_u32[0] = audit.p;
        KTimer t(c, ms); dev_addr_timestamps(c, a); t.stop();
        OTTI_HIP(hipMemcpyAsync(h_read_ts3, ts.p, 3 * N * 4, hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipMemcpyAsync(h_audit, audit.p, M * 4, hipMemcpyDeviceToHost, c.stream));
        c.sync(); return OTTI_OK;
    });
}
// the decommitment fill from entry lists (snark_encode.cpp decomm_fill_from_entries) on one matrix of a caller's host lists
int32_t otti_k_decomm_entries(const uint32_t *h_row, const uint32_t *h_col, const uint8_t *h_val_mont32, size_t n, size_t N, size_t pad_to, uint32_t pad_col,
                              uint32_t *out_row_u32, uint32_t *out_col_u32, uint8_t *out_row_fr, uint8_t *out_col_fr, uint8_t *out_val_fr, float *ms) {
    return guarded([&] {
        if ((n && (!h_row || !h_col || !h_val_mont32)) || !out_row_u32 || !out_col_u32 || !out_row_fr || !out_col_fr || !out_val_fr) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (N < 1 || N > ((size_t)1 << 28) || n > N || pad_to > N) throw Error(OTTI_ERR_BAD_ARG, "decommitment fill: N outside 1 .. 2^28, or n or pad_to above N");
        const size_t len = std::max(n, pad_to);
        DevCtx &c = DevCtx::get();
        DevBuf<uint32_t> row(std::max<size_t>(1, n)), col(std::max<size_t>(1, n)), ra(N), ca(N); Staged val(c, h_val_mont32, n); DevBuf<Fr> fr(3 * N);
        if (n) { OTTI_HIP(hipMemcpyAsync(row.p, h_row, n * 4, hipMemcpyHostToDevice, c.stream)); OTTI_HIP(hipMemcpyAsync(col.p, h_col, n * 4, hipMemcpyHostToDevice, c.stream)); }
        DecommFill f{}; f.m[0] = DecommFillMat{row.p, col.p, val.d.p, ra.p, ca.p, fr.p, fr.p + N, fr.p + 2 * N, n, len, pad_col};
        KTimer t(c, ms); dev_decomm_fill(c, f, 1, N); t.stop();
        OTTI_HIP(hipMemcpyAsync(out_row_u32, ra.p, N * 4, hipMemcpyDeviceToHost, c.stream)); OTTI_HIP(hipMemcpyAsync(out_col_u32, ca.p, N * 4, hipMemcpyDeviceToHost, c.stream));
        download(c, out_row_fr, fr.p, N); download(c, out_col_fr, fr.p + N, N); download(c, out_val_fr, fr.p + 2 * N, N);
        c.sync(); return OTTI_OK;
    });
}
// a rank's share of an entry list (k_sparse.hip dev_shard_filter, what upload_instance_shard runs on a device-ingested instance) on a caller's host lists
int32_t otti_k_shard_filter(const uint32_t *h_row, const uint32_t *h_col, const uint8_t *h_val_mont32, size_t n, uint32_t world, uint32_t rank, int32_t by_col,
                            uint32_t *out_row, uint32_t *out_col, uint8_t *out_val, size_t *out_n, float *ms) {
    return guarded([&] {
        if (!out_n || (n && (!h_row || !h_col || !h_val_mont32 || !out_row || !out_col || !out_val))) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (world < 1 || (world & (world - 1)) || world > (1u << 30) || rank >= world || n >= ((size_t)1 << 32)) throw Error(OTTI_ERR_BAD_ARG, "shard filter: world must be a power of two above the rank, the list below 2^32 entries");
        DevCtx &c = DevCtx::get();
        DevBuf<uint32_t> row(std::max<size_t>(1, n)), col(std::max<size_t>(1, n)), flags; Staged val(c, h_val_mont32, n);
        std::vector<DevBuf<uint32_t>> levels; levels.reserve(4);
        if (n) { OTTI_HIP(hipMemcpyAsync(row.p, h_row, n * 4, hipMemcpyHostToDevice, c.stream)); OTTI_HIP(hipMemcpyAsync(col.p, h_col, n * 4, hipMemcpyHostToDevice, c.stream)); }
        DeviceCoo out;
        KTimer t(c, ms); dev_shard_filter(c, row.p, col.p, val.d.p, n, (int)world, (int)rank, by_col != 0, out, flags, levels); t.stop();   // (the read of the count in between included)
        if (out.n) {
            OTTI_HIP(hipMemcpyAsync(out_row, out.row.p, out.n * 4, hipMemcpyDeviceToHost, c.stream)); OTTI_HIP(hipMemcpyAsync(out_col, out.col.p, out.n * 4, hipMemcpyDeviceToHost, c.stream));
            download(c, out_val, out.val.p, out.n);
        }
        c.sync(); *out_n = out.n; return OTTI_OK;
    });
}
int32_t otti_k_fr_from_canonical(const uint8_t *in, uint8_t *out, size_t n) {
    return guarded([&] { DevCtx &c = DevCtx::get(); Staged A(c, in, n); dev_from_canonical(c, A.d.p, A.d.p, n); download(c, out, A.d.p, n); c.sync(); return OTTI_OK; });
}
int32_t otti_k_fr_to_canonical(const uint8_t *in, uint8_t *out, size_t n) {
    return guarded([&] { DevCtx &c = DevCtx::get(); Staged A(c, in, n); dev_to_canonical(c, A.d.p, A.d.p, n); download(c, out, A.d.p, n); c.sync(); return OTTI_OK; });
}
int32_t otti_k_multiply_vec(otti_instance *inst, const uint8_t *z, uint8_t *Az, uint8_t *Bz, uint8_t *Cz, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Instance &I = *inst->I; ensure_instance_device(I);
        Staged Z(c, z, 2 * I.num_vars); DevBuf<Fr> a(I.num_cons), b(I.num_cons), d(I.num_cons);
        KTimer t(c, ms); dev_spmv3(c, I.dev->by_row, Z.d.p, a.p, b.p, d.p, false, nullptr); t.stop();
        download(c, Az, a.p, I.num_cons); download(c, Bz, b.p, I.num_cons); download(c, Cz, d.p, I.num_cons); c.sync(); return OTTI_OK;
    });
}
// K staged vectors, one buffer each (what a batch of resident witnesses looks like to the many-vector kernels)
struct StagedMany {
    std::vector<std::unique_ptr<Staged>> v; std::vector<const Fr *> p;
    StagedMany(DevCtx &c, const uint8_t *const *hs, size_t K, size_t n) { for (size_t k = 0; k < K; k++) { v.push_back(std::make_unique<Staged>(c, hs[k], n)); p.push_back(v.back()->d.p); } }
};
// dev_spmv3_many on K staged vectors, tile by tile through one interleaved table (k_sparse.hip): always the many-vector kernels, K = 1 included
int32_t otti_k_multiply_vec_many(otti_instance *inst, const uint8_t *const *h_zs, size_t K, uint8_t *Az, uint8_t *Bz, uint8_t *Cz, float *ms) {
    return guarded([&] {
        if (!inst || !h_zs || !K || !Az || !Bz || !Cz) throw Error(OTTI_ERR_BAD_ARG, "null argument, or no vectors");
        for (size_t k = 0; k < K; k++) if (!h_zs[k]) throw Error(OTTI_ERR_BAD_ARG, "a null vector");
        DevCtx &c = DevCtx::get(); Instance &I = *inst->I; ensure_instance_device(I);
        const size_t N = I.num_cons, V2 = 2 * I.num_vars; const DeviceCsrSet &m = I.dev->by_row;
        StagedMany Z(c, h_zs, K, V2);
        DevBuf<Fr> z_il(kEvalTile * V2), o[3] = {DevBuf<Fr>(K * N), DevBuf<Fr>(K * N), DevBuf<Fr>(K * N)}, seg(std::max<size_t>(1, 3 * kEvalTile * m.n_seg));
        KTimer t(c, ms);
        for (size_t k0 = 0; k0 < K; k0 += kEvalTile) {
            const int nt = (int)std::min<size_t>(kEvalTile, K - k0);
            SpmvManyOut out{};
            for (int a = 0; a < nt; a++) { dev_interleave_slot(c, Z.p[k0 + a], V2, z_il.p, a); for (int j = 0; j < 3; j++) out.o[j][a] = o[j].p + (k0 + a) * N; }
            dev_spmv3_many(c, m, z_il.p, nt, out, seg.p);
        }
        t.stop();
        download(c, Az, o[0].p, K * N); download(c, Bz, o[1].p, K * N); download(c, Cz, o[2].p, K * N); c.sync(); return OTTI_OK;
    });
}
// nizk_prove_many's front half alone (prove_many.cpp prove_front_staged): the joint row jobs and tiles the plan cuts for K witnesses that keep nothing
int32_t otti_k_prove_front(otti_instance *inst, otti_gens *gens, const uint8_t *const *h_zs, const int32_t *small_flags, size_t K, uint8_t *h_rows32,
                           uint8_t *Az, uint8_t *Bz, uint8_t *Cz, otti_prove_many_info *info, float *ms) {
    return guarded([&] {
        if (!inst || !gens || !h_zs || !small_flags || !K || !h_rows32 || !Az || !Bz || !Cz) throw Error(OTTI_ERR_BAD_ARG, "null argument, or no vectors");
        for (size_t k = 0; k < K; k++) if (!h_zs[k]) throw Error(OTTI_ERR_BAD_ARG, "a null vector");
        Instance &I = *inst->I; Gens &g = *gens->g;
        {   const size_t ell = ilog2(I.num_vars);
            if (g.num_vars_padded != I.num_vars || g.R != ((size_t)1 << (ell - ell / 2))) throw Error(OTTI_ERR_BAD_ARG, "generators were made for a different instance size"); }
        DevCtx &c = DevCtx::get(); ensure_device_objects(I, g);
        const size_t N = I.num_cons, V = I.num_vars, L = V / g.R;
        StagedMany Z(c, h_zs, K, 2 * V);
        DevBuf<Pt> rows(K * L); DevBuf<uint8_t> enc(32 * K * L);
        DevBuf<Fr> o[3] = {DevBuf<Fr>(K * N), DevBuf<Fr>(K * N), DevBuf<Fr>(K * N)};
        Fr *const abc[3] = {o[0].p, o[1].p, o[2].p};
        otti_prove_many_info inf{};
        KTimer t(c, ms); prove_front_staged(I, g, Z.p.data(), small_flags, K, rows.p, abc, inf); t.stop();
        dev_encode_points(c, rows.p, K * L, enc.p);
        OTTI_HIP(hipMemcpyAsync(h_rows32, enc.p, 32 * K * L, hipMemcpyDeviceToHost, c.stream));
        download(c, Az, o[0].p, K * N); download(c, Bz, o[1].p, K * N); download(c, Cz, o[2].p, K * N); c.sync();
        if (info) *info = inf;
        return OTTI_OK;
    });
}
// the kept-products step of DeviceWitness::z_written (witness.cpp) on a caller's host state: the same dev_products_patch, so a wrong patch points at a kernel and not at a proof
int32_t otti_k_products_patch(otti_instance *inst, const uint8_t *h_z_new, const uint64_t *h_cols, size_t ncols, size_t first, size_t count,
                              uint8_t *io_Az, uint8_t *io_Bz, uint8_t *io_Cz, uint64_t *io_bits, uint64_t *io_unsat,
                              uint32_t *h_rows, size_t n_rows_cap, uint64_t *n_touched, int32_t *took_full_pass, float *kernel_ms) {
    return guarded([&] {
        if (!inst || !h_z_new || !io_Az || !io_Bz || !io_Cz || !io_bits || !io_unsat || (n_rows_cap && !h_rows) || (!h_cols && ncols)) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        Instance &I = *inst->I;
        const size_t V2 = 2 * I.num_vars, N = I.num_cons, words = (N + 63) >> 6;
        if (h_cols) {
            for (size_t i = 0; i < ncols; i++)
                if (h_cols[i] >= V2 || (i && h_cols[i] <= h_cols[i - 1])) throw Error(OTTI_ERR_INVALID_INDEX, "the columns are not strictly ascending below 2 * padded num_vars");
        } else if (first > V2 || count > V2 - first) throw Error(OTTI_ERR_INVALID_INDEX, "the range ends beyond 2 * padded num_vars");
        DevCtx &c = DevCtx::get(); ensure_instance_device(I);
        Staged Z(c, h_z_new, V2), a(c, io_Az, N), b(c, io_Bz, N), d(c, io_Cz, N);
        DevBuf<unsigned long long> bits(words), unsat(1); DevBuf<uint64_t> cols(std::max<size_t>(1, ncols));
        OTTI_HIP(hipMemcpyAsync(bits.p, io_bits, words * 8, hipMemcpyHostToDevice, c.stream));
        OTTI_HIP(hipMemcpyAsync(unsat.p, io_unsat, 8, hipMemcpyHostToDevice, c.stream));
        if (h_cols && ncols) OTTI_HIP(hipMemcpyAsync(cols.p, h_cols, ncols * 8, hipMemcpyHostToDevice, c.stream));
        const ProductsPatch p = dev_products_patch(c, *I.dev, Z.d.p, h_cols ? cols.p : nullptr, ncols, first, count, a.d.p, b.d.p, d.d.p, bits.p, unsat.p);
        download(c, io_Az, a.d.p, N); download(c, io_Bz, b.d.p, N); download(c, io_Cz, d.d.p, N);
        OTTI_HIP(hipMemcpyAsync(io_bits, bits.p, words * 8, hipMemcpyDeviceToHost, c.stream));
        const size_t k = std::min(p.n_touched, n_rows_cap);
        if (k) OTTI_HIP(hipMemcpyAsync(h_rows, c.prod_rows.p, k * 4, hipMemcpyDeviceToHost, c.stream));
        c.sync();
        *io_unsat = p.n_unsat;
        if (n_touched) *n_touched = p.n_touched;
        if (took_full_pass) *took_full_pass = p.full ? 1 : 0;
        if (kernel_ms) *kernel_ms = p.kernel_ms;
        return OTTI_OK;
    });
}
int32_t otti_k_eval_table_sparse(otti_instance *inst, const uint8_t *eq_rx, const uint8_t *rABC, uint8_t *out, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Instance &I = *inst->I; ensure_instance_device(I);
        Staged E(c, eq_rx, I.num_cons); DevBuf<Fr> o(2 * I.num_vars);
        Fr coef[3] = {fr_load(rABC), fr_load(rABC + 32), fr_load(rABC + 64)};
        KTimer t(c, ms); dev_spmv3(c, I.dev->by_col, E.d.p, o.p, nullptr, nullptr, true, coef); t.stop();
        download(c, out, o.p, 2 * I.num_vars); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_instance_evaluate(otti_instance *inst, const uint8_t *rx32, const uint8_t *ry32, size_t K, uint8_t *out32, float *ms) {
    return guarded([&] {
        if (!inst || (K && (!rx32 || !ry32 || !out32))) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (ms) *ms = 0;
        DevCtx::get();                                             // OTTI_ERR_NO_DEVICE without a device
        if (!K) return OTTI_OK;
        Instance &I = *inst->I;
        const size_t nrx = ilog2(I.num_cons), nry = ilog2(2 * I.num_vars);
        std::vector<Fr> rx(K * nrx + 1), ry(K * nry + 1);
        for (size_t i = 0; i < K * nrx; i++) rx[i] = fr_load(rx32 + 32 * i);
        for (size_t i = 0; i < K * nry; i++) ry[i] = fr_load(ry32 + 32 * i);
        std::vector<Fr> out(3 * K);
        instance_evaluate_many(I, rx.data(), nrx, ry.data(), nry, K, reinterpret_cast<Fr (*)[3]>(out.data()), ms);
        memcpy(out32, out.data(), 3 * K * sizeof(Fr));
        return OTTI_OK;
    });
}
int32_t otti_instance_device_info(otti_instance *inst, int32_t by_col, otti_device_info *out) {
    return guarded([&] {
        if (!inst || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        DevCtx::get(); Instance &I = *inst->I; ensure_instance_device(I);
        const DeviceCsrSet &m = by_col ? I.dev->by_col : I.dev->by_row;
        out->rows = m.rows; for (int k = 0; k < 3; k++) out->entries[k] = I.nnz[k];
        out->n_heavy = m.n_heavy; out->n_seg = m.n_seg; out->use_small = m.use_small ? 1 : 0; out->quad = m.quad() ? 1 : 0;
        return OTTI_OK;
    });
}
int32_t otti_k_instance_values_kernel_ms(const otti_instance *inst, float ms[2]) {
    return guarded([&] {
        if (!inst || !ms) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        const std::shared_ptr<DeviceInstance> d = inst->I->dev;
        for (int k = 0; k < 2; k++) ms[k] = d && d->slots_resident ? d->values_kernel_ms[k] : 0.0f;
        return OTTI_OK;
    });
}
int32_t otti_k_eq_evals(const uint8_t *r, size_t ell, uint8_t *out, float *ms) {
    return guarded([&] {
        if (ell > 25) throw Error(OTTI_ERR_BAD_ARG, "ell > 25");
        DevCtx &c = DevCtx::get(); std::vector<Fr> rr(ell + 1); for (size_t i = 0; i < ell; i++) rr[i] = fr_load(r + 32 * i);
        size_t n = (size_t)1 << ell; DevBuf<Fr> o(n), s(5 * 4096);
        KTimer t(c, ms); dev_eq_evals(c, rr.data(), ell, o.p, s.p); t.stop();
        download(c, out, o.p, n); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_fold_top(const uint8_t *Z, size_t len, const uint8_t *r, uint8_t *out, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Staged z(c, Z, len);
        KTimer t(c, ms); dev_fold_top(c, z.d.p, len, fr_load(r)); t.stop();
        download(c, out, z.d.p, len / 2); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_fold_bot(const uint8_t *Z, size_t len, const uint8_t *r, uint8_t *out, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Staged z(c, Z, len); DevBuf<Fr> o(std::max<size_t>(1, len / 2));
        KTimer t(c, ms); dev_fold_bot(c, z.d.p, o.p, len, fr_load(r)); t.stop();
        download(c, out, o.p, len / 2); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_sc_cubic_round(const uint8_t *A, const uint8_t *B, const uint8_t *C, const uint8_t *D, size_t len, uint8_t *e3, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Staged a(c, A, len), b(c, B, len), cc(c, C, len), d(c, D, len);
        KTimer t(c, ms); auto tk = dev_sc_cubic_eval(c, a.d.p, b.d.p, cc.d.p, d.d.p, len, 0); t.stop();
        c.wait_ticket(tk); memcpy(e3, c.h_results, 96); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_sc_cubic_fold_round(const uint8_t *A, const uint8_t *B, const uint8_t *C, const uint8_t *D, size_t len, const uint8_t *r,
                                   uint8_t *out4, uint8_t *e3, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Staged a(c, A, len), b(c, B, len), cc(c, C, len), d(c, D, len);
        KTimer t(c, ms); auto tk = dev_sc_cubic_fold_eval(c, a.d.p, b.d.p, cc.d.p, d.d.p, len, fr_load(r), 0); t.stop();
        size_t h = len / 2;
        download(c, out4, a.d.p, h); download(c, out4 + 32 * h, b.d.p, h); download(c, out4 + 64 * h, cc.d.p, h); download(c, out4 + 96 * h, d.d.p, h);
        c.sync(); c.wait_ticket(tk); memcpy(e3, c.h_results, 96); return OTTI_OK;
    });
}
int32_t otti_k_sc_quad_round(const uint8_t *A, const uint8_t *B, size_t len, uint8_t *e2, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Staged a(c, A, len), b(c, B, len);
        KTimer t(c, ms); auto tk = dev_sc_quad_eval(c, a.d.p, b.d.p, len, 0); t.stop();
        c.wait_ticket(tk); memcpy(e2, c.h_results, 64); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_sc_quad_fold_round(const uint8_t *A, const uint8_t *B, size_t len, const uint8_t *r, uint8_t *out2, uint8_t *e2, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Staged a(c, A, len), b(c, B, len);
        KTimer t(c, ms); auto tk = dev_sc_quad_fold_eval(c, a.d.p, b.d.p, len, fr_load(r), 0); t.stop();
        size_t h = len / 2; download(c, out2, a.d.p, h); download(c, out2 + 32 * h, b.d.p, h);
        c.sync(); c.wait_ticket(tk); memcpy(e2, c.h_results, 64); return OTTI_OK;
    });
}
// The round launches' grid on demand: capacities in the device's place (num_cu, then resident[] by ScKind), and the plan a launch gets under
// the capacities in force.  For the tests, which thereby walk many items per thread, or spread over the widest grid, on short tables.
int32_t otti_k_sc_caps_override(const uint32_t *caps7) {
    return guarded([&] {
        if (!caps7) { sc_caps_override(nullptr); return OTTI_OK; }
        ScCaps caps; caps.num_cu = caps7[0];
        for (int k = 0; k < kScKinds; k++) caps.resident[k] = caps7[1 + k];
        sc_caps_override(&caps); return OTTI_OK;
    });
}
int32_t otti_k_sc_plan(int32_t kind, size_t len, int32_t armed, uint32_t *workgroups, uint64_t *items_per_thread) {
    return guarded([&] {
        if (kind < 0 || kind >= kScKinds || !workgroups || !items_per_thread) throw Error(OTTI_ERR_BAD_ARG, "unknown kind of round, or null argument");
        if (!pow2(len) || len < ((kind & 1) ? 4u : 2u)) throw Error(OTTI_ERR_BAD_ARG, "table length must be a power of two >= 2 (>= 4 with a fold)");
        const ScPlan p = sc_plan((ScKind)kind, len, armed != 0, sc_caps(DevCtx::get()));
        *workgroups = p.workgroups; *items_per_thread = p.items_per_thread; return OTTI_OK;
    });
}
// Armed launches (device.h): the same fold + sums round three ways on the caller's tables — plain; armed and released by go() after
// `hold_us` microseconds of the kernel waiting; armed and ABORTED (the tables must come back untouched and the stream must drain),
// followed by another armed round that must still work.  out2/e2: the plain launch's folded tables and sums, for the caller's oracle.
int32_t otti_k_armed_selftest(const uint8_t *A, const uint8_t *B, size_t len, const uint8_t *r, uint32_t hold_us, uint8_t *out2, uint8_t *e2) {
    return guarded([&] {
        if (len < 8 || (len & (len - 1))) throw Error(OTTI_ERR_BAD_ARG, "table length must be a power of two >= 8");
        DevCtx &c = DevCtx::get();
        const Fr rr = fr_load(r); const size_t h = len / 2;
        Staged a0(c, A, len), b0(c, B, len), a1(c, A, len), b1(c, B, len);
        auto tk = dev_sc_quad_fold_eval(c, a0.d.p, b0.d.p, len, rr, 0);
        c.wait_ticket(tk); Fr e_plain[2] = {c.h_results[0], c.h_results[1]};
        download(c, out2, a0.d.p, h); download(c, out2 + 32 * h, b0.d.p, h); c.sync(); memcpy(e2, e_plain, 64);
        // armed, released late
        tk = dev_sc_quad_fold_eval_armed(c, a1.d.p, b1.d.p, len, 0);
        { const auto t0 = std::chrono::steady_clock::now(); while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(hold_us)) {} }
        c.go(&rr, 1);
        c.wait_ticket(tk);
        if (memcmp(e_plain, c.h_results, 64)) throw Error(OTTI_ERR_INTERNAL, "armed round: sums differ from the plain launch");
        std::vector<uint8_t> got(64 * h);
        download(c, got.data(), a1.d.p, h); download(c, got.data() + 32 * h, b1.d.p, h); c.sync();
        if (memcmp(got.data(), out2, 64 * h)) throw Error(OTTI_ERR_INTERNAL, "armed round: folded tables differ from the plain launch");
        // armed, aborted: nothing may be written, the stream must drain, the next armed launch must work
        std::vector<uint8_t> before(32 * h), after(32 * h);
        download(c, before.data(), a1.d.p, h); c.sync();
        tk = dev_sc_quad_fold_eval_armed(c, a1.d.p, b1.d.p, h, 0);
        c.go_abort();
        download(c, after.data(), a1.d.p, h); c.sync();
        if (memcmp(before.data(), after.data(), 32 * h)) throw Error(OTTI_ERR_INTERNAL, "aborted armed round wrote to its tables");
        if (*c.h_flag >= tk) throw Error(OTTI_ERR_INTERNAL, "aborted armed round delivered a result");
        tk = dev_sc_quad_fold_eval(c, a0.d.p, b0.d.p, h, rr, 0); c.wait_ticket(tk); e_plain[0] = c.h_results[0]; e_plain[1] = c.h_results[1];
        tk = dev_sc_quad_fold_eval_armed(c, a1.d.p, b1.d.p, h, 0); c.go(&rr, 1); c.wait_ticket(tk);
        if (memcmp(e_plain, c.h_results, 64)) throw Error(OTTI_ERR_INTERNAL, "armed round after an abort: sums differ from the plain launch");
        c.sync();
        // armed, and the host stalls beyond the launch's deadline (shortened to 2 ms here): the leader gives up for the WHOLE grid (nothing
        // folded, in any workgroup), says so, the host's wait fails at once, and the context is clean for the next round
        if (len >= 16) {
            const size_t q = h / 2;                                                      // both table pairs are down to q elements by now
            download(c, before.data(), a1.d.p, q); c.sync();
            struct Restore { DevCtx &c; unsigned long long d; ~Restore() { c.arm_deadline = d; } } restore{c, c.arm_deadline};
            c.arm_deadline = 200000ull;                                                  // 2 ms of the 100 MHz clock
            tk = dev_sc_quad_fold_eval_armed(c, a1.d.p, b1.d.p, q, 0);
            { const auto t0 = std::chrono::steady_clock::now(); while (std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(20)) {} }
            bool failed = false;
            try { c.go(&rr, 1); c.wait_ticket(tk); } catch (const Error &) { failed = true; }
            if (!failed) throw Error(OTTI_ERR_INTERNAL, "armed round past its deadline still delivered a result");
            c.arm_deadline = restore.d;
            download(c, after.data(), a1.d.p, q); c.sync();
            if (memcmp(before.data(), after.data(), 32 * q)) throw Error(OTTI_ERR_INTERNAL, "armed round past its deadline wrote to its tables");
            unsigned cnt = 1; OTTI_HIP(hipMemcpy(&cnt, c.d_counter.p, sizeof cnt, hipMemcpyDeviceToHost));
            if (cnt) throw Error(OTTI_ERR_INTERNAL, "arrival counter left non-zero after a timed-out armed round");
            tk = dev_sc_quad_fold_eval(c, a0.d.p, b0.d.p, q, rr, 0); c.wait_ticket(tk); e_plain[0] = c.h_results[0]; e_plain[1] = c.h_results[1];
            tk = dev_sc_quad_fold_eval_armed(c, a1.d.p, b1.d.p, q, 0); c.go(&rr, 1); c.wait_ticket(tk);
            if (memcmp(e_plain, c.h_results, 64)) throw Error(OTTI_ERR_INTERNAL, "armed round after a timed-out one: sums differ from the plain launch");
            c.sync();
        }
        return OTTI_OK;
    });
}
// The verifier's variable-base sum (spartan.h RowSumBeginHook / FinishHook): sum_i s[i] * decode(C[i]) on the device — batch decompression
// (k_decode_niels), LDS-bucket Pippenger (k_msm_var), window recombination on the host.  No host fallback here: this entry exists to test the device path.
int32_t otti_k_row_sum(const uint8_t *compressed32, size_t n, const uint8_t *scalars_mont32, uint8_t *out32) {
    return guarded([&] {
        if (!compressed32 || !scalars_mont32 || !out32 || n < 256) throw Error(OTTI_ERR_BAD_ARG, "null argument or fewer than 256 points");
        if (!g_row_sum_begin_hook || !g_row_sum_finish_hook) throw Error(OTTI_ERR_NO_DEVICE, "no device path registered");
        DevCtx::get();                                             // NoDevice surfaces here rather than as a declined job
        RowSumJob *job = g_row_sum_begin_hook(reinterpret_cast<const CPoint *>(compressed32), n);
        if (!job) throw Error(OTTI_ERR_NO_DEVICE, "the device declined the row sum");
        std::vector<Fr> s(n); memcpy(s.data(), scalars_mont32, 32 * n);
        Pt sum; const int rc = g_row_sum_finish_hook(job, s.data(), sum);
        if (rc == OTTI_ERR_VERIFY_DECOMPRESS) throw Error(OTTI_ERR_VERIFY_DECOMPRESS, "a point does not decode");
        if (rc) throw Error(OTTI_ERR_INTERNAL, "device row sum failed");
        pt_encode(out32, sum); return OTTI_OK;
    });
}
// Several such sums in one pass (device.h dev_row_sums_many: k_decode_niels_sets, k_msm_var_many).  Set k: points [set_offsets[k], set_offsets[k + 1])
// of compressed32 (nsets + 1 ascending offsets, in points); job j sums set job_set[j] with the next (that set's n) scalars of scalars_mont32.  No host
// fallback.  The arguments are judged before a device is touched.
int32_t otti_k_row_sum_many(size_t nsets, const uint8_t *compressed32, const size_t *set_offsets, size_t njobs, const uint32_t *job_set,
                            const uint8_t *scalars_mont32, uint8_t *out32, int32_t *codes) {
    return guarded([&] {
        if (!compressed32 || !set_offsets || !job_set || !scalars_mont32 || !out32 || !codes || !nsets || !njobs) throw Error(OTTI_ERR_BAD_ARG, "null argument, no sets or no jobs");
        std::vector<RowSumSetIn> sets(nsets); std::vector<RowSumJobIn> jobs(njobs);
        for (size_t k = 0; k < nsets; k++) {
            if (set_offsets[k + 1] <= set_offsets[k] || set_offsets[k + 1] - set_offsets[k] > kRowSumMaxPoints) throw Error(OTTI_ERR_BAD_ARG, "an empty set, or one of more than 2^20 points");
            sets[k].comp32 = compressed32 + 32 * set_offsets[k]; sets[k].n = set_offsets[k + 1] - set_offsets[k];
        }
        size_t total = 0;
        for (size_t j = 0; j < njobs; j++) { if (job_set[j] >= nsets) throw Error(OTTI_ERR_BAD_ARG, "a job names a set that is not there"); total += sets[job_set[j]].n; }
        std::vector<Fr> s(total); memcpy(s.data(), scalars_mont32, 32 * total);
        total = 0;
        for (size_t j = 0; j < njobs; j++) { jobs[j].set = job_set[j]; jobs[j].scalars = s.data() + total; total += sets[job_set[j]].n; }
        std::vector<RowSumOut> res(njobs);
        dev_row_sums_many(DevCtx::get(), sets.data(), nsets, jobs.data(), njobs, res.data());
        for (size_t j = 0; j < njobs; j++) { codes[j] = res[j].code; if (res[j].code) memset(out32 + 32 * j, 0, 32); else pt_encode(out32 + 32 * j, res[j].sum); }
        return OTTI_OK;
    });
}
// The batch verifier's device pass alone (device.h dev_batch_sum).  With two sets or more the last one stands in for the generators: decoded ahead
// (dev_decode_set), resident for the pass.  The arguments are judged before a device is touched.
int32_t otti_k_batch_sum(size_t nsets, const uint8_t *compressed32, const size_t *set_offsets, size_t njobs, const uint32_t *job_first_set,
                         const uint32_t *job_nsets, const uint8_t *scalars_mont32, uint8_t *out32, int32_t *codes, float *kernel_ms) {
    return guarded([&] {
        if (!compressed32 || !set_offsets || !job_first_set || !job_nsets || !scalars_mont32 || !out32 || !codes || !nsets || !njobs) throw Error(OTTI_ERR_BAD_ARG, "null argument, no sets or no jobs");
        if (set_offsets[0] != 0) throw Error(OTTI_ERR_BAD_ARG, "the offsets do not start at 0");
        for (size_t k = 0; k < nsets; k++)
            if (set_offsets[k + 1] <= set_offsets[k] || set_offsets[k + 1] - set_offsets[k] > kRowSumMaxPoints) throw Error(OTTI_ERR_BAD_ARG, "an empty set, or one of more than 2^20 points");
        const size_t up = nsets >= 2 ? nsets - 1 : nsets, ngens = nsets >= 2 ? set_offsets[nsets] - set_offsets[up] : 0;      // `up` sets go up in the pass
        std::vector<BatchSumJobIn> jobs(njobs); size_t total = 0;
        for (size_t j = 0; j < njobs; j++) {
            const size_t f = job_first_set[j], c = job_nsets[j];
            if (!c || f + c > nsets || (f + c == nsets && nsets >= 2 && c != 1)) throw Error(OTTI_ERR_BAD_ARG, "a job names sets that are not there, or the last set with others");
            jobs[j].first_set = f; jobs[j].nsets = c; total += set_offsets[f + c] - set_offsets[f];
        }
        std::vector<Fr> s(total); memcpy(s.data(), scalars_mont32, 32 * total);
        total = 0;
        for (size_t j = 0; j < njobs; j++) { jobs[j].scalars = s.data() + total; total += set_offsets[jobs[j].first_set + jobs[j].nsets] - set_offsets[jobs[j].first_set]; }
        DevCtx &c = DevCtx::get();
        DecodedSet last;
        if (ngens) dev_decode_set(c, compressed32 + 32 * set_offsets[up], ngens, last);
        BatchSumIn in; in.comp32 = compressed32; in.set_off = set_offsets; in.nsets = up; in.gens = ngens ? last.pts.p : nullptr; in.ngens = ngens; in.gens_bad = last.bad;
        std::vector<RowSumOut> res(njobs);
        dev_batch_sum(c, in, jobs.data(), njobs, res.data(), kernel_ms);
        for (size_t j = 0; j < njobs; j++) { codes[j] = res[j].code; if (res[j].code) memset(out32 + 32 * j, 0, 32); else pt_encode(out32 + 32 * j, res[j].sum); }
        return OTTI_OK;
    });
}
// The expansion of product-form generator runs alone (device.h dev_gen_runs: one k_gen_runs launch).  Job j has job_n[j] slots; its base, when
// job_has_base[j], is the next job_n[j] words of base_mont32; run r belongs to job run_job[r] (ascending), has run_lg[r] factors — the next of
// factors_mont32 — and the coefficient run_c_mont32[r].  out_mont32 takes the jobs' vectors one behind the other.  No host fallback.  The arguments
// are judged before a device is touched.
int32_t otti_k_gen_runs(size_t njobs, const size_t *job_n, const uint8_t *job_has_base, const uint8_t *base_mont32, size_t nruns, const uint32_t *run_job,
                        const uint32_t *run_lg, const uint8_t *run_c_mont32, const uint8_t *factors_mont32, uint8_t *out_mont32, float *kernel_ms) {
    return guarded([&] {
        if (!njobs || !job_n || !job_has_base || !out_mont32 || (nruns && (!run_job || !run_lg || !run_c_mont32))) throw Error(OTTI_ERR_BAD_ARG, "null argument, or no jobs");
        size_t total = 0, nbase = 0, nfac = 0;
        for (size_t j = 0; j < njobs; j++) {
            if (job_n[j] < 1 || job_n[j] > kRowSumMaxPoints) throw Error(OTTI_ERR_BAD_ARG, "a job of no slots, or of more than 2^20");
            total += job_n[j]; if (job_has_base[j]) nbase += job_n[j];
        }
        if (nbase && !base_mont32) throw Error(OTTI_ERR_BAD_ARG, "a job has a base and there is none");
        for (size_t r = 0; r < nruns; r++) {
            if (run_job[r] >= njobs || (r && run_job[r] < run_job[r - 1])) throw Error(OTTI_ERR_BAD_ARG, "a run names a job that is not there, or the runs are not sorted by job");
            if (run_lg[r] > kGenRunMaxLg || ((size_t)1 << run_lg[r]) > job_n[run_job[r]]) throw Error(OTTI_ERR_BAD_ARG, "a run of more slots than its job has");
            nfac += run_lg[r];
        }
        if (nfac && !factors_mont32) throw Error(OTTI_ERR_BAD_ARG, "runs with factors and there are none");
        std::vector<Fr> base(nbase), fac(nfac); std::vector<GenRunIn> runs(nruns); std::vector<GenRunsJobIn> jobs(njobs);
        if (nbase) memcpy(base.data(), base_mont32, 32 * nbase);
        if (nfac) memcpy(fac.data(), factors_mont32, 32 * nfac);
        nfac = 0;
        for (size_t r = 0; r < nruns; r++) { memcpy(&runs[r].c, run_c_mont32 + 32 * r, 32); runs[r].lg = run_lg[r]; runs[r].f = fac.data() + nfac; nfac += run_lg[r]; }
        DevCtx &c = DevCtx::get();
        DevBuf<Fr> out(total); GenRunsStaging keep;
        size_t at = 0, r = 0; nbase = 0;
        for (size_t j = 0; j < njobs; j++) {
            jobs[j].n = job_n[j]; jobs[j].out_dev = out.p + at; at += job_n[j];
            if (job_has_base[j]) { jobs[j].base = base.data() + nbase; nbase += job_n[j]; }
            jobs[j].runs = runs.data() + r;
            while (r < nruns && run_job[r] == j) { r++; jobs[j].nruns++; }
        }
        struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{c.stream};
        { KTimer t(c, kernel_ms); dev_gen_runs(c, jobs.data(), njobs, keep); t.stop(); }
        OTTI_HIP(hipMemcpyAsync(out_mont32, out.p, 32 * total, hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipStreamSynchronize(c.stream));
        return OTTI_OK;
    });
}
int32_t otti_k_msm_rows(otti_gens *gens, const uint8_t *Z, size_t L, size_t R, const uint8_t *blinds, uint8_t *out32, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Gens &g = *gens->g;
        if (R != g.R) throw Error(OTTI_ERR_BAD_ARG, "row length differs from the generator count");
        ensure_gens_device(g);
        Staged z(c, Z, L * R), bl(c, blinds, L);
        uint32_t hb = g.pc_n.h;
        const bool sparse = dev_small_fraction(c, z.d.p, L * R) > kSparseWitness;        // the prover takes this from the resident witness
        KTimer t(c, ms); dev_msm_rows(c, *g.dev, {.dense = z.d.p, .n_dense = R, .rows = L, .extra_s = bl.d.p, .extra_base = &hb, .n_extra = 1, .sparse = sparse}); t.stop();
        c.sync(); memcpy(out32, c.h_points, 32 * L); return OTTI_OK;
    });
}
// A general MsmJob through dev_msm_rows (k_msm.hip msm_launch), for the tests: any of the shapes the prover sends (no dense part, up to 8 extras on
// any base, rows shorter than the table, raw and kept sums, force_bulk) and the plan's seam bulk_workgroups (msm_plan.h).  Row sums come back
// compressed in every mode; plan5 = {kernel, chunk, nchunks, fuse, route} of the launch, from the launcher's own call of msm_plan().  The
// arguments are judged on the host, before a device is touched: the kernels take table columns from extra_base.
int32_t otti_k_msm_job(otti_gens *gens, size_t rows, size_t n_dense, const uint8_t *dense, size_t n_extra, const uint8_t *extra_s, const uint32_t *extra_base,
                       int32_t mode, int32_t sparse, int32_t force_bulk, size_t bulk_workgroups, uint8_t *out32, uint32_t *plan5, float *ms) {
    return guarded([&] {
        if (!gens || !out32 || !rows || rows > 65535) throw Error(OTTI_ERR_BAD_ARG, "null argument, or rows outside 1 .. 65535");
        Gens &g = *gens->g;
        if (n_extra > 8) throw Error(OTTI_ERR_BAD_ARG, "more than 8 extra terms");
        if (n_dense > g.R || n_dense + n_extra == 0) throw Error(OTTI_ERR_BAD_ARG, "more dense terms than generators, or no terms at all");
        if ((n_dense && !dense) || (n_extra && (!extra_s || !extra_base))) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        for (size_t e = 0; e < n_extra; e++) if (extra_base[e] >= g.R + 2) throw Error(OTTI_ERR_BAD_ARG, "an extra term's base lies beyond the table");
        if (mode != MSM_COMPRESSED && mode != MSM_RAW && mode != MSM_KEEP) throw Error(OTTI_ERR_BAD_ARG, "unknown mode");
        if (sparse < -1 || sparse > 1) throw Error(OTTI_ERR_BAD_ARG, "sparse is -1 (decide by the scalars), 0 or 1");
        if (mode == MSM_RAW && rows > kHostPtsCap) throw Error(OTTI_ERR_BAD_ARG, "more raw rows than the host's point buffer holds");
        DevCtx &c = DevCtx::get();
        ensure_gens_device(g);
        Staged z(c, dense, rows * n_dense), ex(c, extra_s, rows * n_extra);
        DevBuf<Pt> kept(rows); DevBuf<uint8_t> enc(32 * rows);
        const bool sp = sparse < 0 ? (n_dense && dev_small_fraction(c, z.d.p, rows * n_dense) > kSparseWitness) : sparse != 0;
        MsmJob job{.dense = n_dense ? z.d.p : nullptr, .n_dense = n_dense, .rows = rows, .extra_s = n_extra ? ex.d.p : nullptr, .extra_base = extra_base,
                   .n_extra = n_extra, .mode = mode, .sparse = sp};
        if (mode == MSM_KEEP) job.keep_dst = kept.p;
        job.force_bulk = force_bulk != 0;
        job.bulk_workgroups = bulk_workgroups ? bulk_workgroups : kMsmBulkWorkgroups;
        const MsmPlan p = dev_msm_plan(c, *g.dev, job);
        if (plan5) { plan5[0] = (uint32_t)p.kernel; plan5[1] = (uint32_t)p.chunk; plan5[2] = (uint32_t)p.nchunks; plan5[3] = (uint32_t)p.fuse; plan5[4] = (uint32_t)p.route; }
        KTimer t(c, ms); const MsmTicket tk = dev_msm_rows(c, *g.dev, job); t.stop();
        c.wait_points(tk);                                        // by the ticket's route: mailed and flagged sums arrive without a stream synchronise
        if (mode == MSM_COMPRESSED) { memcpy(out32, c.h_points, 32 * rows); c.sync(); return OTTI_OK; }
        if (mode == MSM_RAW) OTTI_HIP(hipMemcpyAsync(kept.p, c.h_pts, rows * sizeof(Pt), hipMemcpyHostToDevice, c.stream));
        dev_encode_points(c, kept.p, rows, enc.p);
        OTTI_HIP(hipMemcpyAsync(out32, enc.p, 32 * rows, hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipStreamSynchronize(c.stream)); return OTTI_OK;
    });
}

// (index, scalar) lists summed into L rows over the generators' table (k_msm.hip k_msm_scatter, the kernel that patches a witness's kept rows),
// here onto L identity points, which are then compressed.  The index list is judged on the host: the kernel takes table columns from it.
int32_t otti_k_msm_scatter_rows(otti_gens *gens, size_t L, const uint64_t *idx, const uint8_t *s, size_t count, uint8_t *out32, float *ms) {
    return guarded([&] {
        if (!gens || !out32 || !L || L > 4096 || (count && (!idx || !s))) throw Error(OTTI_ERR_BAD_ARG, "null argument, or L outside 1 .. 4096");
        Gens &g = *gens->g;
        for (size_t i = 0; i < count; i++)
            if (idx[i] >= L * g.R || (i && idx[i] <= idx[i - 1])) throw Error(OTTI_ERR_INVALID_INDEX, "the indices are not strictly ascending below L * R");
        DevCtx &c = DevCtx::get();
        ensure_gens_device(g);
        Staged sc(c, s, count);
        DevBuf<uint64_t> d_idx(std::max<size_t>(1, count)); DevBuf<Pt> rows(L); DevBuf<uint8_t> enc(32 * L);
        const std::vector<Pt> id(L, pt_identity());
        if (count) OTTI_HIP(hipMemcpyAsync(d_idx.p, idx, count * sizeof(uint64_t), hipMemcpyHostToDevice, c.stream));
        OTTI_HIP(hipMemcpyAsync(rows.p, id.data(), L * sizeof(Pt), hipMemcpyHostToDevice, c.stream));
        KTimer t(c, ms); dev_msm_scatter(c, *g.dev, d_idx.p, sc.d.p, count, g.R, rows.p, L); t.stop();
        dev_encode_points(c, rows.p, L, enc.p);
        OTTI_HIP(hipMemcpyAsync(out32, enc.p, 32 * L, hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipStreamSynchronize(c.stream)); return OTTI_OK;
    });
}

// DeviceWitness::assign's two passes (k_field.hip k_witness_diff_count / _scan / _apply) on a staged vector: the new vector, the ascending list of
// changed indices and their deltas.  A refused scalar is reported after the count pass, before anything is written or copied back.
int32_t otti_k_witness_diff(const uint8_t *h_old, size_t n, const void *h_src, int32_t format, size_t stride_bytes, uint8_t *h_new, uint64_t *h_idx,
                            uint8_t *h_delta, uint64_t *n_changed, uint32_t *chunk, float *ms) {
    return guarded([&] {
        if (format < OTTI_WIT_CANONICAL32 || format > OTTI_WIT_U64) throw Error(OTTI_ERR_BAD_ARG, "unknown witness format");
        const size_t eb = wit_elem_bytes(format), stride = stride_bytes ? stride_bytes : eb;
        if (stride < eb || stride % 8) throw Error(OTTI_ERR_BAD_ARG, "stride_bytes below the element size or not a multiple of 8");
        if (!n_changed || (n && (!h_old || !h_src || !h_new || !h_idx || !h_delta))) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (chunk) *chunk = (uint32_t)dev_witness_diff_chunk();
        if (!n) { *n_changed = 0; return OTTI_OK; }
        DevCtx &c = DevCtx::get();
        Staged z(c, h_old, n);
        const size_t span = (n - 1) * stride + eb;
        DevBuf<uint8_t> src(span);
        OTTI_HIP(hipMemcpyAsync(src.p, h_src, span, hipMemcpyHostToDevice, c.stream));
        KTimer t(c, ms);
        const WitDiff d = dev_witness_diff_count(c, format, src.p, stride, n, z.d.p);
        const size_t k = d.n_changed;
        if (d.bad_scalars) { t.stop(); throw Error(OTTI_ERR_INVALID_SCALAR, "non-canonical scalar in the assignment"); }
        DevBuf<uint64_t> idx(std::max<size_t>(1, k)); DevBuf<Fr> delta(std::max<size_t>(1, k));
        dev_witness_diff_apply(c, format, src.p, stride, n, z.d.p, 0, k, idx.p, delta.p, true);
        t.stop();
        download(c, h_new, z.d.p, n); download(c, h_delta, delta.p, k);
        if (k) OTTI_HIP(hipMemcpyAsync(h_idx, idx.p, k * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream));
        c.sync(); *n_changed = k; return OTTI_OK;
    });
}

// ---- the prover's own kernels for phase one / evaluation proof / bullet reduction
int32_t otti_k_eq_pyramid(const uint8_t *r, size_t n, uint8_t *out) {
    return guarded([&] {
        if (n > 13) throw Error(OTTI_ERR_BAD_ARG, "n > 13");
        DevCtx &c = DevCtx::get(); std::vector<Fr> rr = fr_load_vec(r, n); const size_t total = ((size_t)2 << n) - 1;
        DevBuf<Fr> o(total); dev_eq_pyramid(c, rr.data(), n, o.p); download(c, out, o.p, total); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_sc_cubic3_round(const uint8_t *B, const uint8_t *C, const uint8_t *D, size_t len, const uint8_t *tau, uint8_t *e3, float *ms) {
    return guarded([&] {
        if (len < 2 || (len & (len - 1))) throw Error(OTTI_ERR_BAD_ARG, "len must be a power of two >= 2");
        DevCtx &c = DevCtx::get(); Staged b(c, B, len), cc(c, C, len), d(c, D, len);
        const size_t m = ilog2(len) - 1; std::vector<Fr> t = fr_load_vec(tau, m); EqPyramids py(c, t.data(), m);
        KTimer tm(c, ms); auto tk = dev_sc_cubic3_eval(c, b.d.p, cc.d.p, d.d.p, len, py.top(), 0); tm.stop();
        c.wait_ticket(tk); memcpy(e3, c.h_results, 96); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_sc_cubic3_fold_round(const uint8_t *B, const uint8_t *C, const uint8_t *D, size_t len, const uint8_t *r, const uint8_t *tau,
                                    uint8_t *out3, uint8_t *e3, float *ms) {
    return guarded([&] {
        if (len < 4 || (len & (len - 1))) throw Error(OTTI_ERR_BAD_ARG, "len must be a power of two >= 4");
        DevCtx &c = DevCtx::get(); Staged b(c, B, len), cc(c, C, len), d(c, D, len);
        const size_t m = ilog2(len) - 2; std::vector<Fr> t = fr_load_vec(tau, m); EqPyramids py(c, t.data(), m);
        KTimer tm(c, ms); auto tk = dev_sc_cubic3_fold_eval(c, b.d.p, cc.d.p, d.d.p, len, fr_load(r), py.top(), 0); tm.stop();
        const size_t h = len / 2;
        download(c, out3, b.d.p, h); download(c, out3 + 32 * h, cc.d.p, h); download(c, out3 + 64 * h, d.d.p, h);
        c.sync(); c.wait_ticket(tk); memcpy(e3, c.h_results, 96); return OTTI_OK;
    });
}
int32_t otti_k_poly_bound(const uint8_t *Z, size_t L, size_t R, const uint8_t *Lv, uint8_t *out, float *ms) {
    return guarded([&] {
        if (!L || !R) throw Error(OTTI_ERR_BAD_ARG, "empty matrix");
        DevCtx &c = DevCtx::get(); Staged z(c, Z, L * R), lv(c, Lv, L); DevBuf<Fr> o(R), scratch(64 * R);
        KTimer tm(c, ms); dev_poly_bound(c, z.d.p, L, R, lv.d.p, o.p, scratch.p); tm.stop();
        download(c, out, o.p, R); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_bullet_round(otti_gens *gens, size_t n_cur, int32_t fold, const uint8_t *u, const uint8_t *uinv, const uint8_t *a, const uint8_t *b,
                            const uint8_t *s, const uint8_t *blinds2, uint8_t *a_out, uint8_t *b_out, uint8_t *s_out, uint8_t *LR64, float *ms) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); Gens &g = *gens->g; ensure_gens_device(g);
        const size_t R = g.R;
        if (n_cur < 2 || n_cur > R || (n_cur & (n_cur - 1))) throw Error(OTTI_ERR_BAD_ARG, "n_cur must be a power of two in [2, R]");
        const size_t n_in = fold ? 2 * n_cur : n_cur;
        if (n_in > R) throw Error(OTTI_ERR_BAD_ARG, "folding needs 2 * n_cur <= R");
        Staged A(c, a, n_in), B(c, b, n_in), S(c, s, R); DevBuf<Fr> Ao(R), Bo(R), So(R), ex(4);
        Fr exh[4] = {fr_zero(), fr_load(blinds2), fr_zero(), fr_load(blinds2 + 32)};
        OTTI_HIP(hipMemcpyAsync(ex.p, exh, sizeof exh, hipMemcpyHostToDevice, c.stream));
        OTTI_HIP(hipMemcpyAsync(So.p, S.d.p, R * sizeof(Fr), hipMemcpyDeviceToDevice, c.stream));   // slots this round does not walk keep their value
        c.ensure_points(2, 128);
        const uint32_t qh[2] = {g.pc_1.G[0], g.pc_n.h};
        const Fr uu = fold ? fr_load(u) : fr_zero(), ui = fold ? fr_load(uinv) : fr_zero();
        KTimer tm(c, ms);
        auto tk = dev_bullet_round(c, *g.dev, {.R = R, .n_cur = n_cur, .fold = fold != 0, .u = uu, .u_inv = ui, .a_in = A.d.p, .b_in = B.d.p, .s_in = S.d.p,
                                               .a_out = Ao.p, .b_out = Bo.p, .s_out = So.p, .extra_s = ex.p, .extra_base = qh});
        tm.stop();
        c.wait_points(tk); memcpy(LR64, c.h_points, 64);
        download(c, a_out, Ao.p, n_cur); download(c, b_out, Bo.p, n_cur); download(c, s_out, So.p, R); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_bullet_last_fold(size_t R, const uint8_t *u, const uint8_t *uinv, uint8_t *a2, uint8_t *b2, uint8_t *s) {
    return guarded([&] {
        if (R < 2) throw Error(OTTI_ERR_BAD_ARG, "R < 2");
        DevCtx &c = DevCtx::get(); Staged A(c, a2, 2), B(c, b2, 2), S(c, s, R); DevBuf<Fr> rows(2 * R), ex(4);
        dev_bullet_step(c, A.d.p, B.d.p, S.d.p, R, 1, true, fr_load(u), fr_load(uinv), rows.p, ex.p);
        download(c, a2, A.d.p, 1); download(c, b2, B.d.p, 1); download(c, s, S.d.p, R); c.sync(); return OTTI_OK;
    });
}

// ---- SNARK mode's kernels (k_snark.hip, snark_dev.h): each entry stages the caller's tables and calls the launch function the prover's sources (snark_encode.cpp, snark_pc.cpp, snark_prover.cpp) call.
// Lists travel as ONE array: instance y's table at element y * len; third tables only for the instances that have one (has_C[y] != 0), in order.
int32_t otti_k_pc_round(const uint8_t *A, const uint8_t *B, const uint8_t *C, const uint8_t *has_C, size_t ninst, size_t len, const uint8_t *tau, const uint8_t *r,
                        uint32_t G, uint32_t rk, uint8_t *out, uint8_t *e, float *ms) {
    return guarded([&] {
        check_pc_list(A, B, C, has_C, ninst, len);
        if (!e || (r && !out)) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (len < (r ? 4u : 2u)) throw Error(OTTI_ERR_BAD_ARG, "table length must be >= 2 (>= 4 with a fold)");
        if (!pow2(G) || rk >= G) throw Error(OTTI_ERR_BAD_ARG, "G must be a power of two and rk below it");
        const size_t items = len / (r ? 4 : 2), m = ilog2(items * G);               // the eq table covers every rank's items
        if (m > 25 || (m && !tau)) throw Error(OTTI_ERR_BAD_ARG, "eq table over more than 25 variables, or no tau");
        DevCtx &c = DevCtx::get(); StagedPc T(c, A, B, C, has_C, ninst, len);
        std::vector<Fr> t = fr_load_vec(tau, m); EqPyramids py(c, t.data(), m);
        EqSrc E = py.top(); E.stride = G; E.offset = rk;
        const Fr rr = r ? fr_load(r) : fr_zero();
        KTimer tm(c, ms); auto tk = r ? dev_pc_fold_eval(c, T.L, len, &rr, E, kSumSlot) : dev_pc_eval(c, T.L, len, E, kSumSlot); tm.stop();
        if (r) { const size_t h = len / 2; uint8_t *o = out;
            for (size_t y = 0; y < ninst; y++, o += 32 * h) download(c, o, T.L.A[y], h);
            for (size_t y = 0; y < ninst; y++, o += 32 * h) download(c, o, T.L.B[y], h);
            for (size_t y = 0; y < ninst; y++) if (T.L.C[y]) { download(c, o, T.L.C[y], h); o += 32 * h; } }
        c.sync(); c.wait_ticket(tk); memcpy(e, &c.h_results[kSumSlot], 96 * ninst); return OTTI_OK;
    });
}
// The batched launches' grid on demand (k_snark.hip pc_grid): a block cap in the device's place, and the plan a launch over ninst instances of
// `items` items gets under the cap in force.  For the tests, which thereby walk many items per thread on short tables.
int32_t otti_k_pc_grid_cap_override(const uint32_t *max_blocks) {
    return guarded([&] { pc_grid_cap_override(max_blocks ? *max_blocks : 0u); return OTTI_OK; });
}
int32_t otti_k_pc_plan(size_t ninst, size_t items, uint32_t *workgroups, uint64_t *items_per_thread) {
    return guarded([&] {
        if (!workgroups || !items_per_thread) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (ninst < 1 || ninst > 64 || items < 1) throw Error(OTTI_ERR_BAD_ARG, "1 .. 64 instances of at least one item");
        const PcGrid g = pc_grid(items, (int)ninst);
        *workgroups = g.workgroups; *items_per_thread = g.items_per_thread; return OTTI_OK;
    });
}
int32_t otti_k_pc_export(const uint8_t *A, const uint8_t *B, const uint8_t *C, const uint8_t *has_C, size_t ninst, size_t len, const uint8_t *fold_r, uint8_t *out) {
    return guarded([&] {
        check_pc_list(A, B, C, has_C, ninst, len);
        if (!out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (fold_r && len < 2) throw Error(OTTI_ERR_BAD_ARG, "table length must be >= 2 with a fold");
        const size_t n_out = fold_r ? len / 2 : len;
        if (kPcTailSlot + 3 * ninst * n_out > (size_t)kResultSlots) throw Error(OTTI_ERR_BAD_ARG, "the exported tables do not fit the pinned result buffer");
        DevCtx &c = DevCtx::get(); StagedPc T(c, A, B, C, has_C, ninst, len);
        const Fr rr = fold_r ? fr_load(fold_r) : fr_zero();
        memset(&c.h_results[kPcTailSlot], 0, 96 * ninst * n_out);                      // (an absent third table's place is not written)
        auto tk = dev_pc_export(c, T.L, len, fold_r != nullptr, fold_r ? &rr : nullptr, kPcTailSlot);
        c.wait_ticket(tk); memcpy(out, &c.h_results[kPcTailSlot], 96 * ninst * n_out); c.sync(); return OTTI_OK;
    });
}
// the rounds of one persistent launch played as pcbatch_prove plays them: per round the W * ninst mail lines summed per instance, then the challenge
int32_t otti_k_pc_tail(const uint8_t *A, const uint8_t *B, const uint8_t *C, const uint8_t *has_C, size_t ninst, size_t len0, uint32_t W, size_t t_out,
                       const uint8_t *tau, const uint8_t *rs, const uint8_t *fold_r, int32_t top, uint8_t *sums, uint8_t *out) {
    return guarded([&] {
        check_pc_list(A, B, C, has_C, ninst, len0);
        if (!tau || !rs || !sums || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (!pow2(W) || !pow2(t_out) || ninst * W > (size_t)kTailMaxGroups || len0 / W > (size_t)kTailCap || t_out < W || len0 <= t_out)
            throw Error(OTTI_ERR_BAD_ARG, "persistent sum-check tail: W and t_out powers of two, W <= t_out < len0, at most kTailCap elements per workgroup, at most kTailMaxGroups workgroups");
        if (kPcTailSlot + 3 * ninst * t_out > (size_t)kResultSlots) throw Error(OTTI_ERR_BAD_ARG, "the handed-over tables do not fit the pinned result buffer");
        const size_t nt = ilog2(len0), rounds = nt - ilog2(t_out);
        DevCtx &c = DevCtx::get();
        if (!c.armed_ok()) throw Error(OTTI_ERR_BAD_ARG, "armed launches are off: the prover would not launch the persistent tail");
        if (ninst * W > (size_t)std::min(kTailMaxGroups, c.num_cu)) throw Error(OTTI_ERR_BAD_ARG, "more workgroups than the device has CUs: the grid would not be resident as a whole");
        StagedPc T(c, A, B, C, has_C, ninst, fold_r ? 2 * len0 : len0);
        std::vector<Fr> t = fr_load_vec(tau, nt), rr = fr_load_vec(rs, rounds);
        const size_t mt = top ? nt - 1 : nt;                                            // tabulated variables; top: tau[0] travels as EqSrc.top
        EqPyramids py(c, t.data() + (top ? 1 : 0), mt);
        EqSrc E = py.top(); if (top) { E.top_bit = (int)mt; E.top = t[0]; }
        const Fr fr = fold_r ? fr_load(fold_r) : fr_zero();
        memset(&c.h_results[kPcTailSlot], 0, 96 * ninst * t_out);
        SpinPool::Session pool_session;
        struct Release { DevCtx &c; ~Release() { c.go_abort(); } } release{c};          // an exception must not leave the grid waiting for the host
        const unsigned long long seq0 = dev_pc_tail(c, T.L, (int)W, len0, t_out, fold_r ? &fr : nullptr, E, kPcTailSlot);
        for (size_t j = 0; j < rounds; j++) {
            Fr s[3 * kMaxInst];
            c.wait_tail_sums((int)ninst, (int)W, seq0 + j, s);
            memcpy(sums + 96 * ninst * j, s, 96 * ninst);
            c.go(&rr[j], 1);
        }
        c.wait_tail((int)(ninst * W), seq0 + rounds);
        memcpy(out, &c.h_results[kPcTailSlot], 96 * ninst * t_out);
        c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_prod_layer(const uint8_t *left, const uint8_t *right, size_t ninst, size_t q, uint8_t *out_left, uint8_t *out_right, float *ms) {
    return guarded([&] {
        if (!left || !right || !out_left || !out_right) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (ninst < 1 || ninst > 16 || q < 1) throw Error(OTTI_ERR_BAD_ARG, "a layer has 1 .. 16 circuits of at least one pair");
        DevCtx &c = DevCtx::get(); Staged l(c, left, ninst * 2 * q), r(c, right, ninst * 2 * q); DevBuf<Fr> ol(ninst * q), orr(ninst * q);
        LayerList L; L.n = (int)ninst;
        for (size_t y = 0; y < ninst; y++) { L.in_left[y] = l.d.p + y * 2 * q; L.in_right[y] = r.d.p + y * 2 * q; L.out_left[y] = ol.p + y * q; L.out_right[y] = orr.p + y * q; }
        KTimer tm(c, ms); dev_prod_layer(c, L, q); tm.stop();
        download(c, out_left, ol.p, ninst * q); download(c, out_right, orr.p, ninst * q); c.sync(); return OTTI_OK;
    });
}
static void check_shard(size_t n, uint32_t G, uint32_t rk) {
    if (!pow2(n) || !pow2(G) || rk >= G || n / G < 2) throw Error(OTTI_ERR_BAD_ARG, "hash layer: n and G powers of two, rk < G, at least two elements per rank");
}
int32_t otti_k_hash_mem(const uint8_t *eval_table, const uint8_t *audit_ts, size_t M, const uint8_t *r, const uint8_t *gamma, uint32_t G, uint32_t rk,
                        uint8_t *out_init, uint8_t *out_audit, float *ms) {
    return guarded([&] {
        if (!eval_table || !audit_ts || !r || !gamma || !out_init || !out_audit) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        check_shard(M, G, rk);
        DevCtx &c = DevCtx::get(); Staged ev(c, eval_table, M), au(c, audit_ts, M); const size_t Ml = M / G; DevBuf<Fr> oi(Ml), oa(Ml);
        KTimer tm(c, ms); dev_hash_mem(c, ev.d.p, au.d.p, oi.p, oa.p, M, fr_load(r), fr_load(gamma), (int)G, (int)rk); tm.stop();
        download(c, out_init, oi.p, Ml); download(c, out_audit, oa.p, Ml); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_hash_ops(const uint8_t *addr, const uint8_t *deref, const uint8_t *read_ts, size_t N, const uint8_t *r, const uint8_t *gamma, uint32_t G, uint32_t rk,
                        uint8_t *out_read, uint8_t *out_write, float *ms) {
    return guarded([&] {
        if (!addr || !deref || !read_ts || !r || !gamma || !out_read || !out_write) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        check_shard(N, G, rk);
        DevCtx &c = DevCtx::get(); Staged ad(c, addr, N), de(c, deref, N), ts(c, read_ts, N); const size_t Nl = N / G; DevBuf<Fr> ord(Nl), owr(Nl);
        KTimer tm(c, ms); dev_hash_ops(c, ad.d.p, de.d.p, ts.d.p, ord.p, owr.p, N, fr_load(r), fr_load(gamma), (int)G, (int)rk); tm.stop();
        download(c, out_read, ord.p, Nl); download(c, out_write, owr.p, Nl); c.sync(); return OTTI_OK;
    });
}
int32_t otti_k_dot_many(const uint8_t *E, const uint8_t *Ps, size_t npoly, size_t n, uint8_t *out, float *ms) {
    return guarded([&] {
        if (!E || !Ps || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (npoly < 1 || npoly > 64 || n < 1) throw Error(OTTI_ERR_BAD_ARG, "1 .. 64 polynomials of at least one element");
        DevCtx &c = DevCtx::get(); Staged e(c, E, n), p(c, Ps, npoly * n); DevBuf<Fr> partials(kSnarkPartials);
        PtrList L; L.n = (int)npoly; for (size_t y = 0; y < npoly; y++) L.p[y] = p.d.p + y * n;
        KTimer tm(c, ms); dev_dot_many(c, e.d.p, L, n, partials.p, kSumSlot); tm.stop();
        c.sync(); memcpy(out, &c.h_results[kSumSlot], 32 * npoly); return OTTI_OK;
    });
}
int32_t otti_k_sum3(const uint8_t *A, const uint8_t *B, const uint8_t *C, size_t ninst, size_t n, uint8_t *out, float *ms) {
    return guarded([&] {
        if (!A || !B || !C || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (ninst < 1 || ninst > (size_t)kMaxInst || n < 1) throw Error(OTTI_ERR_BAD_ARG, "1 .. kMaxInst triples of at least one element");
        DevCtx &c = DevCtx::get(); Staged a(c, A, ninst * n), b(c, B, ninst * n), cc(c, C, ninst * n); DevBuf<Fr> partials(kSnarkPartials);
        AbcList L; L.n = (int)ninst; for (size_t y = 0; y < ninst; y++) { L.A[y] = a.d.p + y * n; L.B[y] = b.d.p + y * n; L.C[y] = cc.d.p + y * n; }
        KTimer tm(c, ms); dev_sum3(c, L, n, partials.p, kSumSlot); tm.stop();
        c.sync(); memcpy(out, &c.h_results[kSumSlot], 32 * ninst); return OTTI_OK;
    });
}
int32_t otti_k_poly_bound_chunks(const uint8_t *Z, size_t L, size_t R, const uint8_t *Lv_rest, size_t m, uint8_t *out, int32_t *launched, float *ms) {
    return guarded([&] {
        if (!Z || !Lv_rest || !out || !launched) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (!L || !R || !m) throw Error(OTTI_ERR_BAD_ARG, "empty matrix");
        DevCtx &c = DevCtx::get(); Staged z(c, Z, L * R), lv(c, Lv_rest, m); DevBuf<Fr> o(std::max<size_t>(1, (L / m) * R)), scratch(64 * R);
        KTimer tm(c, ms); const bool ok = dev_poly_bound_chunks(c, z.d.p, L, R, lv.d.p, m, o.p, scratch.p); tm.stop();
        *launched = ok ? 1 : 0;
        if (ok) download(c, out, o.p, (L / m) * R);
        c.sync(); return OTTI_OK;
    });
}

// ---- device pointers + caller's stream
static const Fr *dfr(const void *p) { return reinterpret_cast<const Fr *>(p); }
static Fr *dfr(void *p) { return reinterpret_cast<Fr *>(p); }
int32_t otti_dev_alloc(size_t nbytes, void **out) { return guarded([&] { if (!out) throw Error(OTTI_ERR_BAD_ARG, "null argument"); DevCtx::get(); OTTI_HIP(hipMalloc(out, std::max<size_t>(nbytes, 1))); return OTTI_OK; }); }
int32_t otti_dev_free(void *d) { return guarded([&] { if (d) OTTI_HIP(hipFree(d)); return OTTI_OK; }); }
int32_t otti_dev_upload(void *d, const void *h, size_t n) { return guarded([&] { DevCtx::get(); if (n) OTTI_HIP(hipMemcpy(d, h, n, hipMemcpyHostToDevice)); return OTTI_OK; }); }
int32_t otti_dev_download(void *h, const void *d, size_t n) { return guarded([&] { DevCtx::get(); if (n) OTTI_HIP(hipMemcpy(h, d, n, hipMemcpyDeviceToHost)); return OTTI_OK; }); }
int32_t otti_dev_stream_create(void **out) { return guarded([&] { if (!out) throw Error(OTTI_ERR_BAD_ARG, "null argument"); DevCtx::get(); hipStream_t s; OTTI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); *out = (void *)s; return OTTI_OK; }); }
int32_t otti_dev_stream_sync(void *stream) { return guarded([&] { OTTI_HIP(hipStreamSynchronize((hipStream_t)stream)); return OTTI_OK; }); }
int32_t otti_dev_stream_destroy(void *stream) { return guarded([&] { if (stream) OTTI_HIP(hipStreamDestroy((hipStream_t)stream)); return OTTI_OK; }); }
int32_t otti_kd_multiply_vec(otti_instance *inst, const void *z, void *Az, void *Bz, void *Cz, void *stream) {
    return guarded([&] {
        if (!inst || !z || !Az || !Bz || !Cz) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        DevCtx &c = DevCtx::get(); Instance &I = *inst->I; ensure_instance_device(I); StreamScope ss(c, stream);
        dev_spmv3(c, I.dev->by_row, dfr(z), dfr(Az), dfr(Bz), dfr(Cz), false, nullptr); return OTTI_OK;
    });
}
int32_t otti_kd_check_sat(otti_instance *inst, const void *z, void *bits, uint64_t *n_unsat, void *stream) {
    return guarded([&] {
        if (!inst || !z || !bits) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        DevCtx &c = DevCtx::get(); Instance &I = *inst->I; ensure_instance_device(I); StreamScope ss(c, stream);
        dev_sat_pass(c, I.dev->by_row, dfr(z), reinterpret_cast<unsigned long long *>(bits));
        if (n_unsat) *n_unsat = dev_sat_count(c);                 // waits for the pass; without it the call only enqueues
        return OTTI_OK;
    });
}
int32_t otti_kd_eval_table_sparse(otti_instance *inst, const void *eq_rx, const uint8_t *rABC, void *out, void *stream) {
    return guarded([&] {
        if (!inst || !eq_rx || !rABC || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        DevCtx &c = DevCtx::get(); Instance &I = *inst->I; ensure_instance_device(I); StreamScope ss(c, stream);
        Fr coef[3] = {fr_load(rABC), fr_load(rABC + 32), fr_load(rABC + 64)};
        dev_spmv3(c, I.dev->by_col, dfr(eq_rx), dfr(out), nullptr, nullptr, true, coef); return OTTI_OK;
    });
}
int32_t otti_kd_eq_evals(const uint8_t *r, size_t ell, void *out, void *stream) {
    return guarded([&] {
        if (ell > 25 || !out) throw Error(OTTI_ERR_BAD_ARG, "ell > 25 or null output");
        DevCtx &c = DevCtx::get(); StreamScope ss(c, stream); std::vector<Fr> rr = fr_load_vec(r, ell);
        DevBuf<Fr> s(5 * 4096);
        dev_eq_evals(c, rr.data(), ell, dfr(out), s.p);
        OTTI_HIP(hipStreamSynchronize(c.stream));                // the scratch tables are freed on return
        return OTTI_OK;
    });
}
int32_t otti_kd_fold_top(void *Z, size_t len, const uint8_t *r, void *stream) {
    return guarded([&] { DevCtx &c = DevCtx::get(); StreamScope ss(c, stream); dev_fold_top(c, dfr(Z), len, fr_load(r)); return OTTI_OK; });
}
int32_t otti_kd_fold_bot(const void *Z, void *out, size_t len, const uint8_t *r, void *stream) {
    return guarded([&] { DevCtx &c = DevCtx::get(); StreamScope ss(c, stream); dev_fold_bot(c, dfr(Z), dfr(out), len, fr_load(r)); return OTTI_OK; });
}
int32_t otti_kd_sc_cubic_round(const void *A, const void *B, const void *C, const void *D, size_t len, uint8_t *e3, void *stream) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); StreamScope ss(c, stream);
        auto tk = dev_sc_cubic_eval(c, dfr(A), dfr(B), dfr(C), dfr(D), len, 0); c.wait_ticket(tk); memcpy(e3, c.h_results, 96); return OTTI_OK;
    });
}
int32_t otti_kd_sc_cubic_fold_round(void *A, void *B, void *C, void *D, size_t len, const uint8_t *r, uint8_t *e3, void *stream) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); StreamScope ss(c, stream);
        auto tk = dev_sc_cubic_fold_eval(c, dfr(A), dfr(B), dfr(C), dfr(D), len, fr_load(r), 0); c.wait_ticket(tk); memcpy(e3, c.h_results, 96); return OTTI_OK;
    });
}
int32_t otti_kd_sc_quad_round(const void *A, const void *B, size_t len, uint8_t *e2, void *stream) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); StreamScope ss(c, stream);
        auto tk = dev_sc_quad_eval(c, dfr(A), dfr(B), len, 0); c.wait_ticket(tk); memcpy(e2, c.h_results, 64); return OTTI_OK;
    });
}
int32_t otti_kd_sc_quad_fold_round(void *A, void *B, size_t len, const uint8_t *r, uint8_t *e2, void *stream) {
    return guarded([&] {
        DevCtx &c = DevCtx::get(); StreamScope ss(c, stream);
        auto tk = dev_sc_quad_fold_eval(c, dfr(A), dfr(B), len, fr_load(r), 0); c.wait_ticket(tk); memcpy(e2, c.h_results, 64); return OTTI_OK;
    });
}
int32_t otti_kd_msm_rows(otti_gens *gens, const void *Z, size_t L, size_t R, const void *blinds, void *out32, void *stream) {
    return guarded([&] {
        if (!gens || !Z || !blinds || !out32 || !L) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        DevCtx &c = DevCtx::get(); Gens &g = *gens->g;
        if (R != g.R) throw Error(OTTI_ERR_BAD_ARG, "row length differs from the generator count");
        ensure_gens_device(g); StreamScope ss(c, stream);
        uint32_t hb = g.pc_n.h;
        const MsmTicket tk = dev_msm_rows(c, *g.dev, {.dense = dfr(Z), .n_dense = R, .rows = L, .extra_s = dfr(blinds), .extra_base = &hb, .n_extra = 1});
        if (tk.points_on_device()) OTTI_HIP(hipMemcpyAsync(out32, c.d_points.p, 32 * L, hipMemcpyDeviceToDevice, c.stream));
        else { c.sync(); OTTI_HIP(hipMemcpyAsync(out32, c.h_points, 32 * L, hipMemcpyHostToDevice, c.stream)); OTTI_HIP(hipStreamSynchronize(c.stream)); }
        return OTTI_OK;
    });
}

int32_t otti_bench_madd_peak(double *madds_per_second) {
    return guarded([&] { if (!madds_per_second) throw Error(OTTI_ERR_BAD_ARG, "null argument"); *madds_per_second = dev_madd_peak(DevCtx::get()); return OTTI_OK; });
}

int32_t otti_bench_fr_mul_peak(double *products_per_second) {
    return guarded([&] { if (!products_per_second) throw Error(OTTI_ERR_BAD_ARG, "null argument"); *products_per_second = dev_fr_mul_peak(DevCtx::get()); return OTTI_OK; });
}

// ------------------------------------------------------------------------------------------------ kernel timing (HIP events on the library stream)
static const char *kClassNames[KC_COUNT] = {"msm_rows", "msm_small", "msm_finish", "sc_cubic", "sc_quad", "spmv", "eq", "reduce", "poly_bound", "bullet", "other",
                                               "pc_round", "prod_layer", "hash_layer", "gather", "dot_many", "decode", "msm_var", "sat_check"};
int32_t otti_stats_enable(int32_t on) { KStats::get().on = on != 0; KStats::get().mask = 0xffffffffu; KStats::get().reset(); return OTTI_OK; }
int32_t otti_stats_select(const char *kernel_class) {
    for (int k = 0; k < KC_COUNT; k++) if (!strcmp(kernel_class, kClassNames[k])) { KStats::get().mask = 1u << k; return OTTI_OK; }
    return OTTI_ERR_BAD_ARG;
}
int32_t otti_armed_launches_on(int32_t *on) { return guarded([&] { if (!on) throw Error(OTTI_ERR_BAD_ARG, "null argument"); *on = DevCtx::get().armed_ok() ? 1 : 0; return OTTI_OK; }); }
int32_t otti_stats_read(const char *kernel_class, uint64_t *count, double *total_ms) {
    return guarded([&] {
        KStats &s = KStats::get();
        if (s.used) { DevCtx::get().sync(); s.flush(); }
        for (int k = 0; k < KC_COUNT; k++) if (!strcmp(kernel_class, kClassNames[k])) { if (count) *count = s.count[k]; if (total_ms) *total_ms = s.total_ms[k]; return OTTI_OK; }
        throw Error(OTTI_ERR_BAD_ARG, "unknown kernel class");
    });
}

// ------------------------------------------------------------------------------------------------ u64-lane transport of Fr sums
void otti_lanes_pack(const uint8_t *fr, size_t n, uint64_t *lanes) {
    for (size_t i = 0; i < n; i++) for (int k = 0; k < 8; k++) { uint32_t w; memcpy(&w, fr + 32 * i + 4 * k, 4); lanes[8 * i + k] = w; }
}
void otti_lanes_unpack(const uint64_t *lanes, size_t n, uint8_t *fr) {
    std::vector<Fr> out(n);
    lanes_to_fr(lanes, n, out.data());                                  // shard.cpp: carries, then reduction mod l (Montgomery form kept)
    for (size_t i = 0; i < n; i++) memcpy(fr + 32 * i, out[i].v, 32);
}

}  // extern "C"
