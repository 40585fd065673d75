// Test-only launches over GF(2^255-19) (otti_k_fp_op, otti_k_pt_op) and over GF(l) in nine limbs (otti_k_fr9_op): the inline functions of field.h,
// fp9.h, fp10.h and fr9.h that the MSM, sum-check, eq-table and sparse kernels are made of, one case per lane (the quad forms: one case per four
// lanes), on operands a test chooses.  Nothing is restated here: every operation is a call of the function the hot kernels call, so what these
// launches return is what k_msm.hip, k_sumcheck.hip and k_sparse.hip compute on the same operands.
#include "kernels_common.h"

namespace otti {

// ------------------------------------------------------------------------------------------------ field operations, by form
struct Fp8Ops {
    typedef Fp E; static constexpr int kLimbs = 8;
    static __device__ __forceinline__ E unpack(const Fp &a) { return a; }
    static __device__ __forceinline__ Fp pack(const E &a) { return a; }
    static __device__ __forceinline__ E repack(const Fp &a) { uint8_t b[32]; fp_to_bytes(b, a); return fp_from_bytes(b); }
    static __device__ __forceinline__ E mul(const E &a, const E &b) { return fp_mul(a, b); }
    static __device__ __forceinline__ E sqr(const E &a) { return fp_sqr(a); }
    static __device__ __forceinline__ E add(const E &a, const E &b) { return fp_add(a, b); }
    static __device__ __forceinline__ E sub(const E &a, const E &b) { return fp_sub(a, b); }
    static __device__ __forceinline__ E neg(const E &a) { return fp_neg(a); }
    static __device__ __forceinline__ E carry(const E &a) { return fp_canon(a); }            // the saturated form's normalisation: the representative below p
    static __device__ __forceinline__ E pow22523(const E &a) { return fp_pow22523(a); }
};
struct F9Ops {
    typedef F9 E; static constexpr int kLimbs = 9;
    static __device__ __forceinline__ E unpack(const Fp &a) { return f9_unpack(a); }
    static __device__ __forceinline__ Fp pack(const E &a) { return f9_pack(a); }
    static __device__ __forceinline__ E repack(const Fp &a) { return f9_unpack(f9_pack(f9_unpack(a))); }
    static __device__ __forceinline__ E mul(const E &a, const E &b) { return f9_mul(a, b); }
    static __device__ __forceinline__ E sqr(const E &a) { return f9_mul(a, a); }             // (not offered: fp9.h has no square; the host entry refuses it)
    static __device__ __forceinline__ E add(const E &a, const E &b) { return f9_add(a, b); }
    static __device__ __forceinline__ E sub(const E &a, const E &b) { return f9_sub(a, b); }
    static __device__ __forceinline__ E neg(const E &a) { return f9_neg(a); }
    static __device__ __forceinline__ E carry(const E &a) { return f9_carry(a); }
    static __device__ __forceinline__ E pow22523(const E &a) { return a; }                   // (not offered)
};
struct F10Ops {
    typedef F10 E; static constexpr int kLimbs = 10;
    static __device__ __forceinline__ E unpack(const Fp &a) { return f10_unpack(a); }
    static __device__ __forceinline__ Fp pack(const E &a) { return f10_pack(a); }
    static __device__ __forceinline__ E repack(const Fp &a) { return f10_unpack(f10_pack(f10_unpack(a))); }
    static __device__ __forceinline__ E mul(const E &a, const E &b) { return f10_mul(a, b); }
    static __device__ __forceinline__ E sqr(const E &a) { return f10_sqr(a); }
    static __device__ __forceinline__ E add(const E &a, const E &b) { return f10_add(a, b); }
    static __device__ __forceinline__ E sub(const E &a, const E &b) { return f10_sub(a, b); }
    static __device__ __forceinline__ E neg(const E &a) { return f10_neg(a); }
    static __device__ __forceinline__ E carry(const E &a) { return f10_carry(a); }
    static __device__ __forceinline__ E pow22523(const E &a) { return f10_pow22523(a); }
};

// out[i]: the packed result; limbs[i * kFpOpLimbStride ..): the raw limbs (words, for the saturated form) of the unpacked result
template <class O> __global__ __launch_bounds__(kBlock) void k_fp_op(int op, const Fp *a, const Fp *b, const Fp *c, const Fp *d, Fp *out, uint32_t *limbs, size_t n) {
    typedef typename O::E E;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const E x = O::unpack(a[i]), y = O::unpack(b[i]), z = O::unpack(c[i]), w = O::unpack(d[i]);
        E r;
        switch (op) {
        case FPOP_MUL: r = O::mul(x, y); break;
        case FPOP_SQR: r = O::sqr(x); break;
        case FPOP_ADD: r = O::add(x, y); break;
        case FPOP_SUB: r = O::sub(x, y); break;
        case FPOP_NEG: r = O::neg(x); break;
        case FPOP_CARRY: r = O::carry(O::add(O::sub(x, y), O::add(z, w))); break;
        case FPOP_REPACK: r = O::repack(a[i]); break;
        case FPOP_MUL_SUB_ADD: r = O::mul(O::sub(x, y), O::add(z, w)); break;
        case FPOP_MUL_3A_2B: r = O::mul(O::add(O::add(x, x), x), O::add(y, y)); break;
        case FPOP_MUL_F_E: r = O::mul(O::sub(O::add(x, x), y), O::sub(z, w)); break;
        case FPOP_MUL_CARRIED_F_G: r = O::mul(O::carry(O::sub(O::add(x, x), y)), O::add(O::add(z, z), w)); break;
        default: r = O::pow22523(x); break;
        }
        out[i] = O::pack(r);
        for (int k = 0; k < O::kLimbs; k++) limbs[i * kFpOpLimbStride + k] = r.v[k];
    }
}
void dev_fp_op(DevCtx &c, int form, int op, const Fp *a, const Fp *b, const Fp *cc, const Fp *d, Fp *out, uint32_t *limbs, size_t n) {
    if (!n) return;
    KScope ks(c, KC_OTHER);
    if (form == FPFORM_FP8) hipLaunchKernelGGL(k_fp_op<Fp8Ops>, grid_for(n), kBlock, 0, c.stream, op, a, b, cc, d, out, limbs, n);
    else if (form == FPFORM_F9) hipLaunchKernelGGL(k_fp_op<F9Ops>, grid_for(n), kBlock, 0, c.stream, op, a, b, cc, d, out, limbs, n);
    else hipLaunchKernelGGL(k_fp_op<F10Ops>, grid_for(n), kBlock, 0, c.stream, op, a, b, cc, d, out, limbs, n);
}

// ------------------------------------------------------------------------------------------------ point formulas
// out[i]: the packed sum; limbs[i * 4 * kFpOpLimbStride ..): the raw limbs of X, Y, Z, T as the formula left them.  Q: Niels entries for the mixed
// forms and the chain, points for the full additions.  The quad forms take four lanes per case (lane & 3 holds X, Y, Z, T); the lanes past the
// last case of the last quad's wave compute the last case again and store nothing, so that every quad permute reads live lanes.
__global__ __launch_bounds__(kBlock) void k_pt_op(int op, const Pt *P, const void *Q, int neg, uint32_t k, size_t n, Pt *out, uint32_t *limbs) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const Niels *QN = reinterpret_cast<const Niels *>(Q); const Pt *QP = reinterpret_cast<const Pt *>(Q);
    if (op == PTOP_Q10_MADD || op == PTOP_Q10_ADD) {
        const int q = threadIdx.x & 3;
        const bool live = (i >> 2) < n; const size_t cs = live ? (i >> 2) : n - 1;
        const F10 acc = f10_unpack(reinterpret_cast<const Fp *>(&P[cs])[q]);
        F10 v;
        if (op == PTOP_Q10_MADD) v = q10_load_niels(&QN[cs], neg != 0, q);
        else v = q10_cached(q10_u(f10_unpack(reinterpret_cast<const Fp *>(&QP[cs])[q]), q), q, f10_const(fp_2D()));
        const F10 r = q10_add_cached(acc, v, q);
        if (live) {
            reinterpret_cast<Fp *>(&out[cs])[q] = f10_pack(r);
            for (int j = 0; j < 10; j++) limbs[(cs * 4 + q) * kFpOpLimbStride + j] = r.v[j];
        }
        return;
    }
    if (i >= n) return;
    uint32_t *lm = limbs + i * 4 * kFpOpLimbStride;
    if (op == PTOP_P9_MADD || op == PTOP_P9_CHAIN) {
        N9 e = n9_unpack(QN[i]); if (neg) e = n9_negate(e);
        P9 r = p9_unpack(P[i]);
        const uint32_t reps = op == PTOP_P9_CHAIN ? k : 1u;
#pragma unroll 1
        for (uint32_t j = 0; j < reps; j++) r = p9_madd(r, e);
        out[i] = p9_pack(r);
        for (int j = 0; j < 9; j++) { lm[j] = r.X.v[j]; lm[kFpOpLimbStride + j] = r.Y.v[j]; lm[2 * kFpOpLimbStride + j] = r.Z.v[j]; lm[3 * kFpOpLimbStride + j] = r.T.v[j]; }
        return;
    }
    P10 r;
    if (op == PTOP_P10_MADD) { N10 e = n10_unpack(QN[i]); if (neg) e = n10_negate(e); r = p10_madd(p10_unpack(P[i]), e); }
    else r = p10_add(p10_unpack(P[i]), p10_unpack(QP[i]), f10_const(fp_2D()));
    out[i] = p10_pack(r);
    for (int j = 0; j < 10; j++) { lm[j] = r.X.v[j]; lm[kFpOpLimbStride + j] = r.Y.v[j]; lm[2 * kFpOpLimbStride + j] = r.Z.v[j]; lm[3 * kFpOpLimbStride + j] = r.T.v[j]; }
}
void dev_pt_op(DevCtx &c, int op, const Pt *P, const void *Q, bool neg, uint32_t k, size_t n, Pt *out, uint32_t *limbs) {
    if (!n) return;
    const size_t lanes = (op == PTOP_Q10_MADD || op == PTOP_Q10_ADD) ? 4 * n : n;
    KScope ks(c, KC_OTHER);
    hipLaunchKernelGGL(k_pt_op, (unsigned)((lanes + kBlock - 1) / kBlock), kBlock, 0, c.stream, op, P, Q, neg ? 1 : 0, k, n, out, limbs);
}

// ------------------------------------------------------------------------------------------------ GF(l), nine limbs of 29 bits
__device__ __forceinline__ Fr9 fr9_op_load(const uint32_t *l, size_t i) { Fr9 r; for (int k = 0; k < kFr9OpLimbs; k++) r.v[k] = l[i * kFr9OpLimbs + k]; return r; }
// out[i]: the word an operation produces; limbs[i * kFr9OpLimbs ..): the limbs it produces (device.h Fr9Op: which operands it reads)
__global__ __launch_bounds__(kBlock) void k_fr9_op(int op, const Fr *aw, const Fr *bw, const Fr *cw, const uint32_t *al, const uint32_t *bl, Fr *out, uint32_t *limbs, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr9 x = fr9_zero(), y = fr9_zero(), r = fr9_zero();
        if (fr9_op_limbs_in(op) >= 1) x = fr9_op_load(al, i);
        if (fr9_op_limbs_in(op) >= 2) y = fr9_op_load(bl, i);
        Fr w = fr_zero(); bool has_word = false, has_limbs = true;
        switch (op) {
        case FR9OP_UNPACK: r = fr9_unpack(aw[i]); break;
        case FR9OP_UNPACK5: r = fr9_unpack5(aw[i]); break;
        case FR9OP_UNPACK10: r = fr9_unpack_s<10>(aw[i]); break;
        case FR9OP_MUL: r = fr9_mul(x, y); break;
        case FR9OP_MUL_SELF: r = fr9_mul(x, x); break;
        case FR9OP_ADD: r = fr9_add(x, y); break;
        case FR9OP_NORM: r = fr9_norm(x); break;
        case FR9OP_SUB_KL2: r = fr9_sub_kl<2>(x, y); break;
        case FR9OP_SUB_KL4: r = fr9_sub_kl<4>(x, y); break;
        case FR9OP_SUB_KL8: r = fr9_sub_kl<8>(x, y); break;
        case FR9OP_SUB_KL16: r = fr9_sub_kl<16>(x, y); break;
        case FR9OP_SUB_KL128: r = fr9_sub_kl<128>(x, y); break;
        case FR9OP_FOLD_TOP: r = fr9_fold_top(x); break;
        case FR9OP_SHL5: r = fr9_shl5(x); break;
        case FR9OP_PACK_LT2L: w = fr9_pack_lt2l(x); has_word = true; has_limbs = false; break;
        case FR9OP_PACK_LT3L: w = fr9_pack_lt3l(x); has_word = true; has_limbs = false; break;
        case FR9OP_CANON: w = fr9_canon(x); has_word = true; has_limbs = false; break;
        case FR9OP_MUL9: r = fr9_mul(fr9_unpack5(aw[i]), fr9_unpack(bw[i])); w = fr9_pack_lt2l(r); has_word = true; break;
        default: r = fold9(aw[i], bw[i], fr9_unpack5(cw[i]), w); has_word = true; break;                  // FR9OP_FOLD9
        }
        if (has_word) out[i] = w;
        if (has_limbs) for (int k = 0; k < kFr9OpLimbs; k++) limbs[i * kFr9OpLimbs + k] = r.v[k];
    }
}
void dev_fr9_op(DevCtx &c, int op, const Fr *aw, const Fr *bw, const Fr *cw, const uint32_t *al, const uint32_t *bl, Fr *out, uint32_t *limbs, size_t n) {
    if (!n) return;
    KScope ks(c, KC_OTHER);
    hipLaunchKernelGGL(k_fr9_op, grid_for(n), kBlock, 0, c.stream, op, aw, bw, cw, al, bl, out, limbs, n);
}

}  // namespace otti
