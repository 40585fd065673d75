// Element-wise field kernels, conversions, strided gather.
#include "kernels_common.h"

namespace otti {

// ------------------------------------------------------------------------------------------------ element-wise
__global__ void k_fr_op(int op, const Fr *a, const Fr *b, Fr *out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr x = a[i], y = b[i];
        out[i] = op == 0 ? fr_mul(x, y) : op == 1 ? fr_add(x, y) : fr_sub(x, y);
    }
}
__global__ void k_fr_scale(const Fr *in, Fr k, Fr *out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = fr_mul(in[i], k);
}
__global__ void k_fr_fill(Fr *p, Fr v, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
void dev_fr_op(DevCtx &c, int op, const Fr *a, const Fr *b, Fr *out, size_t n) { if (n) hipLaunchKernelGGL(k_fr_op, grid_for(n), kBlock, 0, c.stream, op, a, b, out, n); }
void dev_scale(DevCtx &c, const Fr *in, const Fr &k, Fr *out, size_t n) { if (n) hipLaunchKernelGGL(k_fr_scale, grid_for(n), kBlock, 0, c.stream, in, k, out, n); }
void dev_from_canonical(DevCtx &c, const Fr *in, Fr *out, size_t n) { dev_scale(c, in, fr_R2(), out, n); }
void dev_to_canonical(DevCtx &c, const Fr *in, Fr *out, size_t n) { Fr one = fr_zero(); one.v[0] = 1; dev_scale(c, in, one, out, n); }
void dev_fill_zero(DevCtx &c, Fr *p, size_t n) { if (n) OTTI_HIP(hipMemsetAsync(p, 0, n * sizeof(Fr), c.stream)); }
void dev_fill_one(DevCtx &c, Fr *p, size_t n) { if (n) hipLaunchKernelGGL(k_fr_fill, grid_for(n), kBlock, 0, c.stream, p, fr_one(), n); }
void dev_fetch(DevCtx &c, const Fr *src, int slot, size_t n) { OTTI_HIP(hipMemcpyAsync(c.h_results + slot, src, n * sizeof(Fr), hipMemcpyDeviceToHost, c.stream)); }

// VarsAssignment::new on the device, from wherever an assignment lives (device.h WitFormat): element i is read at src + i * stride bytes and
// lands, in Montgomery form, in z[dst_off + i].  src is device memory that is either disjoint from the destination or is the destination
// itself, packed (src == z + dst_off, stride 32: the caller's canonical bytes uploaded as they are and converted in place — every lane loads
// all 32 bytes of its own element before it stores them).  Integers are loaded as one 8-byte word and widened; the 32-byte formats as two
// 16-byte loads when base and stride allow it (wide), else as four 8-byte ones.
// counts[0]: non-canonical scalars (upstream: R1CSError::InvalidScalar); counts[1]: scalars below 2^128 (their share picks the commitment's MSM variant)
typedef uint32_t wit_u32x4 __attribute__((ext_vector_type(4)));
template <int F> __device__ __forceinline__ Fr wit_load(const unsigned char *p, bool wide, bool &neg) {
    Fr raw; neg = false;
    if constexpr (F == WIT_I64 || F == WIT_U64) {
        unsigned long long x = *reinterpret_cast<const unsigned long long *>(p);
        if (F == WIT_I64 && (long long)x < 0) { neg = true; x = 0ull - x; }      // |INT64_MIN| = 2^63 comes out of the wrap-around as it should
        raw = fr_zero(); raw.v[0] = (uint32_t)x; raw.v[1] = (uint32_t)(x >> 32);
    } else if (wide) {
        const wit_u32x4 lo = *reinterpret_cast<const wit_u32x4 *>(p), hi = *reinterpret_cast<const wit_u32x4 *>(p + 16);
        for (int k = 0; k < 4; k++) { raw.v[k] = lo[k]; raw.v[4 + k] = hi[k]; }
    } else {
        for (int k = 0; k < 4; k++) {
            const unsigned long long w = *reinterpret_cast<const unsigned long long *>(p + 8 * k);
            raw.v[2 * k] = (uint32_t)w; raw.v[2 * k + 1] = (uint32_t)(w >> 32);
        }
    }
    return raw;
}
// THE conversion rule, for every kernel that takes witness elements in: the word wit_load<F> returned -> the Montgomery element.  An integer is
// always a scalar; a negative one is l - |x| and so never small.  A 32-byte word >= l is refused: stored as zero, and counted as small as well.
// small: the canonical value is below 2^128 (MONTGOMERY32: judged on fr_to_raw of the word).
__device__ __forceinline__ bool fr_raw_below_2p128(const Fr &c) { return (c.v[4] | c.v[5] | c.v[6] | c.v[7]) == 0; }
template <int F> __device__ __forceinline__ Fr wit_convert(Fr raw, bool neg, bool &refused, bool &small) {
    Fr out; refused = false;
    if constexpr (F == WIT_I64 || F == WIT_U64) {
        if (neg) raw = fr_sub(fr_zero(), raw);                                   // l - |x| (on canonical integers the field subtraction is the integer one mod l)
        small = !neg;
        out = fr_mul(raw, fr_R2());
    } else {
        small = fr_raw_below_2p128(F == WIT_CANONICAL32 ? raw : fr_to_raw(raw));
        if (!fr_raw_is_canonical(raw.v)) { out = fr_zero(); refused = small = true; }
        else if constexpr (F == WIT_CANONICAL32) out = fr_mul(raw, fr_R2());
        else out = raw;
    }
    return out;
}
// a lane's two tallies summed over its wave and added to counts[0], counts[1]
__device__ __forceinline__ void wit_tally(unsigned a, unsigned b, unsigned long long *counts) {
    for (int o = 32; o >= 1; o >>= 1) { a += __shfl_down(a, o); b += __shfl_down(b, o); }
    if ((threadIdx.x & 63) == 0) { if (a) atomicAdd(&counts[0], (unsigned long long)a); if (b) atomicAdd(&counts[1], (unsigned long long)b); }
}
template <int F> __global__ __launch_bounds__(kBlock) void k_witness_ingest_from(const unsigned char *src, size_t stride, size_t n, Fr *z, size_t dst_off,
                                                                               unsigned long long *counts) {
    unsigned bad = 0, nsmall = 0;
    const bool wide = (((size_t)src | stride) & 15) == 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        bool neg, refused, small; const Fr raw = wit_load<F>(src + i * stride, wide, neg);
        z[dst_off + i] = wit_convert<F>(raw, neg, refused, small);
        bad += refused; nsmall += small;
    }
    wit_tally(bad, nsmall, counts);
}
// the runtime format -> the kernels' template argument, as an std::integral_constant
template <class Fn> static void wit_dispatch(int format, Fn fn) {
    switch (format) {
    case WIT_CANONICAL32: return fn(std::integral_constant<int, WIT_CANONICAL32>{});
    case WIT_MONTGOMERY32: return fn(std::integral_constant<int, WIT_MONTGOMERY32>{});
    case WIT_I64: return fn(std::integral_constant<int, WIT_I64>{});
    case WIT_U64: return fn(std::integral_constant<int, WIT_U64>{});
    default: throw Error(OTTI_ERR_BAD_ARG, "unknown witness format");
    }
}
size_t dev_witness_ingest_from(DevCtx &c, int format, const void *src, size_t stride, size_t n, Fr *z, size_t dst_off, size_t *n_small) {
    if (n_small) *n_small = 0;
    if (!n) return 0;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(src);
    const Tallies t = counted_launch(c, [&](unsigned long long *counts) {
        KScope ks(c, KC_OTHER);
        wit_dispatch(format, [&](auto F) { hipLaunchKernelGGL(k_witness_ingest_from<decltype(F)::value>, grid_for(n), kBlock, 0, c.stream, s, stride, n, z, dst_off, counts); });
    });
    if (n_small) *n_small = (size_t)t.second;
    return (size_t)t.first;
}
// ---- a scatter update of the resident assignment (DeviceWitness::scatter): element i of the source replaces z[idx[i]].  Two launches, so that a
// refused list has changed nothing.  The first converts every element into a staging buffer by the rule above (wit_convert) and counts what the host
// refuses: counts[0] scalars >= l, counts[1] indices that are not below V or not above their predecessor (so a list that passes has no index twice).
// As for the ingest, src is either disjoint from conv or is conv itself, packed.
template <int F> __global__ __launch_bounds__(kBlock) void k_witness_scatter_check(const unsigned char *src, size_t stride, const unsigned long long *idx, size_t n,
                                                                                 size_t V, Fr *conv, unsigned long long *counts) {
    unsigned bad = 0, bad_idx = 0;
    const bool wide = (((size_t)src | stride) & 15) == 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        bool neg, refused, small; const Fr raw = wit_load<F>(src + i * stride, wide, neg);
        conv[i] = wit_convert<F>(raw, neg, refused, small);
        bad += refused;
        const unsigned long long j = idx[i];
        if (j >= V || (i > 0 && j <= idx[i - 1])) bad_idx++;
    }
    wit_tally(bad, bad_idx, counts);
}
// The second writes: the indices are distinct and below V (checked above), so no two lanes touch one element of z.  delta (kept rows only):
// what the element moved by, the scalar of its row's patch.
__global__ __launch_bounds__(kBlock) void k_witness_scatter_apply(const unsigned long long *idx, const Fr *conv, size_t n, size_t V, Fr *z, Fr *delta) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t j = (size_t)idx[i];
        if (j >= V) continue;                                                    // a list rewritten since the check: never a store outside z
        const Fr now = conv[i], old = z[j];
        z[j] = now;
        if (delta) delta[i] = fr_sub(now, old);
    }
}
void dev_witness_scatter_check(DevCtx &c, int format, const void *src, size_t stride, const uint64_t *d_idx, size_t n, size_t V, Fr *conv,
                               size_t *bad_scalars, size_t *bad_indices) {
    *bad_scalars = *bad_indices = 0;
    if (!n) return;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(src);
    const unsigned long long *ix = reinterpret_cast<const unsigned long long *>(d_idx);
    const Tallies t = counted_launch(c, [&](unsigned long long *counts) {
        KScope ks(c, KC_OTHER);
        wit_dispatch(format, [&](auto F) { hipLaunchKernelGGL(k_witness_scatter_check<decltype(F)::value>, grid_for(n), kBlock, 0, c.stream, s, stride, ix, n, V, conv, counts); });
    });
    *bad_scalars = (size_t)t.first; *bad_indices = (size_t)t.second;
}
void dev_witness_scatter_apply(DevCtx &c, const uint64_t *d_idx, const Fr *conv, size_t n, size_t V, Fr *z, Fr *delta) {
    if (!n) return;
    KScope ks(c, KC_OTHER);
    hipLaunchKernelGGL(k_witness_scatter_apply, grid_for(n), kBlock, 0, c.stream, reinterpret_cast<const unsigned long long *>(d_idx), conv, n, V, z, delta);
}
// Whole-chip throughput of the Montgomery product in GF(l) (operands in registers, every CU busy): what the sum-check, sparse-product
// and eq kernels are priced against beside the HBM roof — at 7-13 products per 192 bytes they are bounded by the multiplier first.
__global__ __launch_bounds__(kBlock) void k_fr_mul_peak(Fr *io, int iters) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    // the form the streaming kernels use since round 4: nine 29-bit limbs kept unpacked (fr9.h), two chains per lane; x <- x * y in the memory
    // format is mont261(x, 32 y) (every product below 1.1 l: no normalisation between them)
    const Fr9 y5 = fr9_unpack5(io[2 * i + 1]); Fr9 x = fr9_unpack(io[2 * i]), z = fr9_unpack(io[2 * i + 1]);
    for (int k = 0; k < iters; k++) { x = fr9_mul(x, y5); z = fr9_mul(z, y5); }
    io[2 * i] = fr_add(fr9_pack_lt2l(x), fr9_pack_lt2l(z));
}
double dev_fr_mul_peak(DevCtx &c) {
    const int blocks = 2048, iters = 250; const size_t n = (size_t)blocks * kBlock;
    DevBuf<Fr> io(2 * n);
    dev_fill_one(c, io.p, 2 * n);
    double best = 0;
    for (int rep = 0; rep < 4; rep++) {                                  // the first launch warms up; best of the rest
        OTTI_HIP(hipEventRecord(c.ev0, c.stream));
        hipLaunchKernelGGL(k_fr_mul_peak, blocks, kBlock, 0, c.stream, io.p, iters);
        OTTI_HIP(hipEventRecord(c.ev1, c.stream)); OTTI_HIP(hipEventSynchronize(c.ev1));
        float ms = 0; OTTI_HIP(hipEventElapsedTime(&ms, c.ev0, c.ev1));
        if (rep && ms > 0) best = std::max(best, 2.0 * (double)n * iters / (ms * 1e-3));
    }
    return best;
}
__global__ __launch_bounds__(kBlock) void k_gather_strided(const Fr *in, size_t stride, size_t offset, Fr *out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = in[i * stride + offset];
}
void dev_gather_strided(DevCtx &c, const Fr *in, size_t stride, size_t offset, Fr *out, size_t n) {
    KScope ks(c, KC_OTHER);
    hipLaunchKernelGGL(k_gather_strided, grid_for(n), kBlock, 0, c.stream, in, stride, offset, out, n);
}

}  // namespace otti
