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
// (the load wit_load<F>, the conversion rule wit_convert<F> and the tally wit_tally: kernels_common.h — k_wit_ingest.hip applies the same rule to the
// elements of a .wit.zkif, k_coo_ingest.hip load and rule to the coefficients of a matrix)
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
// ---- a whole assignment compared with the resident one (DeviceWitness::assign / diff): element i of the source against z[i], both in Montgomery
// form, so that equal values in other clothes (-5, l - 5 as canonical bytes, the resident word) are equal.  Workgroup c owns the FIXED contiguous
// chunk [c * kDiffChunk, (c + 1) * kDiffChunk) — no grid stride: the compacted list comes out ascending by construction.  Three launches:
//   count: chunk_counts[c] = changed elements of chunk c, counts[0] += scalars >= l, ends[0 .. 2) = the first and last changed element (what decides
//          between patching and re-summing kept rows before anything is written); writes nothing else (a refused vector has changed nothing);
//   scan:  chunk_counts[0 .. nchunks] becomes its exclusive prefix sum (entry nchunks: the total, also left in counts[1]);
//   apply: every element converted again (twice the products, against 32 bytes per element of HBM for a staging copy), its rank among the
//          chunk's changed elements from a wave ballot, a popcount prefix and the waves' counts in LDS, and for a changed element
//          idx[base + rank] = first + i (idx given), delta[base + rank] = now - old (delta given), z[i] = now (write_z).  Unchanged elements are
//          not written.  z points at the range's first element here and in the count pass; `first` only names it in the list.
// A chunk stores into its own slots [base[c], base[c + 1]) alone: a device source rewritten between the launches may change FEWER or MORE elements
// than were counted — the surplus is left as it was (z too), and slots left over are filled with the chunk's last index and a zero delta, so the
// list stays ascending (not strictly) and the patch of the kept rows (k_msm_scatter) still moves the rows by exactly what z moved by.
constexpr int kDiffChunk = 1024;               // elements per workgroup: kDiffChunk / kBlock passes of one element per lane
static_assert(kDiffChunk % kBlock == 0 && kBlock % 64 == 0, "a chunk is whole passes of whole waves");
template <int F> __device__ __forceinline__ Fr wit_diff_load(const unsigned char *src, size_t stride, bool wide, size_t i, const Fr *z, bool &changed, bool &refused, Fr &old) {
    bool neg, small; const Fr raw = wit_load<F>(src + i * stride, wide, neg);
    const Fr now = wit_convert<F>(raw, neg, refused, small);
    old = z[i];
    uint32_t d = 0;
    for (int k = 0; k < 8; k++) d |= now.v[k] ^ old.v[k];
    changed = d != 0;
    return now;
}
template <int F> __global__ __launch_bounds__(kBlock) void k_witness_diff_count(const unsigned char *src, size_t stride, size_t n, const Fr *z, unsigned long long *chunk_counts,
                                                                              unsigned long long *ends, unsigned long long *counts) {
    __shared__ unsigned s_wave[kBlock / 64];
    const bool wide = (((size_t)src | stride) & 15) == 0;
    const size_t i0 = (size_t)blockIdx.x * kDiffChunk + threadIdx.x;
    unsigned bad = 0, wave_changed = 0;                           // wave_changed, lo and hi are the same in every lane of a wave
    unsigned long long lo = ~0ull, hi = 0;                        // the wave's first and last changed element
    for (int pass = 0; pass < kDiffChunk / kBlock; pass++) {
        const size_t i = i0 + (size_t)pass * kBlock;
        bool changed = false, refused = false;
        if (i < n) { Fr old; (void)wit_diff_load<F>(src, stride, wide, i, z, changed, refused, old); }
        bad += refused;
        const unsigned long long ballot = __ballot(changed);
        if (ballot) {
            const unsigned long long lane0 = i - (threadIdx.x & 63);           // the element of the wave's lane 0 in this pass
            lo = min(lo, lane0 + (unsigned)(__ffsll((long long)ballot) - 1)); hi = max(hi, lane0 + (unsigned)(63 - __clzll((long long)ballot)));
            wave_changed += (unsigned)__popcll(ballot);
        }
    }
    if ((threadIdx.x & 63) == 0) {
        s_wave[threadIdx.x >> 6] = wave_changed;
        if (wave_changed) { atomicMin(&ends[0], lo); atomicMax(&ends[1], hi); }
    }
    __syncthreads();
    if (threadIdx.x == 0) { unsigned t = 0; for (int w = 0; w < kBlock / 64; w++) t += s_wave[w]; chunk_counts[blockIdx.x] = t; }
    wit_tally(bad, 0, counts);
}
// one workgroup: the exclusive prefix sum of v[0 .. n) in place, v[n] = the total = counts[1]
__global__ __launch_bounds__(kBlock) void k_witness_diff_scan(unsigned long long *v, size_t n, unsigned long long *counts) {
    __shared__ unsigned long long s_wave[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (size_t t0 = 0; t0 < n; t0 += kBlock) {
        const size_t i = t0 + threadIdx.x;
        const unsigned long long x = i < n ? v[i] : 0;
        unsigned long long incl = x;                              // inclusive scan over the wave
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_up(incl, o); if (lane >= o) incl += y; }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, tile = 0;
        for (int w = 0; w < kBlock / 64; w++) { const unsigned long long s = s_wave[w]; if (w < wave) before += s; tile += s; }
        if (i < n) v[i] = carry + before + incl - x;
        carry += tile;
        __syncthreads();                                          // s_wave is written again by the next tile
    }
    if (threadIdx.x == 0) { v[n] = carry; counts[1] = carry; }
}
template <int F> __global__ __launch_bounds__(kBlock) void k_witness_diff_apply(const unsigned char *src, size_t stride, size_t n, Fr *z, size_t first,
                                                                              const unsigned long long *chunk_base, unsigned long long cap,
                                                                              unsigned long long *idx, Fr *delta, bool write_z) {
    __shared__ unsigned s_wave[2][kBlock / 64];
    const unsigned long long base = chunk_base[blockIdx.x], limit = min(chunk_base[blockIdx.x + 1], cap);   // this chunk's slots, whatever the source says now
    if (base >= limit) return;                                    // the whole workgroup: nothing of this chunk was counted, or (diff) the list is full before it
    const bool wide = (((size_t)src | stride) & 15) == 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t i0 = (size_t)blockIdx.x * kDiffChunk + threadIdx.x;
    unsigned long long run = base;                                // the slot of the pass's first changed element
    for (int pass = 0; pass < kDiffChunk / kBlock; pass++) {
        const size_t i = i0 + (size_t)pass * kBlock;
        bool changed = false, refused = false; Fr now, old;
        if (i < n) now = wit_diff_load<F>(src, stride, wide, i, z, changed, refused, old);
        changed = changed && !refused;                            // the count pass saw none: a scalar >= l has appeared since, and is left out
        const unsigned long long ballot = __ballot(changed);
        if (lane == 0) s_wave[pass & 1][wave] = (unsigned)__popcll(ballot);
        __syncthreads();                                          // one barrier a pass: the next pass writes the other half of s_wave
        unsigned before = 0, total = 0;
        for (int w = 0; w < kBlock / 64; w++) { const unsigned s = s_wave[pass & 1][w]; if (w < wave) before += s; total += s; }
        const unsigned long long out = run + before + (unsigned)__popcll(ballot & ((1ull << lane) - 1));
        if (changed && out < limit) {
            if (idx) idx[out] = (unsigned long long)(first + i);
            if (delta) delta[out] = fr_sub(now, old);
            if (write_z) z[i] = now;
        }
        run += total;
    }
    // fewer changed than counted: the slots left over name the chunk's last element with a zero delta (ascending, and nothing for the patch to add)
    const size_t last = min((size_t)(blockIdx.x + 1) * kDiffChunk, n) - 1;
    for (unsigned long long out = run + threadIdx.x; out < limit; out += kBlock) { if (idx) idx[out] = (unsigned long long)(first + last); if (delta) delta[out] = fr_zero(); }
}
// c.diff_chunks: [0], [1] the first and last changed element of the latest count pass, [2] dev_witness_rows_touched's tally, [3] unused, then the
// chunks' counts / prefix sums
constexpr size_t kDiffHead = 4;
size_t dev_witness_diff_chunk() { return kDiffChunk; }
WitDiff dev_witness_diff_count(DevCtx &c, int format, const void *src, size_t stride, size_t n, const Fr *z) {
    WitDiff d;
    if (!n) return d;
    const size_t nchunks = (n + kDiffChunk - 1) / kDiffChunk;
    if (c.diff_chunks.n < kDiffHead + nchunks + 1) c.diff_chunks.alloc(kDiffHead + nchunks + 1);
    unsigned long long *head = c.diff_chunks.p, *chunks = head + kDiffHead;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(src);
    unsigned long long ends[2] = {0, 0};
    const Tallies t = counted_launch(c, [&](unsigned long long *counts) {
        OTTI_HIP(hipMemsetAsync(head, 0xff, sizeof(unsigned long long), c.stream)); OTTI_HIP(hipMemsetAsync(head + 1, 0, sizeof(unsigned long long), c.stream));
        KScope ks(c, KC_OTHER);
        wit_dispatch(format, [&](auto F) { hipLaunchKernelGGL(k_witness_diff_count<decltype(F)::value>, (unsigned)nchunks, kBlock, 0, c.stream, s, stride, n, z, chunks, head, counts); });
        hipLaunchKernelGGL(k_witness_diff_scan, 1, kBlock, 0, c.stream, chunks, nchunks, counts);
        OTTI_HIP(hipMemcpyAsync(ends, head, sizeof ends, hipMemcpyDeviceToHost, c.stream));
    });
    d.bad_scalars = (size_t)t.first; d.n_changed = (size_t)t.second; d.lo = (size_t)ends[0]; d.hi = (size_t)ends[1];
    return d;
}
void dev_witness_diff_apply(DevCtx &c, int format, const void *src, size_t stride, size_t n, Fr *z, size_t first, size_t cap, uint64_t *d_idx, Fr *delta, bool write_z) {
    if (!n || !cap) return;
    const size_t nchunks = (n + kDiffChunk - 1) / kDiffChunk;
    if (c.diff_chunks.n < kDiffHead + nchunks + 1) throw Error(OTTI_ERR_INTERNAL, "witness diff: apply without the count pass before it");
    const unsigned char *s = reinterpret_cast<const unsigned char *>(src);
    KScope ks(c, KC_OTHER);
    wit_dispatch(format, [&](auto F) {
        hipLaunchKernelGGL(k_witness_diff_apply<decltype(F)::value>, (unsigned)nchunks, kBlock, 0, c.stream, s, stride, n, z, first, c.diff_chunks.p + kDiffHead, (unsigned long long)cap,
                           reinterpret_cast<unsigned long long *>(d_idx), delta, write_z);
    });
}
// how many rows of R an ascending index list touches: the i whose row differs from their predecessor's, added to *tally
__global__ __launch_bounds__(kBlock) void k_witness_rows_touched(const unsigned long long *idx, size_t n, size_t R, unsigned long long *tally) {
    unsigned rows = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) rows += i == 0 || idx[i] / R != idx[i - 1] / R;
    for (int o = 32; o >= 1; o >>= 1) rows += __shfl_down(rows, o);
    if ((threadIdx.x & 63) == 0 && rows) atomicAdd(tally, (unsigned long long)rows);
}
void dev_witness_rows_touched(DevCtx &c, const uint64_t *d_idx, size_t n, size_t R, uint64_t *h_rows) {
    *h_rows = 0;
    if (!n) return;
    unsigned long long *tally = c.diff_chunks.p + 2;              // the count pass before this list has made the buffer
    OTTI_HIP(hipMemsetAsync(tally, 0, sizeof(unsigned long long), c.stream));
    { KScope ks(c, KC_OTHER); hipLaunchKernelGGL(k_witness_rows_touched, grid_for(n), kBlock, 0, c.stream, reinterpret_cast<const unsigned long long *>(d_idx), n, R, tally); }
    OTTI_HIP(hipMemcpyAsync(h_rows, tally, sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream));
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
