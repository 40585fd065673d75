// K1 / K6: the sparse matrix-vector products (multiply_vec, compute_eval_table_sparse) and the CSR copies they read, built on the device
// from the uploaded entry lists (whole instance, or one rank's shard).
#include "kernels_common.h"

namespace otti {

// ------------------------------------------------------------------------------------------------ what every pass over a DCsr3 shares
// one entry's product.  kSmall: the coefficient is read as a 4-byte code first; only codes that are not small integers touch the 32-byte value
template <bool kSmall> __device__ __forceinline__ Fr entry_term(const DCsr3 &m, int k, uint32_t p, const Fr *x) {
    const Fr xv = x[m.idx[k][p]];
    if (kSmall) { const int32_t c = m.small[k][p]; if (c != kNotSmall) return fr_mul_small(xv, c); }
    return fr9_pack_lt2l(fr9_mul(fr9_unpack5(m.val[k][p]), fr9_unpack(xv)));           // nine limbs (fr9.h): 32 v x / 2^261 + l < 1.1 l
}
// c0 a0 + c1 a1 + c2 a2 in nine limbs (fr9.h): three products summed limb by limb, one reduction (each product < 1.1 l)
__device__ __forceinline__ Fr combine3(const Fr &c0, const Fr &c1, const Fr &c2, const Fr &a0, const Fr &a1, const Fr &a2) {
    const Fr9 t = fr9_add(fr9_add(fr9_mul(fr9_unpack5(c0), fr9_unpack(a0)), fr9_mul(fr9_unpack5(c1), fr9_unpack(a1))), fr9_mul(fr9_unpack5(c2), fr9_unpack(a2)));
    return fr9_canon(fr9_norm(t));
}
// THE long-row rule: a row (of the by-column set: a column) whose longest list exceeds kHeavyRow belongs to the workgroup-per-row or segmented
// kernels and to nobody else.  Every kernel, the CSR builder's count and its segment lists ask here, so no row is written twice or not at all.
__host__ __device__ __forceinline__ bool len_is_heavy(uint32_t longest) { return longest > (uint32_t)kHeavyRow; }
__device__ __forceinline__ bool row_is_heavy(const DCsr3 &m, size_t r) {
    return len_is_heavy(max(m.ptr[0][r + 1] - m.ptr[0][r], max(m.ptr[1][r + 1] - m.ptr[1][r], m.ptr[2][r + 1] - m.ptr[2][r])));
}
// Long lists (a linear combination over thousands of variables; the constant-1 column of a compiled circuit, which can hold O(N)
// entries in the transposed copy) are cut into segments of kHeavySeg entries: one workgroup per segment writes the three raw partial
// sums, then one workgroup per long list adds its segments up and applies the combination.
constexpr uint32_t kHeavySeg = 2048;
constexpr uint32_t kWholeList = 0xffffffffu;           // for_entries' segment number: the list is not clipped
// THE entry walk: f(p) for the entries first, first + step, .. of list k of row r — first = 0, step = 1 for a row per lane; the lane's place in its
// quad and 4 for a row per quad; threadIdx.x and kBlock for a workgroup per row — or of that list's segment sn alone.  How a row's entries are
// fetched is decided here and nowhere else.
template <class F> __device__ __forceinline__ void for_entries(const DCsr3 &m, int k, size_t r, uint32_t first, uint32_t step, uint32_t sn, F f) {
    uint32_t p = m.ptr[k][r], p1 = m.ptr[k][r + 1];
    if (sn != kWholeList) {
        const uint64_t lo = (uint64_t)p + (uint64_t)sn * kHeavySeg;
        if (lo >= p1) return;                                       // (the same for every thread of the workgroup)
        p = (uint32_t)lo; p1 = (uint32_t)min((uint64_t)p1, lo + kHeavySeg);
    }
    for (p += first; p < p1; p += step) f(p);
}
// a[k] = this lane's share (entries q, q + kLanes, ..) of <M_k row r, x>, k = 0, 1, 2: the whole sum for kLanes = 1, to be added up by quad_sum
// for 4 and by block_reduce for kBlock
template <bool kSmall, uint32_t kLanes> __device__ __forceinline__ void row_sums(const DCsr3 &m, const Fr *x, size_t r, uint32_t q, Fr (&a)[3], uint32_t sn = kWholeList) {
    for (int k = 0; k < 3; k++) {
        a[k] = fr_zero();
        for_entries(m, k, r, q, kLanes, sn, [&](uint32_t p) { a[k] = fr_add(a[k], entry_term<kSmall>(m, k, p, x)); });
    }
}
__device__ __forceinline__ Fr quad_sum(Fr a) {
    a = fr_add(a, shfl_xor_fr(a, 1)); a = fr_add(a, shfl_xor_fr(a, 2)); return a;
}
// THE segment add-up: one workgroup per long row h adds its segments' partial sums up, K of them per segment (sum j of segment s is
// partial[s * stride + j]); thread 0 ends up with the totals.  (The constant-1 column of a compiled circuit can have hundreds of segments: one
// thread walking them alone took ~90 us.)
template <int K> __device__ __forceinline__ void segment_sums(const uint32_t *seg_begin, size_t h, const Fr *partial, size_t stride, Fr (&acc)[K]) {
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = fr_zero();
    for (uint32_t s = seg_begin[h] + threadIdx.x; s < seg_begin[h + 1]; s += blockDim.x)
#pragma unroll
        for (int j = 0; j < K; j++) acc[j] = fr_add(acc[j], partial[(size_t)s * stride + j]);
    block_reduce<K>(acc);
}
// The launchers' one dispatch: a run-time flag as a compile-time constant (by_flag: the kernels with one template flag), and a set's two —
// coefficient codes, row per quad — for the row kernels (by_layout).
template <class F> static inline void by_flag(bool flag, F f) { if (flag) f(std::true_type{}); else f(std::false_type{}); }
template <class F> static inline void by_layout(const DeviceCsrSet &m, F f) {
    by_flag(m.use_small, [&](auto small) { by_flag(m.quad(), [&](auto quad) { f(small, quad); }); });
}

// ------------------------------------------------------------------------------------------------ K1 / K6 sparse products
// rows up to kHeavyRow entries, a row per lane
template <bool kSmall> __global__ __launch_bounds__(kBlock) void k_spmv3_light(DCsr3 m, size_t rows, const Fr *x, Fr *o0, Fr *o1, Fr *o2, int combine, Fr c0, Fr c1, Fr c2) {
    for (size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x; r < rows; r += (size_t)gridDim.x * blockDim.x) {
        if (row_is_heavy(m, r)) continue;
        Fr a[3];
        row_sums<kSmall, 1>(m, x, r, 0, a);
        if (combine) o0[r] = combine3(c0, c1, c2, a[0], a[1], a[2]);
        else { o0[r] = a[0]; o1[r] = a[1]; o2[r] = a[2]; }
    }
}
// The same with FOUR lanes per row (a quad walks its row four entries at a time and adds up by quad shuffles): for matrices with several
// entries per row the value / index loads of a wave are then 128-byte runs instead of one entry per lane at row-length strides.
// (Not one body with k_spmv3_light, as k_prod_rows has: merged, three of the four variants took 2 to 6 VGPRs more — profiles/sparse_walk.md.)
template <bool kSmall> __global__ __launch_bounds__(kBlock) void k_spmv3_quad(DCsr3 m, size_t rows, const Fr *x, Fr *o0, Fr *o1, Fr *o2, int combine, Fr c0, Fr c1, Fr c2) {
    const uint32_t q = threadIdx.x & 3;
    for (size_t r = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 2; r < ((rows + 63) & ~(size_t)63); r += ((size_t)gridDim.x * blockDim.x) >> 2) {
        Fr a[3] = {fr_zero(), fr_zero(), fr_zero()};
        bool heavy = false;
        if (r < rows) {
            heavy = row_is_heavy(m, r);
            if (!heavy) row_sums<kSmall, 4>(m, x, r, q, a);
        }
        for (int k = 0; k < 3; k++) a[k] = quad_sum(a[k]);         // every lane of the wave takes part (rows are padded to whole waves above)
        if (r < rows && !heavy && q == 0) {
            if (combine) o0[r] = combine3(c0, c1, c2, a[0], a[1], a[2]);
            else { o0[r] = a[0]; o1[r] = a[1]; o2[r] = a[2]; }
        }
    }
}
// a long row's segment: partial[segment * 3 + k], raw sums
template <bool kSmall> __global__ __launch_bounds__(kBlock) void k_spmv3_heavy_seg(DCsr3 m, const uint32_t *seg_row, const uint32_t *seg_no, const Fr *x, Fr *partial) {
    Fr acc[3];
    row_sums<kSmall, kBlock>(m, x, seg_row[blockIdx.x], threadIdx.x, acc, seg_no[blockIdx.x]);
    block_reduce<3>(acc);
    if (threadIdx.x == 0) for (int k = 0; k < 3; k++) partial[(size_t)blockIdx.x * 3 + k] = acc[k];
}
__global__ __launch_bounds__(kBlock) void k_spmv3_heavy_combine(const uint32_t *heavy, const uint32_t *seg_begin, size_t n_heavy, const Fr *partial, Fr *o0, Fr *o1, Fr *o2,
                                                                int combine, Fr c0, Fr c1, Fr c2) {
    Fr acc[3];
    segment_sums<3>(seg_begin, blockIdx.x, partial, 3, acc);
    if (threadIdx.x != 0) return;
    const size_t r = heavy[blockIdx.x];
    if (combine) o0[r] = fr_add(fr_add(fr_mul(c0, acc[0]), fr_mul(c1, acc[1])), fr_mul(c2, acc[2]));
    else { o0[r] = acc[0]; o1[r] = acc[1]; o2[r] = acc[2]; }
}
// every long row's segments into the CALLER's context (c.spmv_partial: the matrix object itself is shared by concurrent provers), for
// k_spmv3_heavy_combine or k_sat_heavy_check behind it
static void launch_heavy_segments(DevCtx &c, const DeviceCsrSet &m, const Fr *x) {
    if (c.spmv_partial.n < 3 * m.n_seg) { OTTI_HIP(hipStreamSynchronize(c.stream)); c.spmv_partial.alloc(3 * m.n_seg); }
    by_flag(m.use_small, [&](auto small) {
        hipLaunchKernelGGL(k_spmv3_heavy_seg<decltype(small)::value>, (unsigned)m.n_seg, kBlock, 0, c.stream, m.view(), (const uint32_t *)m.seg_row.p, (const uint32_t *)m.seg_no.p, x, c.spmv_partial.p);
    });
}
void dev_spmv3(DevCtx &c, const DeviceCsrSet &m, const Fr *x, Fr *o0, Fr *o1, Fr *o2, bool combine, const Fr coef[3]) {
    Fr z = fr_zero();
    Fr c0 = coef ? coef[0] : z, c1 = coef ? coef[1] : z, c2 = coef ? coef[2] : z;
    KScope ks(c, KC_SPMV);
    // measured on the compiler-like 2^20 instance (4.6 entries per row and matrix): 0.54 -> 0.37 ms; on the uniform one (1 entry) the quad
    // kernel would idle three lanes in four (0.16 -> 0.54 ms)
    by_layout(m, [&](auto small, auto quad) {
        constexpr bool S = decltype(small)::value, Q = decltype(quad)::value;
        hipLaunchKernelGGL((Q ? k_spmv3_quad<S> : k_spmv3_light<S>), grid_for(Q ? 4 * m.rows : m.rows), kBlock, 0, c.stream, m.view(), m.rows, x, o0, o1, o2, (int)combine, c0, c1, c2);
    });
    if (!m.n_heavy) return;
    launch_heavy_segments(c, m, x);
    hipLaunchKernelGGL(k_spmv3_heavy_combine, (unsigned)m.n_heavy, kBlock, 0, c.stream, (const uint32_t *)m.heavy.p, (const uint32_t *)m.seg_begin.p, m.n_heavy,
                       (const Fr *)c.spmv_partial.p, o0, o1, o2, (int)combine, c0, c1, c2);
}

// ------------------------------------------------------------------------------------------------ A, B, C at a tile of points (device.h dev_eval_tile)
// M_k(rx_t, ry_t) = sum over M_k's entries (r, c, v) of v ex_t[r] ey_t[c] for the nt <= KT points of a tile, in ONE walk over the by-row set: an
// entry's index, code and — for a wide coefficient — value and shifted unpack are loaded once and applied to the tile's KT values of column c.
// eq(ry): the tile's tables are stored interleaved, ey_il[col][KT], so one gather of a column brings the values of all KT points in one 32 KT-byte
// run; k_eval_expand writes them that way straight from the two factors of each table (eq(r)[i] = hi[i >> lo_bits] * lo[i & (2^lo_bits - 1)], as
// k_eq_expand forms it) — no table is staged and transposed.  eq(rx) is never written out at all: it is needed once per row, point and matrix, and
// the kernels multiply its two factors, of at most 2^12 and 2^13 elements and interleaved likewise (xlo[j][KT], xhi[h][KT]: they stay in the caches),
// where a row is finished.  The rows one thread walks share the low factor (eval_row_done), so that costs one product per row, as a table would.
// (Measured on the way, profiles/verify_many.md: with eq(ry) from its factors as well the walk costs a product more per ENTRY and point, and the
// compiler-like instance, whose walk the multiplier bounds, took 1.5 x the single evaluations' time; with both tables written out, staged and
// transposed, the uniform one took 1.25 x.)
// A row's inner sums are multiplied by ex_t[r] and added to the thread's running totals; Az, Bz, Cz are never written.  The totals are kept for ONE
// matrix at a time (KT elements: the three matrices are three walks over the rows' pointers), reduced over the workgroup and stored as its partial;
// k_eval_finish adds the partials up.  Every word is canonical after every step (comment above row_fails), so the sums do not depend on the
// geometry.  Slots t >= nt of a short tile are neither read nor accumulated: their totals stay zero.
template <int KT> struct EvalTile { const Fr *xlo, *xhi, *ey_il; int xlo_bits, nt; };
__device__ __forceinline__ Fr mul9(const Fr &a, const Fr &b) { return fr9_pack_lt2l(fr9_mul(fr9_unpack5(a), fr9_unpack(b))); }   // 32 a b / 2^261 + l < 1.1 l
// element i of point t's table from its interleaved factors
template <int KT> __device__ __forceinline__ Fr eval_eq_at(const Fr *lo_il, const Fr *hi_il, int lo_bits, size_t i, int t) {
    return mul9(hi_il[(i >> lo_bits) * KT + t], lo_il[(i & (((size_t)1 << lo_bits) - 1)) * KT + t]);
}
template <bool kSmall, int KT> __device__ __forceinline__ void entry_terms(const DCsr3 &m, int k, uint32_t p, const EvalTile<KT> &T, Fr (&acc)[KT]) {
    const Fr *xv = T.ey_il + (size_t)m.idx[k][p] * KT;
    if (kSmall) {
        const int32_t c = m.small[k][p];
        if (c != kNotSmall) {
#pragma unroll
            for (int t = 0; t < KT; t++) if (t < T.nt) acc[t] = fr_add(acc[t], fr_mul_small(xv[t], c));
            return;
        }
    }
    const Fr9 v5 = fr9_unpack5(m.val[k][p]);
#pragma unroll
    for (int t = 0; t < KT; t++) if (t < T.nt) acc[t] = fr_add(acc[t], fr9_pack_lt2l(fr9_mul(v5, fr9_unpack(xv[t]))));
}
// row_sums' tile form: this lane's share of list k of row r (or of its segment sn), added to the tile's KT inner sums
template <bool kSmall, int KT, uint32_t kLanes> __device__ __forceinline__ void row_terms(const DCsr3 &m, int k, size_t r, uint32_t q, const EvalTile<KT> &T, Fr (&acc)[KT], uint32_t sn = kWholeList) {
    for_entries(m, k, r, q, kLanes, sn, [&](uint32_t p) { entry_terms<kSmall, KT>(m, k, p, T, acc); });
}
template <int KT> __device__ __forceinline__ void eval_zero(Fr (&a)[KT]) {
#pragma unroll
    for (int t = 0; t < KT; t++) a[t] = fr_zero();
}
// The rows one thread walks lie a multiple of 2^xlo_bits apart (dev_eval_tile checks the launch geometry), so the low factor xlo_t[r & mask] is the
// SAME for all of them: a row costs one product with the high factor, tot[t] += xhi_t[r >> xlo_bits] * in[t], and the low factor is applied once,
// to the thread's total (eval_apply_low), before the workgroup adds up.
template <int KT> __device__ __forceinline__ void eval_row_done(const EvalTile<KT> &T, size_t r, const Fr (&in)[KT], Fr (&tot)[KT]) {
    const Fr *hi = T.xhi + (r >> T.xlo_bits) * KT;
#pragma unroll
    for (int t = 0; t < KT; t++) if (t < T.nt) tot[t] = fr_add(tot[t], mul9(hi[t], in[t]));
}
template <int KT> __device__ __forceinline__ void eval_apply_low(const EvalTile<KT> &T, size_t first_row, Fr (&tot)[KT]) {
    const Fr *lo = T.xlo + (first_row & (((size_t)1 << T.xlo_bits) - 1)) * KT;
#pragma unroll
    for (int t = 0; t < KT; t++) if (t < T.nt) tot[t] = mul9(lo[t], tot[t]);
}
// a workgroup's totals of matrix k: partial[(workgroup * 3 + k) * KT + t]
template <int KT> __device__ __forceinline__ void eval_store_partial(Fr (&tot)[KT], Fr *partial, size_t slot, int k) {
    block_reduce<KT>(tot);
    if (threadIdx.x == 0)
#pragma unroll
        for (int t = 0; t < KT; t++) partial[(slot * 3 + k) * KT + t] = tot[t];
}
// row per lane (k_spmv3_light's layout)
template <bool kSmall, int KT> __global__ __launch_bounds__(kBlock) void k_eval_light(DCsr3 m, size_t rows, EvalTile<KT> T, Fr *partial) {
    const size_t r0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
        Fr tot[KT]; eval_zero<KT>(tot);
        for (size_t r = r0; r < rows; r += (size_t)gridDim.x * blockDim.x) {
            if (row_is_heavy(m, r) || m.ptr[k][r] == m.ptr[k][r + 1]) continue;      // (an empty list: no product with the high factor either)
            Fr in[KT]; eval_zero<KT>(in);
            row_terms<kSmall, KT, 1>(m, k, r, 0, T, in);
            eval_row_done<KT>(T, r, in, tot);
        }
        eval_apply_low<KT>(T, r0, tot);
        eval_store_partial<KT>(tot, partial, blockIdx.x, k);
    }
}
// row per quad (k_spmv3_quad's layout and walk): rows are padded to whole waves so that every lane takes part in the shuffles.  After quad_sum all four
// lanes of a quad hold the row's KT inner sums: lane q of the quad takes point q — one product with the high factor per lane, not KT of them on one
// lane with three idle — and keeps ONE running total, that of its point.  The totals of a point then sit in the lanes q = t of every quad: they are
// added up over the wave by shuffles that keep q (offsets 4 .. 32), over the workgroup through LDS.
// The one kernel that writes for_entries' walk out: through row_terms the codes variant took 124 VGPRs for 115 and the compiler-like 2^20 tile
// 1.331 ms for 1.313 (profiles/sparse_walk.md).  A change to for_entries is made in this loop as well.
template <bool kSmall, int KT> __global__ __launch_bounds__(kBlock) void k_eval_quad(DCsr3 m, size_t rows, EvalTile<KT> T, Fr *partial) {
    static_assert(KT <= 4, "a quad's four lanes take a point each");
    __shared__ Fr sm[KT][16];
    const int q = threadIdx.x & 3, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const size_t r0 = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 2;
    const bool mine_live = q < T.nt;
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
        Fr tot = fr_zero();
        for (size_t r = r0; r < ((rows + 63) & ~(size_t)63); r += ((size_t)gridDim.x * blockDim.x) >> 2) {
            Fr in[KT]; eval_zero<KT>(in);
            const bool live = r < rows && !row_is_heavy(m, r);
            if (live) {                                                     // for_entries' walk, written out (above)
                const uint32_t p1 = m.ptr[k][r + 1];
                for (uint32_t p = m.ptr[k][r] + (uint32_t)q; p < p1; p += 4) entry_terms<kSmall, KT>(m, k, p, T, in);
            }
#pragma unroll
            for (int t = 0; t < KT; t++) in[t] = quad_sum(in[t]);          // every lane of the wave takes part
            Fr mine = in[0];
#pragma unroll
            for (int t = 1; t < KT; t++) if (q == t) mine = in[t];
            if (live && mine_live) tot = fr_add(tot, mul9(T.xhi[(r >> T.xlo_bits) * KT + q], mine));
        }
        if (mine_live) tot = mul9(T.xlo[(r0 & (((size_t)1 << T.xlo_bits) - 1)) * KT + q], tot);
#pragma unroll
        for (int off = 32; off >= 4; off >>= 1) tot = fr_add(tot, shfl_xor_fr(tot, off));
        __syncthreads();                                                   // sm may still be read for the matrix before
        if (lane < KT) sm[lane][wave] = tot;
        __syncthreads();
        if (threadIdx.x < KT) {
            Fr s = sm[threadIdx.x][0];
            for (int w = 1; w < nw; w++) s = fr_add(s, sm[threadIdx.x][w]);
            partial[((size_t)blockIdx.x * 3 + k) * KT + threadIdx.x] = s;
        }
    }
}
// the long lists, segment by segment as k_spmv3_heavy_seg walks them: seg_partial[(segment * 3 + k) * KT + t], raw inner sums
template <bool kSmall, int KT> __global__ __launch_bounds__(kBlock) void k_eval_heavy_seg(DCsr3 m, const uint32_t *seg_row, const uint32_t *seg_no, EvalTile<KT> T, Fr *seg_partial) {
    const size_t r = seg_row[blockIdx.x]; const uint32_t sn = seg_no[blockIdx.x];
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
        Fr acc[KT]; eval_zero<KT>(acc);
        row_terms<kSmall, KT, kBlock>(m, k, r, threadIdx.x, T, acc, sn);
        eval_store_partial<KT>(acc, seg_partial, blockIdx.x, k);
    }
}
// one workgroup per long row adds its segments' sums up, multiplies by ex and stores the row's share as partial slot first_slot + h: the long rows
// join the workgroups' partials and k_eval_finish sees one list
template <int KT> __global__ __launch_bounds__(kBlock) void k_eval_heavy_combine(const uint32_t *heavy, const uint32_t *seg_begin, const Fr *seg_partial, EvalTile<KT> T, Fr *partial, size_t first_slot) {
    const size_t h = blockIdx.x, r = heavy[h];
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
        Fr acc[KT];
        segment_sums<KT>(seg_begin, h, seg_partial + (size_t)k * KT, 3 * KT, acc);
        if (threadIdx.x == 0) {
            Fr tot[KT]; eval_zero<KT>(tot);
            eval_row_done<KT>(T, r, acc, tot);
            eval_apply_low<KT>(T, r, tot);
#pragma unroll
            for (int t = 0; t < KT; t++) partial[((first_slot + h) * 3 + k) * KT + t] = tot[t];
        }
    }
}
// the short second launch: workgroup (k, t) adds the n_slots partials of matrix k and point t up; out[t * 3 + k]
template <int KT> __global__ __launch_bounds__(kBlock) void k_eval_finish(const Fr *partial, size_t n_slots, int nt, Fr *out) {
    const int k = blockIdx.x % 3, t = blockIdx.x / 3;
    if (t >= nt) return;
    Fr acc[1] = {fr_zero()};
    for (size_t s = threadIdx.x; s < n_slots; s += blockDim.x) acc[0] = fr_add(acc[0], partial[(s * 3 + k) * KT + t]);
    block_reduce<1>(acc);
    if (threadIdx.x == 0) out[t * 3 + k] = acc[0];
}
// slot t of the interleaved factor tables from one point's factors: lo_il[i][KT] slot t = lo[i], i < n0, and the same for hi
template <int KT> __global__ __launch_bounds__(kBlock) void k_eval_interleave(const Fr *src0, size_t n0, Fr *dst0, const Fr *src1, size_t n1, Fr *dst1, int t) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n0 + n1; i += (size_t)gridDim.x * blockDim.x) {
        if (i < n0) dst0[i * KT + t] = src0[i]; else dst1[(i - n0) * KT + t] = src1[i - n0];
    }
}
// slot t of ey_il from one point's factors: ey_il[(h << lo_bits | j)][KT] slot t = hi[h] * lo[j] (k_eq_expand's walk: a thread keeps one lo entry
// unpacked and walks `per` hi entries; the grid's x is exact, 2^lo_bits / blockDim.x)
template <int KT> __global__ __launch_bounds__(kBlock) void k_eval_expand(const Fr *__restrict__ hi, const Fr *__restrict__ lo, int lo_bits, Fr *__restrict__ ey_il, int t, size_t n_hi, size_t per) {
    const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= ((size_t)1 << lo_bits)) return;
    const Fr9 l9 = fr9_unpack(lo[j]);
    const size_t h0 = (size_t)blockIdx.y * per, h1 = min(n_hi, h0 + per);
    for (size_t h = h0; h < h1; h++) ey_il[((h << lo_bits) | j) * KT + t] = fr9_pack_lt2l(fr9_mul(fr9_unpack5(hi[h]), l9));
}
EvalFactors eval_factors(size_t ell) { EvalFactors f; f.lo_bits = (int)std::min<size_t>(ell, 12); f.hi_bits = (int)ell - f.lo_bits; return f; }
static void eval_slot_check(int t) { if (t < 0 || t >= kEvalTile) throw Error(OTTI_ERR_INTERNAL, "evaluation tile: a slot outside the tile"); }
void dev_eval_point_x(DevCtx &c, const Fr *r, size_t ell, int t, Fr *lo_il, Fr *hi_il, Fr *scratch) {
    eval_slot_check(t);
    const EvalFactors f = eval_factors(ell);
    Fr *lo = scratch, *hi = scratch + 4096;
    dev_eq_factors(c, r, ell, (size_t)f.lo_bits, lo, hi);
    KScope ks(c, KC_EQ);
    const size_t n0 = (size_t)1 << f.lo_bits, n1 = (size_t)1 << f.hi_bits;
    hipLaunchKernelGGL(k_eval_interleave<kEvalTile>, grid_for(n0 + n1), kBlock, 0, c.stream, (const Fr *)lo, n0, lo_il, (const Fr *)hi, n1, hi_il, t);
}
void dev_eval_point_y(DevCtx &c, const Fr *r, size_t ell, int t, Fr *ey_il, Fr *scratch) {
    eval_slot_check(t);
    const EvalFactors f = eval_factors(ell);
    Fr *lo = scratch, *hi = scratch + 4096;
    dev_eq_factors(c, r, ell, (size_t)f.lo_bits, lo, hi);
    KScope ks(c, KC_EQ);
    const size_t n_lo = (size_t)1 << f.lo_bits, n_hi = (size_t)1 << f.hi_bits, per = std::min<size_t>(16, std::max<size_t>(1, n_hi / 128));
    hipLaunchKernelGGL(k_eval_expand<kEvalTile>, dim3((unsigned)((n_lo + kBlock - 1) / kBlock), (unsigned)((n_hi + per - 1) / per)), kBlock, 0, c.stream,
                       (const Fr *)hi, (const Fr *)lo, f.lo_bits, ey_il, t, n_hi, per);
}
size_t dev_eval_partial_slots(const DeviceCsrSet &m) { return (size_t)grid_for(m.quad() ? 4 * m.rows : m.rows) + m.n_heavy; }
void dev_eval_tile(DevCtx &c, const DeviceCsrSet &m, const EvalTables &tab, int nt, Fr *partial, Fr *seg_partial, Fr *out) {
    constexpr int KT = kEvalTile;
    if (nt < 1 || nt > KT) throw Error(OTTI_ERR_INTERNAL, "evaluation tile: 1 .. kEvalTile points");
    EvalTile<KT> T; T.xlo = tab.xlo; T.xhi = tab.xhi; T.ey_il = tab.ey_il; T.xlo_bits = tab.xlo_bits; T.nt = nt;
    KScope ks(c, KC_SPMV);
    const bool quad = m.quad();                        // the layouts dev_spmv3 picks, for its reasons
    const int grid = grid_for(quad ? 4 * m.rows : m.rows);
    {   // eval_apply_low's premise: a thread's rows lie a multiple of 2^xlo_bits apart, or it has at most one
        const size_t stride = ((size_t)grid * kBlock) / (quad ? 4 : 1);
        if (stride < m.rows && (stride & (((size_t)1 << tab.xlo_bits) - 1)) != 0) throw Error(OTTI_ERR_INTERNAL, "evaluation tile: the launch's row stride splits the low factor");
    }
    by_layout(m, [&](auto small, auto quad) {
        constexpr bool S = decltype(small)::value, Q = decltype(quad)::value;
        hipLaunchKernelGGL((Q ? k_eval_quad<S, KT> : k_eval_light<S, KT>), grid, kBlock, 0, c.stream, m.view(), m.rows, T, partial);
    });
    if (m.n_heavy) {
        by_flag(m.use_small, [&](auto small) {
            hipLaunchKernelGGL((k_eval_heavy_seg<decltype(small)::value, KT>), (unsigned)m.n_seg, kBlock, 0, c.stream, m.view(), (const uint32_t *)m.seg_row.p, (const uint32_t *)m.seg_no.p, T, seg_partial);
        });
        hipLaunchKernelGGL(k_eval_heavy_combine<KT>, (unsigned)m.n_heavy, kBlock, 0, c.stream, (const uint32_t *)m.heavy.p, (const uint32_t *)m.seg_begin.p, (const Fr *)seg_partial, T, partial, (size_t)grid);
    }
    hipLaunchKernelGGL(k_eval_finish<KT>, 3u * KT, kBlock, 0, c.stream, (const Fr *)partial, (size_t)grid + m.n_heavy, nt, out);
}

// ------------------------------------------------------------------------------------------------ multiply_vec for a tile of vectors (device.h dev_spmv3_many)
// Az, Bz, Cz of the nt <= KT vectors of a tile in ONE walk over the by-row set: the k_spmv3_* kernels with entry_terms / row_terms as their inner step
// and the tile's interleaved vectors, z_il[col][KT], in ey_il's place — an entry's index, code and value are loaded once for the KT witnesses.  One
// matrix at a time, as k_eval_light walks (KT accumulators live, not 3 KT).  Every partial sum is the canonical word (comment above row_fails), so the
// words stored are those dev_spmv3 stores for each vector alone, whatever the geometry.  Slots t >= nt are neither read nor written.
static_assert(kEvalTile == 4, "SpmvManyOut (device.h) holds a tile of four vectors");
template <int KT> __device__ __forceinline__ EvalTile<KT> vec_tile(const Fr *z_il, int nt) { EvalTile<KT> T; T.xlo = T.xhi = nullptr; T.ey_il = z_il; T.xlo_bits = 0; T.nt = nt; return T; }
// row per lane (k_spmv3_light's layout)
template <bool kSmall, int KT> __global__ __launch_bounds__(kBlock) void k_spmv3_many_light(DCsr3 m, size_t rows, const Fr *z_il, int nt, SpmvManyOut O) {
    const EvalTile<KT> T = vec_tile<KT>(z_il, nt);
    for (size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x; r < rows; r += (size_t)gridDim.x * blockDim.x) {
        if (row_is_heavy(m, r)) continue;
#pragma unroll 1
        for (int k = 0; k < 3; k++) {
            Fr acc[KT]; eval_zero<KT>(acc);
            row_terms<kSmall, KT, 1>(m, k, r, 0, T, acc);
#pragma unroll
            for (int t = 0; t < KT; t++) if (t < nt) O.o[k][t][r] = acc[t];
        }
    }
}
// row per quad (k_spmv3_quad's layout, walk and padding to whole waves).  After quad_sum all four lanes of a quad hold the row's KT sums: lane q
// stores vector q's, so a row's KT stores leave from four lanes at once.
template <bool kSmall, int KT> __global__ __launch_bounds__(kBlock) void k_spmv3_many_quad(DCsr3 m, size_t rows, const Fr *z_il, int nt, SpmvManyOut O) {
    static_assert(KT <= 4, "a quad's four lanes take a vector each");
    const EvalTile<KT> T = vec_tile<KT>(z_il, nt);
    const uint32_t q = threadIdx.x & 3;
    for (size_t r = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 2; r < ((rows + 63) & ~(size_t)63); r += ((size_t)gridDim.x * blockDim.x) >> 2) {
        const bool live = r < rows && !row_is_heavy(m, r);
#pragma unroll 1
        for (int k = 0; k < 3; k++) {
            Fr acc[KT]; eval_zero<KT>(acc);
            if (live) row_terms<kSmall, KT, 4>(m, k, r, q, T, acc);
#pragma unroll
            for (int t = 0; t < KT; t++) acc[t] = quad_sum(acc[t]);       // every lane of the wave takes part
            Fr mine = acc[0]; Fr *dst = O.o[k][0];
#pragma unroll
            for (int t = 1; t < KT; t++) if (q == (uint32_t)t) { mine = acc[t]; dst = O.o[k][t]; }
            if (live && (int)q < nt) dst[r] = mine;
        }
    }
}
// a long row's segment, as k_eval_heavy_seg walks it: seg_partial[(segment * 3 + k) * KT + t], raw sums
template <bool kSmall, int KT> __global__ __launch_bounds__(kBlock) void k_spmv3_many_heavy_seg(DCsr3 m, const uint32_t *seg_row, const uint32_t *seg_no, const Fr *z_il, int nt, Fr *seg_partial) {
    const EvalTile<KT> T = vec_tile<KT>(z_il, nt);
    const size_t r = seg_row[blockIdx.x]; const uint32_t sn = seg_no[blockIdx.x];
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
        Fr acc[KT]; eval_zero<KT>(acc);
        row_terms<kSmall, KT, kBlock>(m, k, r, threadIdx.x, T, acc, sn);
        eval_store_partial<KT>(acc, seg_partial, blockIdx.x, k);
    }
}
// one workgroup per long row adds its segments' sums up and stores the row's KT x 3 words
template <int KT> __global__ __launch_bounds__(kBlock) void k_spmv3_many_heavy_combine(const uint32_t *heavy, const uint32_t *seg_begin, const Fr *seg_partial, int nt, SpmvManyOut O) {
    const size_t h = blockIdx.x, r = heavy[h];
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
        Fr acc[KT];
        segment_sums<KT>(seg_begin, h, seg_partial + (size_t)k * KT, 3 * KT, acc);
        if (threadIdx.x == 0)
#pragma unroll
            for (int t = 0; t < KT; t++) if (t < nt) O.o[k][t][r] = acc[t];
    }
}
void dev_interleave_slot(DevCtx &c, const Fr *src, size_t n, Fr *dst_il, int t) {
    eval_slot_check(t);
    KScope ks(c, KC_SPMV);                                    // the tile's cost beside K single passes includes putting its vectors side by side
    hipLaunchKernelGGL(k_eval_interleave<kEvalTile>, grid_for(n), kBlock, 0, c.stream, src, n, dst_il, (const Fr *)nullptr, (size_t)0, (Fr *)nullptr, t);
}
void dev_spmv3_many(DevCtx &c, const DeviceCsrSet &m, const Fr *z_il, int nt, const SpmvManyOut &out, Fr *seg_partial) {
    constexpr int KT = kEvalTile;
    if (nt < 1 || nt > KT) throw Error(OTTI_ERR_INTERNAL, "vector tile: 1 .. kEvalTile vectors");
    for (int k = 0; k < 3; k++) for (int t = 0; t < nt; t++) if (!out.o[k][t]) throw Error(OTTI_ERR_INTERNAL, "vector tile: a live slot without an output");
    if (m.n_heavy && !seg_partial) throw Error(OTTI_ERR_INTERNAL, "vector tile: long rows without segment memory");
    KScope ks(c, KC_SPMV);
    by_layout(m, [&](auto small, auto quad) {                 // the layouts dev_spmv3 picks, for its reasons
        constexpr bool S = decltype(small)::value, Q = decltype(quad)::value;
        hipLaunchKernelGGL((Q ? k_spmv3_many_quad<S, KT> : k_spmv3_many_light<S, KT>), grid_for(Q ? 4 * m.rows : m.rows), kBlock, 0, c.stream, m.view(), m.rows, z_il, nt, out);
    });
    if (!m.n_heavy) return;
    by_flag(m.use_small, [&](auto small) {
        hipLaunchKernelGGL((k_spmv3_many_heavy_seg<decltype(small)::value, KT>), (unsigned)m.n_seg, kBlock, 0, c.stream, m.view(), (const uint32_t *)m.seg_row.p, (const uint32_t *)m.seg_no.p, z_il, nt, seg_partial);
    });
    hipLaunchKernelGGL(k_spmv3_many_heavy_combine<KT>, (unsigned)m.n_heavy, kBlock, 0, c.stream, (const uint32_t *)m.heavy.p, (const uint32_t *)m.seg_begin.p, (const Fr *)seg_partial, nt, out);
}

// ------------------------------------------------------------------------------------------------ satisfiability pass (Instance::is_sat on the device)
// Per constraint row r: a = <A_r,z>, b = <B_r,z>, c = <C_r,z> formed exactly as the products above form them, then a b == c in GF(l).  Az, Bz and
// Cz are never written: a row's only output is bit (r & 63) of bits[r >> 6], set when the row FAILS, and the failing rows are counted in *count.
// Forms: z and the coefficients are canonical Montgomery words (< l).  entry_term ends in a conditional subtraction (both of its paths return a
// word in [0, l)) and fr_add keeps [0, l), so row_sums — and a quad's or a workgroup's sum of such words — is the CANONICAL Montgomery word of the
// row sum, never a representative in [l, 2l).  fr_mul(aR, bR) is the canonical word of abR.  Equal field elements are therefore equal words and
// the comparison is a plain word compare.  The verdict depends on the row alone, so every launch geometry gives the same bitmap and count.
// Bitmap writes: a wave owns whole 64-row words and lane 0 stores each with one ordinary 8-byte store (every word of the bitmap is written,
// so it needs no zeroing); only the long rows, judged by a later launch, come in with atomicOr.  The count costs one atomicAdd per wave with
// failures: at most one per wave of the grid when every row fails.
__device__ __forceinline__ bool row_fails(const Fr &a, const Fr &b, const Fr &c) { return !fr_eq(fr_mul(a, b), c); }
// row per lane (k_spmv3_light's layout): a wave's 64 rows are one word, its verdicts one __ballot
template <bool kSmall> __global__ __launch_bounds__(kBlock) void k_sat_light(DCsr3 m, size_t rows, const Fr *x, unsigned long long *bits, unsigned long long *count) {
    unsigned long long mine = 0;                                    // failing rows of this wave's words (lane 0)
    const size_t padded = (rows + 63) & ~(size_t)63;                // grid strides are multiples of 64: a wave enters and leaves the loop as a whole
    for (size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x; r < padded; r += (size_t)gridDim.x * blockDim.x) {
        bool fail = false;
        if (r < rows && !row_is_heavy(m, r)) {
            Fr a[3];
            row_sums<kSmall, 1>(m, x, r, 0, a);
            fail = row_fails(a[0], a[1], a[2]);
        }
        const unsigned long long word = (unsigned long long)__ballot(fail);
        if ((threadIdx.x & 63) == 0) { bits[r >> 6] = word; mine += (unsigned long long)__popcll(word); }
    }
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}
// bits 0, 4, 8, .. 60 of a ballot (one lane of each quad) packed into bits 0 .. 15
__device__ __forceinline__ unsigned long long quad_votes(unsigned long long v) {
    v &= 0x1111111111111111ull;
    v = (v | (v >> 3)) & 0x0303030303030303ull;
    v = (v | (v >> 6)) & 0x000f000f000f000full;
    v = (v | (v >> 12)) & 0x000000ff000000ffull;
    return (v | (v >> 24)) & 0xffffull;
}
// row per quad (k_spmv3_quad's layout: four lanes walk a row, 16 rows per wave and step).  A wave takes the four steps of one 64-row word in
// turn.  After quad_sum all four lanes of a quad hold the row's sums: lane q of the quad keeps those of step q, so that after the fourth
// step each of the 64 lanes holds ONE row of the word (lane L: row 16 (L & 3) + (L >> 2)) and the product a b is formed once per word with
// every lane busy, not once per step with one lane in four.  The ballot comes in that lane order; lane 0 puts it in row order and stores it.
// Measured on the compiler-like 2^20 instance (multiply_vec: 0.32 ms): 0.30 ms this way (99 VGPRs, 4 waves per SIMD); 0.335 ms with the
// product in every step (75 VGPRs) and the same with the sums handed over through LDS instead of kept in registers.
template <bool kSmall> __global__ __launch_bounds__(kBlock) void k_sat_quad(DCsr3 m, size_t rows, const Fr *x, unsigned long long *bits, unsigned long long *count) {
    const int q = threadIdx.x & 3, lane = threadIdx.x & 63;
    const size_t words = (rows + 63) >> 6, nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long mine = 0;
    for (size_t w = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6; w < words; w += nwaves) {
        Fr keep[3] = {fr_zero(), fr_zero(), fr_zero()};            // a padding or long row keeps 0, 0, 0: it passes here
#pragma unroll 1
        for (int j = 0; j < 4; j++) {
            const size_t r = (w << 6) + (size_t)(16 * j + (lane >> 2));
            Fr a[3] = {fr_zero(), fr_zero(), fr_zero()};
            if (r < rows && !row_is_heavy(m, r)) row_sums<kSmall, 4>(m, x, r, (uint32_t)q, a);
            for (int k = 0; k < 3; k++) a[k] = quad_sum(a[k]);     // every lane of the wave takes part
            if (q == j) for (int k = 0; k < 3; k++) keep[k] = a[k];
        }
        const unsigned long long v = (unsigned long long)__ballot(row_fails(keep[0], keep[1], keep[2]));
        if (lane == 0) {
            const unsigned long long word = quad_votes(v) | (quad_votes(v >> 1) << 16) | (quad_votes(v >> 2) << 32) | (quad_votes(v >> 3) << 48);
            bits[w] = word; mine += (unsigned long long)__popcll(word);
        }
    }
    if (lane == 0 && mine) atomicAdd(count, mine);
}
// the checking form of k_spmv3_heavy_combine: one workgroup per long row adds its segments' partial sums up and sets the row's bit.  Runs after
// the launch above has stored the row's word (with the bit clear), on the same stream.
__global__ __launch_bounds__(kBlock) void k_sat_heavy_check(const uint32_t *heavy, const uint32_t *seg_begin, const Fr *partial, unsigned long long *bits, unsigned long long *count) {
    Fr acc[3];
    segment_sums<3>(seg_begin, blockIdx.x, partial, 3, acc);
    if (threadIdx.x != 0 || !row_fails(acc[0], acc[1], acc[2])) return;
    const size_t r = heavy[blockIdx.x];
    atomicOr(&bits[r >> 6], 1ull << (r & 63));
    atomicAdd(count, 1ull);
}
// The report: one workgroup per listed row recomputes the three sums (a row of any length: the workgroup strides over it) and writes them
// out of Montgomery form, as canonical integers — little-endian words, i.e. the 32 canonical bytes of each.
template <bool kSmall> __global__ __launch_bounds__(kBlock) void k_sat_report(DCsr3 m, const uint32_t *row_ids, const Fr *x, Fr *out) {
    Fr acc[3];
    row_sums<kSmall, kBlock>(m, x, row_ids[blockIdx.x], threadIdx.x, acc);
    block_reduce<3>(acc);
    if (threadIdx.x == 0) for (int k = 0; k < 3; k++) out[(size_t)blockIdx.x * 3 + k] = fr_to_raw(acc[k]);
}
void dev_sat_pass(DevCtx &c, const DeviceCsrSet &m, const Fr *z, unsigned long long *bits) {
    unsigned long long *count = c.d_counts.p;
    OTTI_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long), c.stream));
    KScope ks(c, KC_SAT_CHECK);
    by_layout(m, [&](auto small, auto quad) {            // the layouts dev_spmv3 picks, for its reasons
        constexpr bool S = decltype(small)::value, Q = decltype(quad)::value;
        hipLaunchKernelGGL((Q ? k_sat_quad<S> : k_sat_light<S>), grid_for(Q ? 4 * m.rows : m.rows), kBlock, 0, c.stream, m.view(), m.rows, z, bits, count);
    });
    if (!m.n_heavy) return;
    launch_heavy_segments(c, m, z);
    hipLaunchKernelGGL(k_sat_heavy_check, (unsigned)m.n_heavy, kBlock, 0, c.stream, (const uint32_t *)m.heavy.p, (const uint32_t *)m.seg_begin.p, (const Fr *)c.spmv_partial.p, bits, count);
}
uint64_t dev_sat_count(DevCtx &c) {
    unsigned long long *h = reinterpret_cast<unsigned long long *>(&c.h_results[kSatCountSlot]);
    OTTI_HIP(hipMemcpyAsync(h, c.d_counts.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));
    return (uint64_t)*h;
}
SatReport dev_check_sat(DevCtx &c, DeviceInstance &d, const Fr *z, size_t max_rows, bool with_values) {
    const DeviceCsrSet &m = d.by_row;
    const size_t words = (m.rows + 63) >> 6;
    if (c.sat_bits.n < words) { OTTI_HIP(hipStreamSynchronize(c.stream)); c.sat_bits.alloc(words); }
    SatReport rep;
    OTTI_HIP(hipEventRecord(c.ev0, c.stream));
    dev_sat_pass(c, m, z, c.sat_bits.p);
    OTTI_HIP(hipEventRecord(c.ev1, c.stream));
    rep.n_unsat = dev_sat_count(c);
    OTTI_HIP(hipEventElapsedTime(&rep.kernel_ms, c.ev0, c.ev1));
    dev_sat_report(c, d, z, c.sat_bits.p, max_rows, with_values, false, rep);
    return rep;
}
void dev_sat_report(DevCtx &c, DeviceInstance &d, const Fr *z, const unsigned long long *d_bits, size_t max_rows, bool with_values, bool timed, SatReport &rep) {
    const DeviceCsrSet &m = d.by_row;
    const size_t words = (m.rows + 63) >> 6;
    const size_t k = (size_t)std::min<uint64_t>(rep.n_unsat, max_rows);
    if (!k) return;
    std::vector<unsigned long long> bits(words);
    OTTI_HIP(hipMemcpy(bits.data(), d_bits, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    rep.rows.reserve(k);
    for (size_t w = 0; w < words && rep.rows.size() < k; w++)
        for (unsigned long long v = bits[w]; v && rep.rows.size() < k; v &= v - 1) {
            const size_t r = (w << 6) + (size_t)__builtin_ctzll(v);
            if (r < m.rows) rep.rows.push_back((uint64_t)r);
        }
    if (!with_values) return;
    if (c.sat_rows.n < kSatReportRows) { c.sat_rows.alloc(kSatReportRows); c.sat_abc.alloc(3 * kSatReportRows); }
    rep.abc96.resize(96 * rep.rows.size());
    uint32_t ids[kSatReportRows];
    for (size_t i0 = 0; i0 < rep.rows.size(); i0 += kSatReportRows) {
        const size_t n = std::min(kSatReportRows, rep.rows.size() - i0);
        for (size_t i = 0; i < n; i++) ids[i] = (uint32_t)rep.rows[i0 + i];
        OTTI_HIP(hipMemcpyAsync(c.sat_rows.p, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
        if (timed) OTTI_HIP(hipEventRecord(c.ev0, c.stream));
        by_flag(m.use_small, [&](auto small) { hipLaunchKernelGGL(k_sat_report<decltype(small)::value>, (unsigned)n, kBlock, 0, c.stream, m.view(), (const uint32_t *)c.sat_rows.p, z, c.sat_abc.p); });
        if (timed) OTTI_HIP(hipEventRecord(c.ev1, c.stream));
        OTTI_HIP(hipMemcpyAsync(rep.abc96.data() + 96 * i0, c.sat_abc.p, 96 * n, hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipStreamSynchronize(c.stream));              // `ids` and the device buffers are reused by the next batch
        if (timed) { float ms = 0; OTTI_HIP(hipEventElapsedTime(&ms, c.ev0, c.ev1)); rep.kernel_ms += ms; }
    }
}

// ------------------------------------------------------------------------------------------------ kept products (device.h dev_products_patch)
// MARK: the by-column lists of the changed columns set their rows' bits in `touched` (zeroed by the launcher).  Column i of the launch is cols[i], or
// first + i when there is no list.  A short column goes to one lane, or to a quad where the by-column set has the quad layout (the lanes only store:
// no shuffle, so a wave needs no padding); a column longer than kHeavyRow is left to k_prod_mark_heavy, where a workgroup strides over it.
// row_sums' bit-setting form: this lane's share of column j's three lists
template <uint32_t kLanes> __device__ __forceinline__ void mark_rows(const DCsr3 &m, size_t j, uint32_t q, unsigned long long *touched) {
    for (int k = 0; k < 3; k++)
        for_entries(m, k, j, q, kLanes, kWholeList, [&](uint32_t p) { const uint32_t r = m.idx[k][p]; atomicOr(&touched[r >> 6], 1ull << (r & 63)); });
}
template <bool kQuad> __global__ __launch_bounds__(kBlock) void k_prod_mark(DCsr3 m, const uint64_t *cols, size_t first, size_t n, unsigned long long *touched) {
    constexpr uint32_t kLanes = kQuad ? 4 : 1;
    const uint32_t q = kQuad ? (threadIdx.x & 3) : 0;
    for (size_t i = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) / kLanes; i < n; i += ((size_t)gridDim.x * blockDim.x) / kLanes) {
        const size_t j = cols ? (size_t)cols[i] : first + i;
        if (!row_is_heavy(m, j)) mark_rows<kLanes>(m, j, q, touched);
    }
}
__global__ __launch_bounds__(kBlock) void k_prod_mark_heavy(DCsr3 m, const uint64_t *cols, size_t first, size_t n, unsigned long long *touched) {
    for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
        const size_t j = cols ? (size_t)cols[i] : first + i;
        if (row_is_heavy(m, j)) mark_rows<kBlock>(m, j, threadIdx.x, touched);
    }
}
// COMPACT: a popcount per word, scanned in place (scan_inplace: inclusive), then every word writes its rows behind those of the words before it
__global__ __launch_bounds__(kBlock) void k_prod_popc(const unsigned long long *touched, size_t words, uint32_t *cnt) {
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x) cnt[w] = (uint32_t)__popcll(touched[w]);
}
__global__ __launch_bounds__(kBlock) void k_prod_emit(const unsigned long long *touched, const uint32_t *cnt, size_t words, uint32_t *rows) {
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x) {
        unsigned long long v = touched[w];
        uint32_t o = cnt[w] - (uint32_t)__popcll(v);
        for (; v; v &= v - 1) rows[o++] = (uint32_t)(w << 6) + (uint32_t)__ffsll((long long)v) - 1u;
    }
}
// RECOMPUTE.  One row's three sums stored, its verdict bit set or cleared; returns the change of the failing count (-1, 0, 1).  Each row is listed
// once, so no other lane writes this bit: the plain load sees it, and the word is only touched (atomically: its other bits have other writers) when
// the verdict has moved.
__device__ __forceinline__ int prod_store_row(size_t r, const Fr &a, const Fr &b, const Fr &cc, Fr *Az, Fr *Bz, Fr *Cz, unsigned long long *bits) {
    Az[r] = a; Bz[r] = b; Cz[r] = cc;
    const unsigned long long bit = 1ull << (r & 63);
    const bool fail = row_fails(a, b, cc), was = (bits[r >> 6] & bit) != 0;
    if (fail != was) atomicXor(&bits[r >> 6], bit);
    return (int)fail - (int)was;
}
__device__ __forceinline__ void prod_count_move(int mine, unsigned long long *count) {
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, (unsigned long long)(long long)mine);      // two's complement: a negative move wraps the 64-bit tally down
}
// listed rows up to kHeavyRow entries: a row per lane, or per quad in the by-row set's quad layout (k_spmv3_quad's walk and quad_sum; the list is
// padded to whole waves so that every lane takes part in the shuffles).  The order of summation is free: every partial sum is the canonical word
// (comment above row_fails), so the stored words are those k_spmv3_* store.
template <bool kSmall, bool kQuad> __global__ __launch_bounds__(kBlock) void k_prod_rows(DCsr3 m, const uint32_t *rows, size_t n, const Fr *x, Fr *Az, Fr *Bz, Fr *Cz,
                                                                                         unsigned long long *bits, unsigned long long *count) {
    constexpr uint32_t kLanes = kQuad ? 4 : 1;
    constexpr size_t kPerWave = 64 / kLanes;
    const uint32_t q = kQuad ? (threadIdx.x & 3) : 0;
    const size_t padded = (n + kPerWave - 1) & ~(kPerWave - 1);
    int mine = 0;
    for (size_t i = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) / kLanes; i < padded; i += ((size_t)gridDim.x * blockDim.x) / kLanes) {
        const size_t r = i < n ? (size_t)rows[i] : 0;
        const bool live = i < n && !row_is_heavy(m, r);
        Fr a[3] = {fr_zero(), fr_zero(), fr_zero()};
        if (live) row_sums<kSmall, kLanes>(m, x, r, q, a);
        if (kQuad) for (int k = 0; k < 3; k++) a[k] = quad_sum(a[k]);
        if (live && q == 0) mine += prod_store_row(r, a[0], a[1], a[2], Az, Bz, Cz, bits);
    }
    prod_count_move(mine, count);
}
// the longer ones: a workgroup per row strides over it, as k_sat_report does (launched behind the kernel above, and only for an instance that has such rows)
template <bool kSmall> __global__ __launch_bounds__(kBlock) void k_prod_rows_heavy(DCsr3 m, const uint32_t *rows, size_t n, const Fr *x, Fr *Az, Fr *Bz, Fr *Cz,
                                                                                   unsigned long long *bits, unsigned long long *count) {
    for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
        const size_t r = rows[i];
        if (!row_is_heavy(m, r)) continue;                          // (the same for every thread of the workgroup)
        Fr acc[3];
        row_sums<kSmall, kBlock>(m, x, r, threadIdx.x, acc);
        block_reduce<3>(acc);
        if (threadIdx.x == 0) { const int d = prod_store_row(r, acc[0], acc[1], acc[2], Az, Bz, Cz, bits); if (d) atomicAdd(count, (unsigned long long)(long long)d); }
    }
}
// the full pass's second half: every verdict from the vectors dev_spmv3 has just written (k_sat_light's bitmap writes: a wave owns whole words)
__global__ __launch_bounds__(kBlock) void k_prod_verdicts(const Fr *Az, const Fr *Bz, const Fr *Cz, size_t rows, unsigned long long *bits, unsigned long long *count) {
    unsigned long long mine = 0;
    const size_t padded = (rows + 63) & ~(size_t)63;
    for (size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x; r < padded; r += (size_t)gridDim.x * blockDim.x) {
        const bool fail = r < rows && row_fails(Az[r], Bz[r], Cz[r]);
        const unsigned long long word = (unsigned long long)__ballot(fail);
        if ((threadIdx.x & 63) == 0) { bits[r >> 6] = word; mine += (unsigned long long)__popcll(word); }
    }
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}
double products_full_share() {
    if (const char *e = getenv("OTTI_PRODUCTS_FULL_SHARE")) { char *end = nullptr; const double v = strtod(e, &end); if (end != e && v >= 0) return v; }
    return kProductsFullShare;
}
void dev_products_full(DevCtx &c, const DeviceInstance &d, const Fr *z, Fr *Az, Fr *Bz, Fr *Cz, unsigned long long *bits, unsigned long long *d_unsat) {
    const DeviceCsrSet &m = d.by_row;
    dev_spmv3(c, m, z, Az, Bz, Cz, false, nullptr);
    OTTI_HIP(hipMemsetAsync(d_unsat, 0, sizeof(unsigned long long), c.stream));
    KScope ks(c, KC_SPMV);
    hipLaunchKernelGGL(k_prod_verdicts, grid_for(m.rows), kBlock, 0, c.stream, (const Fr *)Az, (const Fr *)Bz, (const Fr *)Cz, m.rows, bits, d_unsat);
}
ProductsPatch dev_products_patch(DevCtx &c, const DeviceInstance &d, const Fr *z, const uint64_t *d_cols, size_t ncols, size_t first, size_t count,
                                 Fr *Az, Fr *Bz, Fr *Cz, unsigned long long *bits, unsigned long long *d_unsat) {
    const DeviceCsrSet &bc = d.by_col, &br = d.by_row;
    const size_t N = br.rows, words = (N + 63) >> 6, n = d_cols ? ncols : count;
    if (n > bc.rows || (!d_cols && first > bc.rows - n)) throw Error(OTTI_ERR_BAD_ARG, "products patch: the changed columns end beyond the instance's");
    if (c.prod_touched.n < words || c.prod_rows.n < N) {
        OTTI_HIP(hipStreamSynchronize(c.stream));
        c.prod_touched.alloc(words); c.prod_cnt.alloc(words); c.prod_rows.alloc(N);
    }
    ProductsPatch out;
    unsigned long long *touched = c.prod_touched.p;
    volatile uint32_t *h_touched = reinterpret_cast<volatile uint32_t *>(&c.h_results[kProdCountSlot]);
    volatile unsigned long long *h_unsat = reinterpret_cast<volatile unsigned long long *>(&c.h_results[kProdCountSlot + 1]);
    OTTI_HIP(hipEventRecord(c.ev0, c.stream));                      // kernel_ms: from here to the last launch, the host's look at the count included
    {
        KScope ks(c, KC_SPMV);
        OTTI_HIP(hipMemsetAsync(touched, 0, words * sizeof(unsigned long long), c.stream));
        if (n) {
            by_flag(bc.quad(), [&](auto quad) {
                constexpr bool Q = decltype(quad)::value;
                hipLaunchKernelGGL(k_prod_mark<Q>, grid_for(Q ? 4 * n : n), kBlock, 0, c.stream, bc.view(), d_cols, first, n, touched);
            });
            if (bc.n_heavy) hipLaunchKernelGGL(k_prod_mark_heavy, (unsigned)std::min<size_t>(n, kMaxBlocks), kBlock, 0, c.stream, bc.view(), d_cols, first, n, touched);
        }
        hipLaunchKernelGGL(k_prod_popc, grid_for(words), kBlock, 0, c.stream, (const unsigned long long *)touched, words, c.prod_cnt.p);
        scan_inplace(c, c.prod_cnt.p, words, c.prod_scan);
        hipLaunchKernelGGL(k_prod_emit, grid_for(words), kBlock, 0, c.stream, (const unsigned long long *)touched, (const uint32_t *)c.prod_cnt.p, words, c.prod_rows.p);
    }
    OTTI_HIP(hipMemcpyAsync((void *)h_touched, c.prod_cnt.p + (words - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));
    out.n_touched = (size_t)*h_touched;
    const double share = products_full_share();
    out.full = share < 1.0 && (double)out.n_touched >= share * (double)N;
    if (out.full) dev_products_full(c, d, z, Az, Bz, Cz, bits, d_unsat);
    else if (out.n_touched) {
        KScope ks(c, KC_SPMV);
        const size_t nt = out.n_touched; const uint32_t *rows = c.prod_rows.p;
        by_layout(br, [&](auto small, auto quad) {                  // the layouts dev_spmv3 picks, for its reasons
            constexpr bool S = decltype(small)::value, Q = decltype(quad)::value;
            hipLaunchKernelGGL((k_prod_rows<S, Q>), grid_for(Q ? 4 * nt : nt), kBlock, 0, c.stream, br.view(), rows, nt, z, Az, Bz, Cz, bits, d_unsat);
        });
        if (br.n_heavy) by_flag(br.use_small, [&](auto small) {
            hipLaunchKernelGGL(k_prod_rows_heavy<decltype(small)::value>, (unsigned)std::min<size_t>(nt, kMaxBlocks), kBlock, 0, c.stream, br.view(), rows, nt, z, Az, Bz, Cz, bits, d_unsat);
        });
    }
    OTTI_HIP(hipEventRecord(c.ev1, c.stream));
    OTTI_HIP(hipMemcpyAsync((void *)h_unsat, d_unsat, sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));
    OTTI_HIP(hipEventElapsedTime(&out.kernel_ms, c.ev0, c.ev1));
    out.n_unsat = (uint64_t)*h_unsat;
    return out;
}

// ------------------------------------------------------------------------------------------------ CSR copies, built on the device
// The host keeps the matrices as entry lists in caller order (upstream's Vec<SparseMatEntry>); the two access paths the kernels want
// (by row for multiply_vec, by column for compute_eval_table_sparse) are counting sorts made here from ONE upload of the lists:
// count per major index (atomics), exclusive scan -> ptr, scatter through per-row cursors.  The order of the entries inside a row
// depends on the scatter's arrival order; every consumer adds the row's products in GF(l), where the sum does not depend on it.
__global__ __launch_bounds__(kBlock) void k_csr_count(const uint32_t *major, size_t n, uint32_t *ptr) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) atomicAdd(&ptr[major[i] + 1], 1u);
}
__global__ __launch_bounds__(kBlock) void k_csr_fill(const uint32_t *major, const uint32_t *minor, const Fr *val, const int32_t *code, size_t n, uint32_t *cursor,
                                                     uint32_t *idx, Fr *out, int32_t *out_code) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t p = atomicAdd(&cursor[major[i]], 1u);
        idx[p] = minor[i]; out[p] = val[i];
        if (out_code) out_code[p] = code[i];
    }
}
// the small-integer codes of an entry list (fr_small_code) and how many of them there are
__global__ __launch_bounds__(kBlock) void k_coef_codes(const Fr *val, size_t n, int32_t *code, unsigned long long *n_small) {
    unsigned mine = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { const int32_t c = fr_small_code(val[i]); code[i] = c; mine += c != kNotSmall; }
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor((int)mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_small, (unsigned long long)mine);
}
// (the in-place inclusive scan of u32 counts, scan_inplace, lives in kernels_common.h: the SNARK address sort uses it as well)
// rows whose longest list (over the three matrices) exceeds kHeavyRow
__global__ __launch_bounds__(kBlock) void k_csr_count_heavy(const uint32_t *p0, const uint32_t *p1, const uint32_t *p2, size_t rows, unsigned *count) {
    for (size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x; r < rows; r += (size_t)gridDim.x * blockDim.x)
        if (len_is_heavy(max(p0[r + 1] - p0[r], max(p1[r + 1] - p1[r], p2[r + 1] - p2[r])))) atomicAdd(count, 1u);
}
static void upload_coo(DevCtx &c, DeviceCoo &d, const std::vector<uint32_t> &row, const std::vector<uint32_t> &col, const std::vector<Fr> &val) {
    d.n = val.size();
    d.row.alloc(std::max<size_t>(1, d.n)); d.col.alloc(std::max<size_t>(1, d.n)); d.val.alloc(std::max<size_t>(1, d.n));
    if (!d.n) return;
    OTTI_HIP(hipMemcpyAsync(d.row.p, row.data(), d.n * 4, hipMemcpyHostToDevice, c.stream));
    OTTI_HIP(hipMemcpyAsync(d.col.p, col.data(), d.n * 4, hipMemcpyHostToDevice, c.stream));
    OTTI_HIP(hipMemcpyAsync(d.val.p, val.data(), d.n * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
}
// decide once per instance whether the kernels read coefficient codes: worth it when most entries are small integers
bool classify_coefficients(DevCtx &c, DeviceCoo coo[3]) {
    DevBuf<unsigned long long> count(1); unsigned long long n_small = 0; size_t total = 0;
    OTTI_HIP(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), c.stream));
    for (int k = 0; k < 3; k++) {
        total += coo[k].n;
        coo[k].code.alloc(std::max<size_t>(1, coo[k].n));
        if (coo[k].n) hipLaunchKernelGGL(k_coef_codes, grid_for(coo[k].n), kBlock, 0, c.stream, (const Fr *)coo[k].val.p, coo[k].n, coo[k].code.p, count.p);
    }
    OTTI_HIP(hipMemcpyAsync(&n_small, count.p, sizeof n_small, hipMemcpyDeviceToHost, c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));
    return total >= 1024 && 2 * n_small >= total;
}
void build_csr_set(DevCtx &c, DeviceCsrSet &d, const DeviceCoo coo[3], bool by_col, size_t rows, bool use_small) {
    if (rows + 1 > ((size_t)1 << 31)) throw Error(OTTI_ERR_BAD_ARG, "instance too large for 32-bit indices");
    d.rows = rows; d.use_small = use_small;
    d.avg_row = rows ? (double)(coo[0].n + coo[1].n + coo[2].n) / (3.0 * (double)rows) : 0.0;
    DevBuf<uint32_t> cursor(rows);
    std::vector<DevBuf<uint32_t>> scan_levels; scan_levels.reserve(4);
    for (int k = 0; k < 3; k++) {
        const DeviceCoo &m = coo[k];
        const uint32_t *major = by_col ? m.col.p : m.row.p, *minor = by_col ? m.row.p : m.col.p;
        d.ptr[k].alloc(rows + 1); d.idx[k].alloc(std::max<size_t>(1, m.n)); d.val[k].alloc(std::max<size_t>(1, m.n));
        if (use_small) d.small[k].alloc(std::max<size_t>(1, m.n));
        OTTI_HIP(hipMemsetAsync(d.ptr[k].p, 0, (rows + 1) * 4, c.stream));
        if (m.n) hipLaunchKernelGGL(k_csr_count, grid_for(m.n), kBlock, 0, c.stream, major, m.n, d.ptr[k].p);
        scan_inplace(c, d.ptr[k].p, rows + 1, scan_levels);   // ptr[0] = 0: the inclusive sum over [0, rows] is the exclusive one shifted
        if (m.n) {
            OTTI_HIP(hipMemcpyAsync(cursor.p, d.ptr[k].p, rows * 4, hipMemcpyDeviceToDevice, c.stream));
            hipLaunchKernelGGL(k_csr_fill, grid_for(m.n), kBlock, 0, c.stream, major, minor, (const Fr *)m.val.p, (const int32_t *)m.code.p, m.n, cursor.p, d.idx[k].p, d.val[k].p,
                               use_small ? d.small[k].p : (int32_t *)nullptr);
        }
    }
    // long lists: found on the device; only when there are any do the row pointers come back for the segment lists
    DevBuf<unsigned> n_heavy_dev(1); unsigned n_heavy = 0;
    OTTI_HIP(hipMemsetAsync(n_heavy_dev.p, 0, sizeof(unsigned), c.stream));
    hipLaunchKernelGGL(k_csr_count_heavy, grid_for(rows), kBlock, 0, c.stream, (const uint32_t *)d.ptr[0].p, (const uint32_t *)d.ptr[1].p, (const uint32_t *)d.ptr[2].p, rows, n_heavy_dev.p);
    OTTI_HIP(hipMemcpyAsync(&n_heavy, n_heavy_dev.p, sizeof(unsigned), hipMemcpyDeviceToHost, c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));                 // also: cursor / scan scratch / the entry lists may go out of scope after this
    d.n_heavy = 0; d.n_seg = 0;
    if (!n_heavy) return;
    std::vector<uint32_t> ptr[3], heavy, seg_row, seg_no, seg_begin;
    for (int k = 0; k < 3; k++) { ptr[k].resize(rows + 1); OTTI_HIP(hipMemcpy(ptr[k].data(), d.ptr[k].p, (rows + 1) * 4, hipMemcpyDeviceToHost)); }
    for (size_t r = 0; r < rows; r++) {
        uint32_t mx = 0;
        for (int k = 0; k < 3; k++) mx = std::max(mx, ptr[k][r + 1] - ptr[k][r]);
        if (len_is_heavy(mx)) {
            heavy.push_back((uint32_t)r); seg_begin.push_back((uint32_t)seg_row.size());
            for (uint32_t sn = 0; sn * kHeavySeg < mx; sn++) { seg_row.push_back((uint32_t)r); seg_no.push_back(sn); }
        }
    }
    seg_begin.push_back((uint32_t)seg_row.size());
    d.n_heavy = heavy.size(); d.n_seg = seg_row.size();
    auto up = [](DevBuf<uint32_t> &b, const std::vector<uint32_t> &v) { b.alloc(v.size()); OTTI_HIP(hipMemcpy(b.p, v.data(), v.size() * 4, hipMemcpyHostToDevice)); };
    up(d.heavy, heavy); up(d.seg_row, seg_row); up(d.seg_no, seg_no); up(d.seg_begin, seg_begin);
}
std::shared_ptr<DeviceInstance> upload_instance(const Instance &I) {
    DevCtx &c = DevCtx::get();
    auto d = std::make_shared<DeviceInstance>();
    DeviceCoo coo[3];
    for (int k = 0; k < 3; k++) upload_coo(c, coo[k], I.mat(k).row, I.mat(k).col, I.mat(k).val);
    const bool use_small = classify_coefficients(c, coo);
    build_csr_set(c, d->by_row, coo, false, I.num_cons, use_small);
    build_csr_set(c, d->by_col, coo, true, 2 * I.num_vars, use_small);
    d->nnz = I.nnz[0] + I.nnz[1] + I.nnz[2];
    return d;
}

// ------------------------------------------------------------------------------------------------ a rank's share of an entry list that is in HBM
// A stable stream compaction: FLAG the entries whose key (row, or column) is k mod g, scan_inplace the flags, SCATTER every flagged entry to its
// scanned position with the key renumbered key / g.  g is a power of two: mask and shift.  File order is kept, as the host loop keeps it.  The
// count comes back with one copy behind the scan, the outputs are allocated to it, and the scatter's positions (1 .. count, less one) lie inside
// them whatever the lists hold.  A streaming pass of about 100 bytes per entry that stays.
__global__ __launch_bounds__(kBlock) void k_shard_flag(const uint32_t *key, size_t n, uint32_t mask, uint32_t k, uint32_t *flag) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) flag[i] = (key[i] & mask) == k ? 1u : 0u;
}
__global__ __launch_bounds__(kBlock) void k_shard_scatter(const uint32_t *row, const uint32_t *col, const Fr *val, size_t n, uint32_t mask, uint32_t k, int shift, int by_col,
                                                          const uint32_t *incl, uint32_t *out_row, uint32_t *out_col, Fr *out_val) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t r = row[i], cl = col[i];
        if (((by_col ? cl : r) & mask) != k) continue;
        const uint32_t p = incl[i] - 1u;                      // this entry's own flag is in the sum: at least 1
        out_row[p] = by_col ? r : r >> shift; out_col[p] = by_col ? cl >> shift : cl; out_val[p] = val[i];
    }
}
void dev_shard_filter(DevCtx &c, const uint32_t *row, const uint32_t *col, const Fr *val, size_t n, int world, int rank, bool by_col, DeviceCoo &out,
                      DevBuf<uint32_t> &flags, std::vector<DevBuf<uint32_t>> &scan_levels) {
    if (world < 1 || (world & (world - 1)) || rank < 0 || rank >= world || n >= ((size_t)1 << 32)) throw Error(OTTI_ERR_BAD_ARG, "shard filter: world must be a power of two above the rank, the list below 2^32 entries");
    const uint32_t mask = (uint32_t)world - 1u, k = (uint32_t)rank; const int shift = (int)ilog2((size_t)world);
    uint32_t count = 0;
    if (n) {
        if (flags.n < n) { OTTI_HIP(hipStreamSynchronize(c.stream)); flags.alloc(n); }
        hipLaunchKernelGGL(k_shard_flag, grid_for(n), kBlock, 0, c.stream, by_col ? col : row, n, mask, k, flags.p);
        scan_inplace(c, flags.p, n, scan_levels);
        OTTI_HIP(hipMemcpyAsync(&count, flags.p + (n - 1), 4, hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipStreamSynchronize(c.stream));
    }
    out.n = count;                                            // an empty selection: n = 0 with one-element buffers, as upload_coo leaves an empty list
    out.row.alloc(std::max<size_t>(1, out.n)); out.col.alloc(std::max<size_t>(1, out.n)); out.val.alloc(std::max<size_t>(1, out.n));
    if (count) hipLaunchKernelGGL(k_shard_scatter, grid_for(n), kBlock, 0, c.stream, row, col, val, n, mask, k, shift, by_col ? 1 : 0, (const uint32_t *)flags.p, out.row.p, out.col.p, out.val.p);
}

std::shared_ptr<DeviceShard> upload_instance_shard(const Instance &I, int rank, int world) {
    DevCtx &c = DevCtx::get();
    if (world < 1 || (world & (world - 1)) || rank < 0 || rank >= world || (size_t)world > I.num_cons || (size_t)world > 2 * I.num_vars)
        throw Error(OTTI_ERR_BAD_ARG, "shard: world must be a power of two not larger than the instance");
    auto d = std::make_shared<DeviceShard>();
    d->rank = rank; d->world = world;
    const uint32_t g = (uint32_t)world, k = (uint32_t)rank;
    // rows r = k (mod g) renumbered r / g, columns untouched; and the entries of columns c = k (mod g) renumbered c / g, rows untouched
    DeviceCoo rows[3], cols[3];
    // an instance ingested on the device keeps its entry lists in HBM (DeviceInstance::ent): its share is filtered there, and mat() is never asked
    const std::shared_ptr<DeviceInstance> di = I.ingested_on_device ? I.dev : nullptr;
    bool resident = di != nullptr;
    for (int m = 0; m < 3 && resident; m++) resident = di->ent[m].n == I.nnz[m];
    if (resident) {
        DevBuf<uint32_t> flags; std::vector<DevBuf<uint32_t>> scan_levels; scan_levels.reserve(4);
        for (int m = 0; m < 3; m++) {
            const DeviceCoo &e = di->ent[m];
            dev_shard_filter(c, e.row.p, e.col.p, e.val.p, e.n, world, rank, false, rows[m], flags, scan_levels);
            dev_shard_filter(c, e.row.p, e.col.p, e.val.p, e.n, world, rank, true, cols[m], flags, scan_levels);
        }
        OTTI_HIP(hipStreamSynchronize(c.stream));             // the flags and the scan's scratch go out of scope
    } else for (int m = 0; m < 3; m++) {                      // host lists: the filter as a loop over them, the shares uploaded
        const SparseMat &M = I.mat(m);
        std::vector<uint32_t> rr, rc, cr, cc; std::vector<Fr> rv, cv;
        for (size_t e = 0; e < M.val.size(); e++) {
            if (M.row[e] % g == k) { rr.push_back(M.row[e] / g); rc.push_back(M.col[e]); rv.push_back(M.val[e]); }
            if (M.col[e] % g == k) { cr.push_back(M.row[e]); cc.push_back(M.col[e] / g); cv.push_back(M.val[e]); }
        }
        upload_coo(c, rows[m], rr, rc, rv); upload_coo(c, cols[m], cr, cc, cv);
        OTTI_HIP(hipStreamSynchronize(c.stream));             // the host lists above go out of scope
    }
    const bool small_rows = classify_coefficients(c, rows), small_cols = classify_coefficients(c, cols);
    build_csr_set(c, d->by_row, rows, false, I.num_cons / g, small_rows);
    build_csr_set(c, d->by_col, cols, true, 2 * I.num_vars / g, small_cols);
    return d;
}

}  // namespace otti
