// Kernels of SNARK mode's R1CSEvalProof (snark.h): dereferencing the eq tables by row / column address, the memory-checking hash
// layer, product-circuit layers, and the rounds of the batched cubic sum-check over many (A, B, C) table triples at once.
// All HBM-streaming work on 32-byte field elements (no MFMA applies: 256-bit modular integers); one launch handles every instance of a
// batch (grid.y = instance), so a round of SumcheckInstanceProof::prove_cubic_batched is one launch whatever the batch size.
//
// Kernel <-> upstream loop [RECALL; the reference's Spartan/ submodule is empty]:
//   k_at_*                  sparse_mlpoly.rs AddrTimestamps::new (read_ts, audit_ts: a stable radix sort by address)
//   k_gather                sparse_mlpoly.rs AddrTimestamps::deref_mem
//   k_hash_mem / k_hash_ops sparse_mlpoly.rs Layers::build_hash_layer (init / audit, read / write)
//   k_prod_layer            product_tree.rs ProductCircuit::compute_layer
//   k_pc_round              sumcheck.rs SumcheckInstanceProof::prove_cubic_batched: one round = bound_poly_var_top of every table of the
//                           batch by the previous challenge + the evaluation loop (comb = A * B * C at 0, 2, 3), fused
//   k_pc_export             the tables' last elements (and the host-played tail of every layer)
//   k_dot_many / k_sum3     DensePolynomial::evaluate (against a shared eq table) / DotProductCircuit::evaluate
#include "kernels_common.h"
#include "snark_dev.h"

namespace otti {

__global__ __launch_bounds__(kBlock) void k_gather(const Fr *table, const uint32_t *idx, Fr *out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = table[idx[i]];
}
void dev_gather(DevCtx &c, const Fr *table, const uint32_t *idx, Fr *out, size_t n) {
    KScope ks(c, KC_GATHER);
    hipLaunchKernelGGL(k_gather, grid_for(n), kBlock, 0, c.stream, table, idx, out, n);
}

// addresses and timestamps of the dense representation: small integers -> Montgomery form
__global__ __launch_bounds__(kBlock) void k_u32_to_fr(const uint32_t *in, Fr *out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = fr_from_u64((uint64_t)in[i]);
}
void dev_u32_to_fr(DevCtx &c, const uint32_t *in, Fr *out, size_t n) {
    if (n) hipLaunchKernelGGL(k_u32_to_fr, grid_for(n), kBlock, 0, c.stream, in, out, n);
}

// The decommitment's addresses and values straight from entry lists that are in HBM already (a device ingest keeps them: device.h DeviceInstance::ent),
// one launch for the matrices of f (grid.y): position i < nv is entry i, nv <= i < len the explicit padding upstream writes below two constraints
// (row i, column pad_col, value zero), the rest address 0 and value zero.  Every element of the five outputs is written: nothing is zeroed beforehand.
// A streaming pass: 40 bytes read per entry, 104 written per position, the 32-byte elements as two 16-byte accesses (Fr is 16-byte aligned).
__global__ __launch_bounds__(kBlock) void k_decomm_fill(DecommFill f, size_t N) {
    const DecommFillMat m = f.m[blockIdx.y];
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < N; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t r = 0, cl = 0; Fr v = fr_zero();
        if (i < m.nv) { r = m.row[i]; cl = m.col[i]; v = m.val[i]; }
        else if (i < m.len) { r = (uint32_t)i; cl = m.pad_col; }
        m.row_addr[i] = r; m.col_addr[i] = cl;
        m.row_fr[i] = r ? fr_from_u64((uint64_t)r) : fr_zero();
        m.col_fr[i] = cl ? fr_from_u64((uint64_t)cl) : fr_zero();
        m.val_fr[i] = v;
    }
}
void dev_decomm_fill(DevCtx &c, const DecommFill &f, int count, size_t N) {
    if (count < 1 || count > 3 || !N) throw Error(OTTI_ERR_INTERNAL, "decommitment fill: one to three matrices, at least one position");
    for (int k = 0; k < count; k++) if (f.m[k].nv > f.m[k].len || f.m[k].len > N) throw Error(OTTI_ERR_INTERNAL, "decommitment fill: lengths out of order");
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((N + kBlock - 1) / kBlock, (size_t)kMaxBlocks / (size_t)count));   // never a zero grid
    hipLaunchKernelGGL(k_decomm_fill, dim3(gx, (unsigned)count), kBlock, 0, c.stream, f, N);
}

// ------------------------------------------------------------------------------------------------ timestamps of the dense representation
// sparse_mlpoly.rs AddrTimestamps::new on the device (snark_dev.h AddrTs): read_ts of an entry = how many entries with the same address come
// before it in the walk over the three lists, audit_ts = how many there are.  A stable LSD radix sort (8-bit digits) of the entries' walk
// positions by address makes equal addresses contiguous and keeps the walk order inside them: rank = sorted position - first position of the
// address.  Every step is a pure function of the lists (the only atomics are a workgroup's LDS digit counts, which commute), so the numbers
// are the sequential scan's whatever the geometry, and the work is linear in the number of entries whatever their distribution.
// Only the entries below len[k] are sorted; the padding behind them (address 0) is ranked in closed form (k_at_tail).
constexpr int kAtItems = 8, kAtTile = kBlock * kAtItems;      // entries of one workgroup's tile: rounds j of kBlock consecutive entries
struct AtLens { uint32_t off[4], pad_before[4]; };            // off[k]: walk position of matrix k's first sorted entry, off[3] = their number; pad_before[k]: padding entries of the matrices before k, [3] = all
__device__ __forceinline__ int at_matrix(const AtLens &l, uint32_t g) { return g >= l.off[2] ? 2 : g >= l.off[1] ? 1 : 0; }

__global__ __launch_bounds__(kBlock) void k_at_pack(AddrTs a, AtLens l, uint32_t *keys) {
    const int side = blockIdx.y; const uint32_t L = l.off[3];
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < L; g += (size_t)gridDim.x * blockDim.x) {
        const int k = at_matrix(l, (uint32_t)g);
        keys[(size_t)side * L + g] = a.addr[side][k][g - l.off[k]];
    }
}
// digit counts of every tile: hist[(side * 256 + digit) * nwg + tile] — scanned in this order, a tile's first output position per digit
__global__ __launch_bounds__(kBlock) void k_at_hist(const uint32_t *keys, uint32_t L, int shift, uint32_t *hist, uint32_t nwg) {
    __shared__ uint32_t s_h[256];
    const int side = blockIdx.y; const uint32_t *k = keys + (size_t)side * L;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    for (int j = 0; j < kAtItems; j++) {
        const size_t e = (size_t)blockIdx.x * kAtTile + (size_t)j * kBlock + threadIdx.x;
        if (e < L) atomicAdd(&s_h[(k[e] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[((size_t)side * 256 + threadIdx.x) * nwg + blockIdx.x] = s_h[threadIdx.x];
}
// one stable pass: inside a tile the order is round, wave, lane.  Per round a wave finds, by eight ballots, the lanes that hold the same
// digit (rank inside the wave = how many of them are below this lane); thread d then turns the waves' counts of digit d into their first positions.
// kFirst: the entries still sit at their walk positions (no index array yet)
template <bool kFirst> __global__ __launch_bounds__(kBlock) void k_at_scatter(const uint32_t *key_in, const uint32_t *idx_in, uint32_t *key_out, uint32_t *idx_out, uint32_t L, int shift,
                                                                              const uint32_t *hist_scanned, uint32_t nwg) {
    __shared__ uint32_t s_cnt[256], s_wave[kBlock / 64][256];
    const int side = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    key_in += (size_t)side * L; key_out += (size_t)side * L; idx_out += (size_t)side * L;
    if (!kFirst) idx_in += (size_t)side * L;
    const size_t h = ((size_t)side * 256 + threadIdx.x) * nwg + blockIdx.x;
    s_cnt[threadIdx.x] = (h ? hist_scanned[h - 1] : 0u) - (uint32_t)side * L;      // (the scan runs over both sides: side 1 starts at L)
    for (int j = 0; j < kAtItems; j++) {
        const size_t e = (size_t)blockIdx.x * kAtTile + (size_t)j * kBlock + threadIdx.x;
        const bool valid = e < L;
        const uint32_t key = valid ? key_in[e] : 0u, d = (key >> shift) & 255u;
        for (int i = lane; i < 256; i += 64) s_wave[wave][i] = 0;
        __syncthreads();
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) { const unsigned long long bal = __ballot((d >> b) & 1u); same &= ((d >> b) & 1u) ? bal : ~bal; }
        const uint32_t below = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && below == 0) s_wave[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        { uint32_t run = s_cnt[threadIdx.x]; for (int w = 0; w < kBlock / 64; w++) { const uint32_t t = s_wave[w][threadIdx.x]; s_wave[w][threadIdx.x] = run; run += t; } s_cnt[threadIdx.x] = run; }
        __syncthreads();
        if (valid) { const uint32_t pos = s_wave[wave][d] + below; key_out[pos] = key; idx_out[pos] = kFirst ? (uint32_t)e : idx_in[e]; }
        __syncthreads();
    }
}
// start[address] = sorted position of its first entry (written for the addresses that occur, read for those alone)
__global__ __launch_bounds__(kBlock) void k_at_heads(const uint32_t *keys, uint32_t L, uint32_t *start, size_t M) {
    const int side = blockIdx.y; const uint32_t *k = keys + (size_t)side * L;
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < L; p += (size_t)gridDim.x * blockDim.x)
        if (p == 0 || k[p - 1] != k[p]) start[(size_t)side * M + k[p]] = (uint32_t)p;
}
// the outputs (u32 and / or Montgomery form); the audit arrays were zeroed before.  Address 0 also holds the padding: an entry there comes
// after the padding of the matrices before its own
__global__ __launch_bounds__(kBlock) void k_at_ranks(AddrTs a, AtLens l, const uint32_t *keys, const uint32_t *idx, const uint32_t *start) {
    const int side = blockIdx.y; const uint32_t L = l.off[3];
    keys += (size_t)side * L; idx += (size_t)side * L; start += (size_t)side * a.M;
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < L; p += (size_t)gridDim.x * blockDim.x) {
        const uint32_t key = keys[p], g = idx[p], in_seg = (uint32_t)p - start[key];
        const int k = at_matrix(l, g); const uint32_t i = g - l.off[k];
        const uint32_t ts = in_seg + (key == 0 ? l.pad_before[k] : 0u);
        if (a.ts_u32[side][k]) a.ts_u32[side][k][i] = ts;
        if (a.ts_fr[side][k]) a.ts_fr[side][k][i] = fr_from_u64((uint64_t)ts);
        if (p + 1 == L || keys[p + 1] != key) {              // the last entry of its address (address 0 with padding: k_at_tail writes the total)
            if (a.audit_u32[side]) a.audit_u32[side][key] = in_seg + 1;
            if (a.audit_fr[side]) a.audit_fr[side][key] = fr_from_u64((uint64_t)in_seg + 1);
        }
    }
}
// zc[side][k] = sorted entries at address 0 in matrices 0 .. k, zc[side][3] = all of them: address 0 sorts first and its entries keep the walk
// order, so these are binary searches in the sorted arrays
__global__ void k_at_zero(AtLens l, const uint32_t *keys, const uint32_t *idx, uint32_t *zc) {
    const int side = blockIdx.x; const uint32_t L = l.off[3];
    if (threadIdx.x != 0) return;
    keys += (size_t)side * L; idx += (size_t)side * L;
    uint32_t lo = 0, hi = L;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (keys[mid] == 0) lo = mid + 1; else hi = mid; }
    const uint32_t n0 = lo;
    for (int k = 0; k < 3; k++) {
        lo = 0; hi = n0;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (idx[mid] < l.off[k + 1]) lo = mid + 1; else hi = mid; }
        zc[4 * side + k] = lo;
    }
    zc[4 * side + 3] = n0;
}
// the padding: entry q of all padding entries in walk order (matrix k, index len[k] + q - pad_before[k]) has seen the sorted entries at
// address 0 of matrices 0 .. k and the q padding entries before it
__global__ __launch_bounds__(kBlock) void k_at_tail(AddrTs a, AtLens l, const uint32_t *zc) {
    const int side = blockIdx.y; const uint32_t P = l.pad_before[3];
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < P; q += (size_t)gridDim.x * blockDim.x) {
        const int k = q >= l.pad_before[2] ? 2 : q >= l.pad_before[1] ? 1 : 0;
        const uint32_t i = (l.off[k + 1] - l.off[k]) + ((uint32_t)q - l.pad_before[k]), ts = zc[4 * side + k] + (uint32_t)q;
        if (a.ts_u32[side][k]) a.ts_u32[side][k][i] = ts;
        if (a.ts_fr[side][k]) a.ts_fr[side][k][i] = fr_from_u64((uint64_t)ts);
        if (q == 0) {
            const uint32_t total = zc[4 * side + 3] + P;
            if (a.audit_u32[side]) a.audit_u32[side][0] = total;
            if (a.audit_fr[side]) a.audit_fr[side][0] = fr_from_u64((uint64_t)total);
        }
    }
}
void dev_addr_timestamps(DevCtx &c, const AddrTs &a) {
    if (a.sides < 1 || a.sides > 2 || a.N < 1 || a.M < 1 || a.N > ((size_t)1 << 28) || a.M > ((size_t)1 << 31)) throw Error(OTTI_ERR_BAD_ARG, "address timestamps: 1 or 2 sides, lists of at most 2^28 entries, at most 2^31 addresses");
    AtLens l; l.off[0] = 0; l.pad_before[0] = 0;
    for (int k = 0; k < 3; k++) {
        if (a.len[k] > a.N) throw Error(OTTI_ERR_BAD_ARG, "address timestamps: a list longer than N");
        l.off[k + 1] = l.off[k] + a.len[k]; l.pad_before[k + 1] = l.pad_before[k] + (uint32_t)(a.N - a.len[k]);
    }
    const uint32_t L = l.off[3], P = l.pad_before[3], nwg = (L + kAtTile - 1) / kAtTile;
    const unsigned sides = (unsigned)a.sides;
    int passes = 1; while (passes < 4 && (a.M - 1) >> (8 * passes)) passes++;
    // scratch: two key and two index arrays (ping-pong), first positions per address, digit counts, the zero counts
    const size_t n_hist = (size_t)sides * 256 * std::max<uint32_t>(nwg, 1);
    DevBuf<uint32_t> scratch((size_t)sides * (4 * (size_t)L + a.M) + n_hist + 8);
    uint32_t *key[2] = {scratch.p, scratch.p + (size_t)sides * L}, *idx[2] = {key[1] + (size_t)sides * L, key[1] + 2 * (size_t)sides * L};
    uint32_t *start = idx[1] + (size_t)sides * L, *hist = start + (size_t)sides * a.M, *zc = hist + n_hist;
    std::vector<DevBuf<uint32_t>> scan_levels; scan_levels.reserve(4);
    KScope ks(c, KC_GATHER);
    for (unsigned s = 0; s < sides; s++) {
        if (a.audit_u32[s]) OTTI_HIP(hipMemsetAsync(a.audit_u32[s], 0, a.M * sizeof(uint32_t), c.stream));
        if (a.audit_fr[s]) OTTI_HIP(hipMemsetAsync(a.audit_fr[s], 0, a.M * sizeof(Fr), c.stream));
    }
    OTTI_HIP(hipMemsetAsync(zc, 0, 8 * sizeof(uint32_t), c.stream));
    if (L) {
        hipLaunchKernelGGL(k_at_pack, dim3(grid_for(L), sides), kBlock, 0, c.stream, a, l, key[0]);
        int cur = 0;
        for (int p = 0; p < passes; p++, cur ^= 1) {
            hipLaunchKernelGGL(k_at_hist, dim3(nwg, sides), kBlock, 0, c.stream, (const uint32_t *)key[cur], L, 8 * p, hist, nwg);
            scan_inplace(c, hist, n_hist, scan_levels);
            if (p == 0) hipLaunchKernelGGL(k_at_scatter<true>, dim3(nwg, sides), kBlock, 0, c.stream, (const uint32_t *)key[cur], (const uint32_t *)nullptr, key[cur ^ 1], idx[cur ^ 1], L, 8 * p, (const uint32_t *)hist, nwg);
            else hipLaunchKernelGGL(k_at_scatter<false>, dim3(nwg, sides), kBlock, 0, c.stream, (const uint32_t *)key[cur], (const uint32_t *)idx[cur], key[cur ^ 1], idx[cur ^ 1], L, 8 * p, (const uint32_t *)hist, nwg);
        }
        hipLaunchKernelGGL(k_at_heads, dim3(grid_for(L), sides), kBlock, 0, c.stream, (const uint32_t *)key[cur], L, start, a.M);
        hipLaunchKernelGGL(k_at_ranks, dim3(grid_for(L), sides), kBlock, 0, c.stream, a, l, (const uint32_t *)key[cur], (const uint32_t *)idx[cur], (const uint32_t *)start);
        if (P) hipLaunchKernelGGL(k_at_zero, sides, 64, 0, c.stream, l, (const uint32_t *)key[cur], (const uint32_t *)idx[cur], zc);
    }
    if (P) hipLaunchKernelGGL(k_at_tail, dim3(grid_for(P), sides), kBlock, 0, c.stream, a, l, (const uint32_t *)zc);
    OTTI_HIP(hipStreamSynchronize(c.stream));                 // the scratch goes out of scope
}

// hash(addr, val, ts) - gamma = ts * r^2 + val * r + addr - gamma
__device__ __forceinline__ Fr hash3(const Fr &addr, const Fr &val, const Fr &ts, const Fr &r, const Fr &r2, const Fr &gamma) {
    return fr_sub(fr_add(fr_add(fr_mul(ts, r2), fr_mul(val, r)), addr), gamma);
}
// A rank's residue class of a hashed vector (sharded SNARK::prove, snark_prover.cpp build_circuits): local element j of a vector of 2 * half_loc elements is
// global element (j / half_loc) * half_glob + (j % half_loc) * G + rk — the circuit's input is its left half then its right half, and every
// layer pairs index i with i + (side length) / 2, so both halves keep the elements with i = rk (mod G).  G = 1: the identity.
struct ShardMap { size_t half_loc, half_glob; uint32_t G, rk; };
__device__ __forceinline__ size_t shard_global(const ShardMap &m, size_t j) { return m.G == 1 ? j : (j / m.half_loc) * m.half_glob + (j % m.half_loc) * m.G + m.rk; }
// memory cells: addr = the cell index, val = the eq table, ts = 0 (init) or the audit timestamp
__global__ __launch_bounds__(kBlock) void k_hash_mem(const Fr *eval_table, const Fr *audit_ts, Fr *out_init, Fr *out_audit, size_t M, Fr r, Fr r2, Fr gamma, ShardMap sm) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < M; j += (size_t)gridDim.x * blockDim.x) {
        const size_t i = shard_global(sm, j);
        const Fr base = fr_sub(fr_add(fr_mul(eval_table[i], r), fr_from_u64((uint64_t)i)), gamma);
        out_init[j] = base;
        out_audit[j] = fr_add(base, fr_mul(audit_ts[i], r2));
    }
}
// operations: read uses the read timestamp, write the same plus one (so write = read + r^2)
__global__ __launch_bounds__(kBlock) void k_hash_ops(const Fr *addr_f, const Fr *deref, const Fr *read_ts, Fr *out_read, Fr *out_write, size_t N, Fr r, Fr r2, Fr gamma, ShardMap sm) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < N; j += (size_t)gridDim.x * blockDim.x) {
        const size_t i = shard_global(sm, j);
        const Fr rd = hash3(addr_f[i], deref[i], read_ts[i], r, r2, gamma);
        out_read[j] = rd; out_write[j] = fr_add(rd, r2);
    }
}
// n = the GLOBAL vector length; G ranks: this rank writes its n / G elements
void dev_hash_mem(DevCtx &c, const Fr *eval_table, const Fr *audit_ts, Fr *out_init, Fr *out_audit, size_t M, const Fr &r, const Fr &gamma, int G, int rk) {
    KScope ks(c, KC_HASH_LAYER);
    const size_t Ml = M / (size_t)G; const ShardMap sm = {std::max<size_t>(1, Ml / 2), M / 2, (uint32_t)G, (uint32_t)rk};
    hipLaunchKernelGGL(k_hash_mem, grid_for(Ml), kBlock, 0, c.stream, eval_table, audit_ts, out_init, out_audit, Ml, r, fr_mul(r, r), gamma, sm);
}
void dev_hash_ops(DevCtx &c, const Fr *addr_f, const Fr *deref, const Fr *read_ts, Fr *out_read, Fr *out_write, size_t N, const Fr &r, const Fr &gamma, int G, int rk) {
    KScope ks(c, KC_HASH_LAYER);
    const size_t Nl = N / (size_t)G; const ShardMap sm = {std::max<size_t>(1, Nl / 2), N / 2, (uint32_t)G, (uint32_t)rk};
    hipLaunchKernelGGL(k_hash_ops, grid_for(Nl), kBlock, 0, c.stream, addr_f, deref, read_ts, out_read, out_write, Nl, r, fr_mul(r, r), gamma, sm);
}

// one layer of every product circuit of a batch: out_left[i] = in_left[i] * in_right[i], out_right[i] = in_left[q + i] * in_right[q + i]
__global__ __launch_bounds__(kBlock) void k_prod_layer(LayerList L, size_t q) {
    const Fr *il = L.in_left[blockIdx.y], *ir = L.in_right[blockIdx.y]; Fr *ol = L.out_left[blockIdx.y], *orr = L.out_right[blockIdx.y];
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < q; i += (size_t)gridDim.x * blockDim.x) {
        ol[i] = fr_mul(il[i], ir[i]); orr[i] = fr_mul(il[q + i], ir[q + i]);
    }
}
void dev_prod_layer(DevCtx &c, const LayerList &L, size_t q) {
    if (!q || !L.n) return;
    KScope ks(c, KC_PROD_LAYER);
    hipLaunchKernelGGL(k_prod_layer, dim3((unsigned)grid_for(q), (unsigned)L.n), kBlock, 0, c.stream, L, q);
}

// out[y * K + k] = sum over the nblk partials of instance y (out may be pinned host memory)
template <int K> __global__ __launch_bounds__(kBlock) void k_reduce_many(const Fr *partials, int nblk, Fr *out) {
    Fr acc[K];
    for (int k = 0; k < K; k++) acc[k] = fr_zero();
    for (int b = threadIdx.x; b < nblk; b += blockDim.x)
        for (int k = 0; k < K; k++) acc[k] = fr_add(acc[k], partials[((size_t)blockIdx.x * nblk + b) * K + k]);
    block_reduce<K>(acc);
    if (threadIdx.x == 0) for (int k = 0; k < K; k++) out[(size_t)blockIdx.x * K + k] = acc[k];
}
// The grid of the launches over a batch (pc_plan.h pc_round_grid) under the block cap in force: the device's own, kMaxBlocks, or what the tests put
// in its place (otti_k_pc_grid_cap_override) so that short tables walk the many-items-per-thread path of long ones.  Never above kMaxBlocks (the
// partial sums' buffers are sized by it); written only while no proof is in flight; never set by the prover.
static_assert(kPcThreads == kBlock && kPcMaxBlocks == kMaxBlocks, "pc_plan.h restates device.h");
static std::atomic<unsigned> g_pc_grid_cap{0};                // 0: the device's own
void pc_grid_cap_override(unsigned max_blocks) {
    if (ActiveProof::count() != 0) throw Error(OTTI_ERR_BAD_ARG, "the batched launches' block cap cannot change while a proof is in flight");
    if (max_blocks > (unsigned)kMaxBlocks) throw Error(OTTI_ERR_BAD_ARG, "a block cap above the device's own (kMaxBlocks): the partial sums' buffers end there");
    g_pc_grid_cap.store(max_blocks, std::memory_order_release);
}
PcGrid pc_grid(size_t items, int ninst) {
    const unsigned cap = g_pc_grid_cap.load(std::memory_order_acquire);
    return pc_round_grid(items, ninst, cap ? cap : (unsigned)kMaxBlocks);
}
static inline int many_grid(size_t n, int ninst) { return (int)pc_grid(n, ninst).workgroups; }
// ---- a round of the batched cubic sum-check as ONE launch (fold by the previous challenge + the sums of this round at the points 0, 2, 3
// of the variable being bound), results mailed to the host by the last workgroup (finish_in_kernel of k_sumcheck.hip, here for every
// instance of the batch at once).
// An instance without a third table (a product circuit: L.C[y] == nullptr): its three totals are (Q(0), Q(1), leading coefficient) of a quadratic (product-circuit instances of the nine-limb
// round kernel) and leave as its values at 0, 2, 3; otherwise they are those values already (dot-product triples).
__device__ __forceinline__ void finish_many(Fr (&acc)[3], const Mailbox &mb, const PcList &L) {
    block_reduce<3>(acc);
    const unsigned total = gridDim.x * gridDim.y, ny = gridDim.y;
    if (total == 1) {
        if (threadIdx.x == 0) {
            if (!L.C[0]) quadratic_to_023(acc);
            for (int k = 0; k < 3; k++) mb.host_results[mb.slot + k] = acc[k];
            __threadfence_system();
            __hip_atomic_store(mb.host_flag, mb.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    __shared__ Fr s_tot[3 * 64];
    if (threadIdx.x == 0) for (int k = 0; k < 3; k++) store_words_sc1(&mb.partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + k], acc[k].v, 8);
    if (!arrive_and_check_last(mb.counter, total)) return;
    // last workgroup: output o = (instance, t) is summed by four adjacent lanes
    const unsigned o = threadIdx.x >> 2, sub = threadIdx.x & 3;
    Fr s = fr_zero();
    if (o < 3 * ny) {
        const unsigned y = o / 3, k = o % 3;
        for (unsigned b = sub; b < gridDim.x; b += 4) { Fr t; load_words_sc1(t.v, &mb.partials[((size_t)y * gridDim.x + b) * 3 + k], 8); s = fr_add(s, t); }
    }
    s = fr_add(s, shfl_xor_fr(s, 1)); s = fr_add(s, shfl_xor_fr(s, 2));
    if (o < 3 * ny && sub == 0) s_tot[o] = s;
    __syncthreads();
    if (threadIdx.x < ny) {
        Fr q[3] = {s_tot[3 * threadIdx.x], s_tot[3 * threadIdx.x + 1], s_tot[3 * threadIdx.x + 2]};
        if (!L.C[threadIdx.x]) quadratic_to_023(q);
        for (int k = 0; k < 3; k++) mb.host_results[mb.slot + 3 * threadIdx.x + k] = q[k];
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(mb.host_flag, mb.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// ---- nine-limb forms (fr9.h).  What an item adds to a thread's three sums — abe_accum9 for a product-circuit instance, abc_accum9 for a dot-product
// triple — and the sweep / fold step after it, pc_acc_step, with the walk bound kPcWalkMax: pc_accum9.h, where a host compiler reads them too.
// kFold: the tables have 4q entries and are folded by r to 2q (pairs (i, i + q)); otherwise they have 2q entries as they are
template <bool kFold> __global__ __launch_bounds__(kBlock) void k_pc_round(PcList L, size_t q, Fr r, EqSrc E, Mailbox mb, Armed go) {
    if (kFold && go.want) { Fr v[1]; if (!armed_fetch<1>(go, v)) return; r = v[0]; }
    Fr *A = L.A[blockIdx.y], *B = L.B[blockIdx.y], *C = L.C[blockIdx.y];
    const Fr9 r5 = fr9_unpack5(r);
    Fr9 acc[3] = {fr9_zero(), fr9_zero(), fr9_zero()}; unsigned n = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < q; i += (size_t)gridDim.x * blockDim.x) {
        Fr9 a_lo, a_hi, b_lo, b_hi;
        if (kFold) {
            const Fr a0 = A[i], a1 = A[i + q], a2 = A[i + 2 * q], a3 = A[i + 3 * q];
            const Fr b0 = B[i], b1 = B[i + q], b2 = B[i + 2 * q], b3 = B[i + 3 * q];
            __builtin_amdgcn_sched_barrier(0);
            Fr w0, w1;
            a_lo = fold9(a0, a2, r5, w0); a_hi = fold9(a1, a3, r5, w1); A[i] = w0; A[i + q] = w1;
            b_lo = fold9(b0, b2, r5, w0); b_hi = fold9(b1, b3, r5, w1); B[i] = w0; B[i + q] = w1;
        } else {
            const Fr a0 = A[i], a1 = A[i + q], b0 = B[i], b1 = B[i + q];
            __builtin_amdgcn_sched_barrier(0);
            a_lo = fr9_unpack(a0); a_hi = fr9_unpack(a1); b_lo = fr9_unpack(b0); b_hi = fr9_unpack(b1);
        }
        if (C) {
            Fr9 c_lo5, c_hi5;
            if (kFold) {
                const Fr c0 = C[i], c1 = C[i + q], c2 = C[i + 2 * q], c3 = C[i + 3 * q];
                Fr w0, w1;
                const Fr9 c_lo = fold9(c0, c2, r5, w0), c_hi = fold9(c1, c3, r5, w1); C[i] = w0; C[i + q] = w1;
                c_lo5 = fr9_shl5(c_lo); c_hi5 = fr9_shl5(c_hi);
            } else { c_lo5 = fr9_unpack5(C[i]); c_hi5 = fr9_unpack5(C[i + q]); }
            abc_accum9(acc, a_lo, a_hi, fr9_shl5(b_lo), fr9_shl5(b_hi), c_lo5, c_hi5);
        } else abe_accum9(acc, a_lo, a_hi, b_lo, b_hi, eq_s_at<10>(E, i));
        pc_acc_step(acc, n);
    }
    Fr tot[3]; acc9_canon<3>(tot, acc);
    finish_many(tot, mb, L);
}
static Mailbox pc_mailbox(DevCtx &c, int slot, int nblocks) {
    if ((size_t)nblocks * 3 > c.partials.n) throw Error(OTTI_ERR_INTERNAL, "round partials exceed the context's buffer");
    return c.next_mailbox(slot);
}
// The walk k_pc_round can take.  Its sums are folded back every kPcWalkMax items (pc_accum9.h), so no length overflows them; what is left is the
// 32-bit item count, which may even wrap (kPcWalkMax divides 2^32).  The refusal below therefore cannot be reached — a walk of 2^32 items needs
// tables of 2^40 elements under a cap of one block — and no test shows it; it stands for the day the step changes.
constexpr size_t kPcWalkLimit = (size_t)1 << 32;
static int pc_round_blocks(size_t items, int ninst) {
    const PcGrid g = pc_grid(items, ninst);
    if (g.items_per_thread > kPcWalkLimit) throw Error(OTTI_ERR_INTERNAL, "a thread of the batched round kernel would walk more items than its sums can take");
    return (int)g.workgroups;
}
unsigned long long dev_pc_eval(DevCtx &c, const PcList &L, size_t len, const EqSrc &E, int slot) {
    const size_t half = len / 2; const int g = pc_round_blocks(half, L.n); Mailbox mb = pc_mailbox(c, slot, g * L.n);
    KScope ks(c, KC_PC_ROUND);
    hipLaunchKernelGGL(k_pc_round<false>, dim3((unsigned)g, (unsigned)L.n), kBlock, 0, c.stream, L, half, fr_zero(), E, mb, Armed{nullptr, nullptr, 0});
    return mb.seq;
}
unsigned long long dev_pc_fold_eval(DevCtx &c, const PcList &L, size_t len, const Fr *r, const EqSrc &E, int slot) {
    if (len < 4) throw Error(OTTI_ERR_INTERNAL, "fold_eval needs len >= 4");
    const size_t q = len / 4; const int g = pc_round_blocks(q, L.n); Mailbox mb = pc_mailbox(c, slot, g * L.n);
    const Armed go = r ? Armed{nullptr, nullptr, 0} : c.arm();
    KScope ks(c, KC_PC_ROUND);
    hipLaunchKernelGGL(k_pc_round<true>, dim3((unsigned)g, (unsigned)L.n), kBlock, 0, c.stream, L, q, r ? *r : fr_zero(), E, mb, go);
    return mb.seq;
}
// tail hand-over: every table of the batch (folded by r when fold is set) into pinned host memory; the flag follows the last workgroup
__global__ __launch_bounds__(64) void k_pc_export(PcList L, size_t n_out, int fold, Fr r, Mailbox mb, Armed go) {
    if (go.want) { Fr v[1]; if (!armed_fetch<1>(go, v)) return; r = v[0]; }
    const Fr *T[3] = {L.A[blockIdx.y], L.B[blockIdx.y], L.C[blockIdx.y]};
    for (int t = 0; t < 3; t++) {
        if (!T[t]) continue;
        Fr *out = mb.host_results + mb.slot + ((size_t)3 * blockIdx.y + t) * n_out;
        for (size_t i = threadIdx.x; i < n_out; i += blockDim.x) {
            Fr v = T[t][i];
            if (fold) v = fr_add(v, fr_mul(r, fr_sub(T[t][i + n_out], v)));
            out[i] = v;
        }
    }
    __threadfence_system();
    __syncthreads();
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        unsigned old = __hip_atomic_fetch_add(mb.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == gridDim.y - 1;
        if (s_last) {
            __hip_atomic_store(mb.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence_system();
            __hip_atomic_store(mb.host_flag, mb.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
unsigned long long dev_pc_export(DevCtx &c, const PcList &L, size_t len, bool fold, const Fr *r, int slot) {
    const size_t n_out = fold ? len / 2 : len;
    if (slot + (size_t)3 * L.n * n_out > (size_t)kResultSlots) throw Error(OTTI_ERR_INTERNAL, "sum-check tail does not fit the pinned result buffer");
    Mailbox mb = c.next_mailbox(slot);
    const Armed go = (fold && !r) ? c.arm() : Armed{nullptr, nullptr, 0};
    KScope ks(c, KC_PC_ROUND);
    hipLaunchKernelGGL(k_pc_export, dim3(1, (unsigned)L.n), 64, 0, c.stream, L, n_out, fold ? 1 : 0, r ? *r : fr_zero(), mb, go);
    return mb.seq;
}
// ------------------------------------------------------------------------------------------------ the persistent tail (snark_dev.h)
struct TailArgs {
    PcList L; int W; uint32_t len0, t_out; int fold_on_load; Fr r; EqSrc E;
    TailMail *mail; Fr *host_out; unsigned long long seq0; Armed go;        // go.want: the go() number of the first round's challenge
    unsigned long long *stamps;                                             // OTTI_TAIL_STAMPS: wall_clock64 (100 MHz) of workgroup (0,0) at the phase boundaries, 8 per round
    int test_drop;                                                          // OTTI_TEST_TAIL_DROP (tests): every other workgroup returns at once, as if it had never become resident
};
// A wave works on ONE evaluation point (wave % 3) and group g = wave / 3 takes the pairs g*64 + lane, + 64*groups, ...: no divergence over
// the point inside a wave, and a wave's 64 partial sums of its one point fold by shuffles of ONE field element per level (the first
// version gave every lane its own point and reduced three elements, two of them zero, over all lanes: 11 us at 1024 elements per table).
// s_part[pt][g] <- the wave's sum; threads 0..2 add the groups that had pairs into s_tot[0..3).  Every thread of the workgroup calls it.
__device__ __forceinline__ void tail_reduce1(Fr acc, int pt, int grp, int ngrp, uint32_t half, Fr (*s_part)[16], Fr *s_tot) {
    const int lane = threadIdx.x & 63, groups = (int)min((uint32_t)ngrp, (half + 63) / 64);
    if (grp < groups) {
        int top = 64; if (half < 64) { top = 1; while ((uint32_t)top < half) top <<= 1; }          // lanes at and beyond `half` hold zero: only as many levels as there is data
#pragma unroll 1
        for (int off = top >> 1; off >= 1; off >>= 1) acc = fr_add(acc, shfl_xor_fr(acc, off));
        if (lane == 0) s_part[pt][grp] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 3) { Fr t = s_part[threadIdx.x][0]; for (int g = 1; g < groups; g++) t = fr_add(t, s_part[threadIdx.x][g]); s_tot[threadIdx.x] = t; }
    __syncthreads();
}
// s_tot: the round's sums in LDS (visible to the whole workgroup).  A round's mail is the line in one instruction (snark_dev.h); the hand-over
// after the last round follows plain stores of the tables into pinned memory and keeps its release fence.
__device__ __forceinline__ void tail_post(TailMail *m, const Fr *s_tot, bool with_sums, unsigned long long seq) {
    if (with_sums) {
        if (threadIdx.x < 8) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            const unsigned lane = threadIdx.x;
            u32x4 q = {0u, 0u, 0u, 0u};
            if (lane < 6) { const Fr &x = s_tot[lane >> 1]; for (int i = 0; i < 4; i++) q[i] = x.v[4 * (lane & 1) + i]; }
            else if (lane == 6) { const unsigned long long tag = go_tag(seq, s_tot, 3); q[0] = (uint32_t)seq; q[1] = (uint32_t)(seq >> 32); q[2] = (uint32_t)tag; q[3] = (uint32_t)(tag >> 32); }
            asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(reinterpret_cast<char *>(m) + 16 * lane), "v"(q) : "memory");
        }
    } else if (threadIdx.x == 0) {
        __threadfence_system();
        __hip_atomic_store(&m->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
__global__ __launch_bounds__(kTailThreads) void k_pc_tail(TailArgs a) {
    __shared__ Fr T0[3 * kTailCap];                                    // three tables of kTailCap elements: A, B, C (96 KB of the CU's 160: one workgroup per CU)
    __shared__ Fr s_part[3][16]; __shared__ Fr s_tot[3];
    const int w = blockIdx.x, y = blockIdx.y, W = a.W, tid = threadIdx.x, nthr = blockDim.x;
    if (a.test_drop && ((w + y) & 1)) return;
    const Fr *src[3] = {a.L.A[y], a.L.B[y], a.L.C[y]};
    TailMail *const mail = a.mail + (size_t)y * W + w;
    uint32_t L = a.len0 / (uint32_t)W;                                  // this workgroup's share of every table
    // ---- load (folding by the previous round's challenge when the tables in HBM are one round behind); element j here is element j W + w there
    const Fr9 r_load5 = fr9_unpack5(a.r);
    for (uint32_t idx = tid; idx < 3 * L; idx += nthr) {
        const uint32_t t = idx / L, j = idx - t * L; const size_t i = (size_t)j * W + w;
        Fr v;
        if (!src[t]) v = eq_at(a.E, i);                                 // product circuit: the shared eq table, materialised (t == 2 only)
        else if (a.fold_on_load) { const Fr lo = src[t][i], hi = src[t][i + a.len0]; (void)fold9(lo, hi, r_load5, v); }
        else v = src[t][i];
        T0[t * kTailCap + j] = v;
    }
    __syncthreads();
    unsigned long long seq = a.seq0, want = a.go.want;
    const uint32_t L_out = a.t_out / (uint32_t)W;
    unsigned long long *stamp = (a.stamps && tid == 0 && w == 0 && y == 0) ? a.stamps : nullptr; int rnd = 0;
    if (stamp) stamp[0] = wall_clock64();
    const int wave = tid >> 6, lane = tid & 63, ngrp = (nthr >> 6) / 3, pt = wave % 3, grp = wave / 3;   // wave -> evaluation point (0, 2, 3) and group of pairs; the 16th wave of 1024 threads idles
    while (L > L_out) {
        const uint32_t half = L / 2;
        // ---- this round's sums: S_t = sum over pairs of (A_t B_t C_t), t in {0, 2, 3}
        // nine limbs (fr9.h): the first table plain, the other two times 32 — each of the two products then has exactly one operand carrying the
        // radix correction (abc_accum9 of pc_accum9.h has the bounds; here every operand comes canonical out of the LDS)
        Fr9 acc9 = fr9_zero(); unsigned n_acc = 0;
        if (grp < ngrp)
            for (uint32_t p = (uint32_t)grp * 64 + lane; p < half; p += (uint32_t)ngrp * 64) {
                const Fr9 a_lo = fr9_unpack(T0[p]), b_lo5 = fr9_unpack5(T0[kTailCap + p]), c_lo5 = fr9_unpack5(T0[2 * kTailCap + p]);
                Fr9 term;
                if (pt == 0) term = fr9_mul(fr9_mul(a_lo, b_lo5), c_lo5);
                else {
                    const Fr9 a_hi = fr9_unpack(T0[p + half]), b_hi5 = fr9_unpack5(T0[kTailCap + p + half]), c_hi5 = fr9_unpack5(T0[2 * kTailCap + p + half]);
                    const Fr9 x2 = fr9_norm(fr9_sub_kl<4>(fr9_add(a_hi, a_hi), a_lo));
                    const Fr9 y2 = fr9_sub_kl<128>(fr9_add(b_hi5, b_hi5), b_lo5), z2 = fr9_sub_kl<128>(fr9_add(c_hi5, c_hi5), c_lo5);
                    if (pt == 1) term = fr9_mul(fr9_mul(x2, y2), z2);
                    else {
                        const Fr9 x3 = fr9_norm(fr9_add(x2, fr9_sub_kl<4>(a_hi, a_lo)));
                        const Fr9 y3 = fr9_norm(fr9_add(y2, fr9_sub_kl<128>(b_hi5, b_lo5))), z3 = fr9_norm(fr9_add(z2, fr9_sub_kl<128>(c_hi5, c_lo5)));
                        term = fr9_mul(fr9_mul(x3, y3), z3);
                    }
                }
                acc9 = fr9_add(acc9, term);
                if ((++n_acc & 3u) == 0) acc9 = fr9_norm(acc9);
            }
        Fr acc = fr9_canon(fr9_norm(acc9));
        if (stamp) stamp[8 * rnd + 1] = wall_clock64();               // sums done
        tail_reduce1(acc, pt, grp, ngrp, half, s_part, s_tot);
        if (stamp) stamp[8 * rnd + 2] = wall_clock64();               // reduced
        tail_post(mail, s_tot, true, seq++);
        if (stamp) stamp[8 * rnd + 3] = wall_clock64();               // mailed
        // ---- the round's challenge, then bound_poly_var_top of the three tables in LDS
        Fr rv[1]; Armed g = a.go; g.want = want++;
        if (!armed_fetch<1>(g, rv)) return;
        if (stamp) stamp[8 * rnd + 4] = wall_clock64();               // challenge here
        const Fr9 r5 = fr9_unpack5(rv[0]);
        for (uint32_t idx = tid; idx < 3 * half; idx += nthr) {
            const uint32_t t = idx / half, e = idx - t * half;
            Fr *X = T0 + t * kTailCap;
            Fr w; (void)fold9(X[e], X[e + half], r5, w);
            X[e] = w;
        }
        __syncthreads();
        L = half;
        if (stamp) { stamp[8 * rnd + 5] = wall_clock64(); rnd++; stamp[8 * rnd] = stamp[8 * (rnd - 1) + 5]; }   // folded = next round's start
    }
    // ---- hand the host-played tail over: table t of instance y at host_out[(3 y + t) * t_out ..), element j of this workgroup at j W + w
    for (uint32_t idx = tid; idx < 3 * L; idx += nthr) {
        const uint32_t t = idx / L, j = idx - t * L;
        if (!src[t]) continue;
        a.host_out[((size_t)3 * y + t) * a.t_out + (size_t)j * W + w] = T0[t * kTailCap + j];
    }
    __threadfence_system();
    __syncthreads();
    tail_post(mail, s_tot, false, seq);
}
unsigned long long dev_pc_tail(DevCtx &c, const PcList &L, int W, size_t len0, size_t t_out, const Fr *fold_r, const EqSrc &E, int slot) {
    int rounds = 0; for (size_t l = len0; l > t_out; l >>= 1) rounds++;
    if (W < 1 || (W & (W - 1)) || L.n < 1 || L.n * W > kTailMaxGroups || len0 / (size_t)W > (size_t)kTailCap || (len0 & (len0 - 1)) || (t_out & (t_out - 1)) ||
        t_out < (size_t)W || len0 <= t_out || rounds < 1)
        throw Error(OTTI_ERR_INTERNAL, "persistent sum-check tail: bad geometry");
    if (slot + (size_t)3 * L.n * t_out > (size_t)kResultSlots) throw Error(OTTI_ERR_INTERNAL, "sum-check tail does not fit the pinned result buffer");
    c.tail_mail.ensure(c);
    TailArgs a;
    a.L = L; a.W = W; a.len0 = (uint32_t)len0; a.t_out = (uint32_t)t_out; a.fold_on_load = fold_r ? 1 : 0; a.r = fold_r ? *fold_r : fr_zero(); a.E = E;
    a.mail = c.tail_mail.dev; a.host_out = c.d_results_alias + slot;
    a.seq0 = c.seq + 1; c.seq += (unsigned long long)rounds + 1;
    a.go = c.arm_many(rounds);
    static const bool test_drop = getenv("OTTI_TEST_TAIL_DROP") != nullptr;
    a.test_drop = test_drop ? 1 : 0;

    static const bool want_stamps = getenv("OTTI_TAIL_STAMPS") != nullptr;
    static thread_local unsigned long long *h_stamps = nullptr, *d_stamps = nullptr;
    a.stamps = nullptr;
    if (want_stamps) {
        if (!h_stamps) { OTTI_HIP(hipHostMalloc((void **)&h_stamps, 8 * 32 * 8, hipHostMallocDefault)); OTTI_HIP(hipHostGetDevicePointer((void **)&d_stamps, h_stamps, 0)); }
        else {                                                    // the previous launch's stamps (its kernel has long finished: the host went through all its rounds)
            const unsigned long long *t = h_stamps; const int nr_ = (int)t[8 * 31];
            for (int r = 0; r < nr_ && r < 30; r++)
                fprintf(stderr, "[otti] k_pc_tail W=%d L=%llu round %d: sums %.2f | reduce %.2f | mail %.2f | wait for the challenge %.2f | fold %.2f us\n", (int)t[8 * 31 + 1], t[8 * 31 + 2] >> r, r,
                        0.01 * (double)(t[8 * r + 1] - t[8 * r]), 0.01 * (double)(t[8 * r + 2] - t[8 * r + 1]), 0.01 * (double)(t[8 * r + 3] - t[8 * r + 2]),
                        0.01 * (double)(t[8 * r + 4] - t[8 * r + 3]), 0.01 * (double)(t[8 * r + 5] - t[8 * r + 4]));
        }
        memset(h_stamps, 0, 8 * 32 * 8); h_stamps[8 * 31] = (unsigned long long)rounds; h_stamps[8 * 31 + 1] = (unsigned long long)W; h_stamps[8 * 31 + 2] = len0 / (size_t)W;
        a.stamps = d_stamps;
    }
    KScope ks(c, KC_PC_ROUND);
    hipLaunchKernelGGL(k_pc_tail, dim3((unsigned)W, (unsigned)L.n), kTailThreads, 0, c.stream, a);
    return a.seq0;
}
// element 0 of every table of the list -> c.h_results[slot ..)
__global__ void k_pick0(PtrList L, Fr *out) { const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < L.n) out[i] = L.p[i][0]; }
void dev_pick0(DevCtx &c, const PtrList &L, int slot) { if (L.n) hipLaunchKernelGGL(k_pick0, 1, 64, 0, c.stream, L, c.d_results_alias + slot); }

// ---- evaluations: out[y] = <E, P_y> for every polynomial of the list (E: the eq table of the point), and sum l * r * w
__global__ __launch_bounds__(kBlock) void k_dot_many(const Fr *E, PtrList L, size_t n, Fr *partials) {
    const Fr *P = L.p[blockIdx.y];
    Fr acc[1] = {fr_zero()};
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc[0] = fr_add(acc[0], fr_mul(E[i], P[i]));
    block_reduce<1>(acc);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}
void dev_dot_many(DevCtx &c, const Fr *E, const PtrList &L, size_t n, Fr *partials, int slot) {
    const int g = many_grid(n, L.n);
    KScope ks(c, KC_DOT_MANY);
    hipLaunchKernelGGL(k_dot_many, dim3((unsigned)g, (unsigned)L.n), kBlock, 0, c.stream, E, L, n, partials);
    hipLaunchKernelGGL(k_reduce_many<1>, L.n, kBlock, 0, c.stream, (const Fr *)partials, g, c.d_results_alias + slot);
}
__global__ __launch_bounds__(kBlock) void k_sum3(AbcList L, size_t n, Fr *partials) {
    const Fr *A = L.A[blockIdx.y], *B = L.B[blockIdx.y], *C = L.C[blockIdx.y];
    Fr acc[1] = {fr_zero()};
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc[0] = fr_add(acc[0], fr_mul(fr_mul(A[i], B[i]), C[i]));
    block_reduce<1>(acc);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}
void dev_sum3(DevCtx &c, const AbcList &L, size_t n, Fr *partials, int slot) {
    const int g = many_grid(n, L.n);
    KScope ks(c, KC_DOT_MANY);
    hipLaunchKernelGGL(k_sum3, dim3((unsigned)g, (unsigned)L.n), kBlock, 0, c.stream, L, n, partials);
    hipLaunchKernelGGL(k_reduce_many<1>, L.n, kBlock, 0, c.stream, (const Fr *)partials, g, c.d_results_alias + slot);
}

}  // namespace otti
