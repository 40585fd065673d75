// What the three sources of SNARK mode's GPU prover share: snark_encode.cpp (SNARK::encode / attach: the decommitment in HBM), snark_pc.cpp
// (the product circuits and their batched sum-check) and snark_prover.cpp (SNARK::prove).  Internal: snark.h is the public face.
#pragma once
#include "snark.h"
#include "snark_dev.h"
#include "shard.h"
#include <chrono>

namespace otti {

static inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the dense representation of sparse_mlpoly.rs MultiSparseMatPolynomialAsDense, resident in HBM
struct DeviceDecomm {
    size_t N = 0, M = 0;
    DevBuf<uint32_t> row_addr[3], col_addr[3];
    DevBuf<Fr> comb_ops;                                     // [row addr A,B,C | row read_ts A,B,C | col addr A,B,C | col read_ts A,B,C | val A,B,C | 0..]: 16 N
    DevBuf<Fr> comb_mem;                                     // [row audit_ts | col audit_ts]: 2 M
    Fr *part(int p, int k) const { return comb_ops.p + (size_t)(3 * p + k) * N; }
};
// Per-proof buffers (2.5 GB at 2^20: dereferenced values, sixteen product circuits with all their layers, dot-product tables, ...) are
// kept with the calling thread's device context and only ever grow: allocating and freeing them per proof cost ~4 ms of a 34 ms proof.
struct SnarkScratch {
    std::vector<DevBuf<Fr>> b;
    Fr *get(size_t slot, size_t n) { if (b.size() <= slot) b.resize(slot + 1); if (b[slot].n < n) b[slot].alloc(n); return b[slot].p; }
};
enum { SS_MEM_RX = 0, SS_MEM_RY, SS_EQS, SS_DEREFS, SS_PARTIALS, SS_DOTP, SS_PYR, SS_EO, SS_EM, SS_PE0 /* 11 slots */, SS_OPS = SS_PE0 + 11 /* 12 */, SS_MEMC = SS_OPS + 12 /* 4 */, SS_AHEAD = SS_MEMC + 4 /* 6: chunk sums of two bounds, their left and right eq tables */ };
inline SnarkScratch &snark_workspace(DevCtx &c) { if (!c.snark_scratch) c.snark_scratch = new SnarkScratch(); return *c.snark_scratch; }
// sparse_hint: 1 / 0 = the scalars are / are not mostly small numbers (picks the bulk MSM variant); -1 = look (a pass over Z and a synchronise)
inline std::vector<CPoint> commit_poly(DevCtx &c, Gens &gens, const Fr *Z, const PcSet &s, int sparse_hint = -1) {
    ensure_gens_device(gens);
    const bool sparse = sparse_hint >= 0 ? sparse_hint != 0 : dev_small_fraction(c, Z, s.L * s.R) > kSparseWitness;
    dev_msm_rows(c, *gens.dev, {.dense = Z, .n_dense = s.R, .rows = s.L, .sparse = sparse});
    c.sync();
    std::vector<CPoint> out(s.L);
    memcpy(out.data(), c.h_points, 32 * s.L);
    return out;
}
// Rank interleave of a sharded proof: element e of rank r's share is element e G + r of the whole.  `all` holds the G ranks' blocks of
// per_rank elements each (an allgather's result); the share starts `off` elements into every block.
inline void interleave_ranks(Fr *out, const Fr *all, size_t G, size_t per_rank, size_t off, size_t len) {
    for (size_t r = 0; r < G; r++) for (size_t e = 0; e < len; e++) out[e * G + r] = all[r * per_rank + off + e];
}
// a batch of product circuits of one size: layer k of circuit i is (left, right) = store + off[k] + {0, n >> (k + 1)}.
// Sharded (G ranks, rank rk): the device holds this rank's residue class of every layer whose sides have at least G elements (element i' here
// is element i' G + rk there: every layer pairs i with i + side / 2, a multiple of G) — n_dev = n / G elements per circuit input, nl_dev layers;
// the few layers above them (sides shorter than G) exist on the host only.  small[k][i] = (left, right) of layer k in full, for every layer
// the host plays by itself (sides of at most kSmallSide elements), gathered from the ranks or computed from the layer below.
constexpr size_t kSmallSide = 256;                          // >= the longest host tail (2^OTTI_PC_LGT_*: 64 / 128 by default, hosttail.h takes up to 256)
struct Circuits {
    size_t n = 0, nl = 0; int count = 0;
    int G = 1, rk = 0; size_t n_dev = 0, nl_dev = 0;
    std::vector<Fr *> store; std::vector<size_t> off;
    std::vector<std::vector<std::pair<std::vector<Fr>, std::vector<Fr>>>> small;   // [layer][circuit], filled by gather_small() when sharded
    void init(int cnt, size_t n_, SnarkScratch &W, size_t first_slot, int G_ = 1, int rk_ = 0) {
        n = n_; count = cnt; nl = std::max<size_t>(1, ilog2(n)); G = G_; rk = rk_; n_dev = n / (size_t)G; nl_dev = std::max<size_t>(1, ilog2(n_dev));
        store.resize(cnt); off.assign(nl_dev, 0);
        size_t o = 0; for (size_t k = 0; k < nl_dev; k++) { off[k] = o; o += n_dev >> k; }
        for (int i = 0; i < cnt; i++) store[i] = W.get(first_slot + i, o);
    }
    size_t side(size_t k) const { return n >> (k + 1); }                 // GLOBAL elements per side of layer k
    size_t side_dev(size_t k) const { return n_dev >> (k + 1); }         // ... of which this rank holds
    Fr *left(int i, size_t k) { return store[i] + off[k]; }
    Fr *right(int i, size_t k) { return store[i] + off[k] + (n_dev >> (k + 1)); }
    Fr *input(int i) { return store[i]; }                     // layer 0: the hashed vector itself, left half then right half
    void build(DevCtx &c) {                                   // ProductCircuit::new: compute_layer, all circuits of the batch per launch
        for (size_t k = 1; k < nl_dev; k++) {
            LayerList L; L.n = count;
            for (int i = 0; i < count; i++) { L.in_left[i] = left(i, k - 1); L.in_right[i] = right(i, k - 1); L.out_left[i] = left(i, k); L.out_right[i] = right(i, k); }
            dev_prod_layer(c, L, n_dev >> (k + 1));
        }
    }
    void gather_small(DevCtx &c, ShardComm &sh);              // sharded: the layers the host plays alone, in full on every rank
};
struct DotpTables { Fr *l[6], *r[6], *w[6]; size_t len = 0; int n = 0; };

// ProductCircuitEvalProofBatched::prove (snark_pc.cpp).  tail_allowed: whether the persistent tail may run at all — false inside a sharded
// proof (snark_prove_resident); beyond that pc_knobs asks the device, OTTI_PC_TAIL and pc_tail_timed_out().
ProductCircuitEvalProofBatched pcbatch_prove(DevCtx &c, Circuits &C, const std::vector<Fr> &evals, DotpTables *D, const std::vector<Fr> &dotp_evals, Transcript &tr,
                                             Fr *pyr, std::vector<Fr> &rand_out, bool tail_allowed, ShardComm *sh = nullptr, const std::function<void()> *on_start = nullptr);
// a persistent tail never answered (TailTimeout): the process goes on with a launch per round.  The setter returns what the flag was.
bool pc_set_tail_timed_out();
bool pc_tail_timed_out();

}  // namespace otti
