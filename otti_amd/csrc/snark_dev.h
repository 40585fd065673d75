// Device-side interface of SNARK mode's kernels (k_snark.hip) for snark_encode.cpp, snark_pc.cpp and snark_prover.cpp.
#pragma once
#include "device.h"
#include "pc_plan.h"

namespace otti {

constexpr int kMaxInst = 20;                                  // 12 product circuits + 6 dot-product halves in the largest batch
// Places in the pinned result buffer (c.h_results) and scratch sizes that the prover and the kernel-level test entries must agree on
constexpr int kSumSlot = 64;                                  // where a round's sums land (kPcTailSlot, where a layer's exported tables start: pc_plan.h)
constexpr size_t kSnarkPartials = (size_t)3 * kMaxBlocks + 64;   // dev_dot_many / dev_sum3 scratch: 3 sums x at most kMaxBlocks workgroups per launch (pc_plan.h pc_round_grid)
// The grid of k_pc_round, k_dot_many and k_sum3 over `ninst` instances of `items` items (pc_plan.h pc_round_grid) under the block cap in force,
// and the tests' seam in it: max_blocks in the place of kMaxBlocks for every later launch (0: the device's own again; never above kMaxBlocks)
PcGrid pc_grid(size_t items, int ninst);
void pc_grid_cap_override(unsigned max_blocks);
struct AbcList { const Fr *A[kMaxInst], *B[kMaxInst], *C[kMaxInst]; int n; };
struct PtrList { Fr *p[64]; int n; };
struct LayerList { const Fr *in_left[16], *in_right[16]; Fr *out_left[16], *out_right[16]; int n; };

// one round of the layered sum-check over a batch of instances: A, B of every instance are folded in place; C[y] == nullptr means the
// instance's third table is the shared eq table, which is never stored (EqSrc, as in phase one of the R1CS proof)
struct PcList { Fr *A[kMaxInst], *B[kMaxInst], *C[kMaxInst]; int n; };
// Sums S_t (t = 0, 2, 3) of instance y land in c.h_results[slot + 3 y ..] once c.wait_ticket(ticket) returns:
//   C[y] given: S_t = sum_i (A_t B_t C_t)[i];  shared eq: S_t = sum_i E[i] (A_t B_t)[i]  (the host applies the bound variable's factor)
unsigned long long dev_pc_eval(DevCtx &c, const PcList &L, size_t len, const EqSrc &E, int slot);
// r == nullptr: an ARMED launch (device.h) — the fold challenge is the next value the host publishes with c.go()
unsigned long long dev_pc_fold_eval(DevCtx &c, const PcList &L, size_t len, const Fr *r, const EqSrc &E, int slot);   // len >= 4: folds to len / 2 first
// the tables (folded by r first when fold is set) go to pinned host memory: table t of instance y at c.h_results[slot + (3 y + t) * len_out ..)
unsigned long long dev_pc_export(DevCtx &c, const PcList &L, size_t len, bool fold, const Fr *r, int slot);

// ---- the persistent tail of a layer's batched sum-check (k_pc_tail): ONE launch plays every round from the point where the tables of
// an instance fit the LDS of W workgroups (kTailCap elements per table and workgroup) down to the host-played tail.  Workgroup (w, y)
// holds the elements i = w (mod W) of instance y's tables (bound_poly_var_top pairs i with i + len/2: always in the same residue
// class) in LDS for the whole launch; per round it mails its three partial sums to its own TailMail line in pinned host memory, waits
// for the challenge (an armed fetch per round: consecutive go() numbers), folds in LDS.  The eq table of a product-circuit instance
// is materialised in LDS here (a real third table, folded like the others; the host multiplies by the factor accumulated before).
// No launch, no HBM round trip, no inter-workgroup hand-off per round: a round costs the host's hash plus ~3 us of arithmetic.
constexpr int kTailThreads = 1024;                            // (kTailCap, kTailMaxGroups: pc_plan.h, with the rule that picks W and the first round)
// The line itself (128 bytes per workgroup, one store instruction, no fence; number and tag): TailMail in mail.h.
// rounds played = log2(len0 / t_out) (>= 1).  Round j's partial sums of workgroup (w, y) arrive in c.tail_mail.host[y * W + w] with seq = first_seq + j;
// after the last fold the tables (t_out elements each) go to c.h_results[slot + (3 y + t) * t_out ..) and every workgroup posts first_seq + rounds.
// fold_r: the source tables hold 2 * len0 elements and are folded by *fold_r on load (nullptr: they hold len0 elements as they are).
// Consumes `rounds` go() values.  Returns first_seq.
unsigned long long dev_pc_tail(DevCtx &c, const PcList &L, int W, size_t len0, size_t t_out, const Fr *fold_r, const EqSrc &E, int slot);

void dev_gather(DevCtx &c, const Fr *table, const uint32_t *idx, Fr *out, size_t n);
void dev_u32_to_fr(DevCtx &c, const uint32_t *in, Fr *out, size_t n);        // out[i] = in[i] as a field element (Montgomery form)
// ---- the decommitment's address and value parts from entry lists in HBM (k_snark.hip k_decomm_fill), `count` matrices in one launch.  Per matrix:
// nv entries (row, col, val), then the explicit padding (i, pad_col, 0) up to len, then zeros up to N; nv <= len <= N.  Outputs of N elements each:
// the addresses as u32 and as field elements (Montgomery form), the values.  Only queues.
struct DecommFillMat { const uint32_t *row, *col; const Fr *val; uint32_t *row_addr, *col_addr; Fr *row_fr, *col_fr, *val_fr; size_t nv, len; uint32_t pad_col; };
struct DecommFill { DecommFillMat m[3]; };
void dev_decomm_fill(DevCtx &c, const DecommFill &f, int count, size_t N);
// ---- sparse_mlpoly.rs AddrTimestamps::new for one side (rows) or both (rows, columns) of the dense representation, in one run of launches.
// Per side three address lists of N entries with values below M; walking k = 0, 1, 2 and i = 0 .. N - 1 in order over ONE counter array shared by
// the three lists, read_ts[k][i] = audit[addr[k][i]]++.  Entries at and beyond len[k] (the same on both sides) must be address 0: they are not
// sorted but ranked in closed form.  Results are those of the sequential walk, bit for bit, for any input (a stable radix sort by address:
// k_snark.hip).  Outputs as u32 and / or as field elements (Montgomery form), each optional (nullptr).  Returns with the stream idle.
struct AddrTs {
    int sides = 1; size_t N = 0, M = 0;
    const uint32_t *addr[2][3] = {}; uint32_t len[3] = {0, 0, 0};
    uint32_t *ts_u32[2][3] = {}; Fr *ts_fr[2][3] = {};        // N entries each
    uint32_t *audit_u32[2] = {}; Fr *audit_fr[2] = {};        // M entries each
};
void dev_addr_timestamps(DevCtx &c, const AddrTs &a);
void dev_hash_mem(DevCtx &c, const Fr *eval_table, const Fr *audit_ts, Fr *out_init, Fr *out_audit, size_t M, const Fr &r, const Fr &gamma, int G = 1, int rk = 0);   // G ranks: this rank's residue class (M / G elements) of the M-element vectors
void dev_hash_ops(DevCtx &c, const Fr *addr_f, const Fr *deref, const Fr *read_ts, Fr *out_read, Fr *out_write, size_t N, const Fr &r, const Fr &gamma, int G = 1, int rk = 0);
void dev_prod_layer(DevCtx &c, const LayerList &L, size_t q);
// partials: kSnarkPartials elements of scratch.Results arrive in c.h_results[slot ..] once the stream has been synchronised.
void dev_pick0(DevCtx &c, const PtrList &L, int slot);
void dev_dot_many(DevCtx &c, const Fr *E, const PtrList &L, size_t n, Fr *partials, int slot);
void dev_sum3(DevCtx &c, const AbcList &L, size_t n, Fr *partials, int slot);

}  // namespace otti
