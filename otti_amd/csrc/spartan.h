// Host-side model of the Spartan NIZK objects for the MI355X proving path: instance (sparse A,B,C), generators,
// proof layout, sigma protocols, verifier.  The prover's data-parallel work lives in k_*.hip / prover.cpp.
// Mirrors upstream libspartan's public API for this path [RECALL lib.rs: Instance, VarsAssignment, InputsAssignment,
// NIZKGens, NIZK::{prove,verify}], reached from `spzk verify --nizk` [REF /root/reference/run.py:58, run.py:100].
#pragma once
#include <atomic>
#include <functional>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include <memory>
#include <mutex>
#include <stdexcept>
#include "field.h"
#include "point.h"
#include "hash.h"
#include "hostgroup.h"
#include "../../include/otti_spartan.h"

namespace otti {

struct Error : std::runtime_error { int code; Error(int c, const std::string &m) : std::runtime_error(m), code(c) {} };

inline size_t ilog2(size_t n) { size_t l = 0; while (((size_t)1 << l) < n) l++; return l; }
inline size_t next_pow2(size_t n) { size_t p = 1; while (p < n) p <<= 1; return p; }

// ---------------------------------------------------------------------------------------------- sparse matrices
// 32-bit indices (N, 2V <= 2^31); values are Montgomery-form Fr.  The host keeps the entry list; the access paths of multiply_vec /
// compute_eval_table_sparse (CSR by row / by column) exist in HBM only (device.h DeviceCsrSet, built by k_sparse.hip).
struct SparseMat {
    std::vector<uint32_t> row, col; std::vector<Fr> val;    // entry list in caller order (as upstream's Vec<SparseMatEntry>)
};

struct DeviceInstance;   // device.h / k_sparse.hip
struct DeviceShard;      // device.h / k_sparse.hip: this rank's slice of the instance when one proof runs over several GPUs (shard.h)
struct DeviceGens;       // device.h / k_msm.hip

struct Instance {
    size_t num_cons = 0, num_vars = 0, num_inputs = 0;      // padded cons / vars (powers of two)
    size_t given_cons = 0;                                  // num_cons as passed to Instance::new (SNARK mode: upstream pads 0 / 1 constraints with explicit entries)
    size_t given_vars = 0;                                  // num_vars as passed (the columns behind the variables are shifted by num_vars - given_vars)
    size_t nnz[3] = {0, 0, 0};                              // entries of A, B, C: known without the host lists
    // A, B, C as host lists.  instance_new fills them.  An instance ingested on the device (k_ingest.hip) has `dev` set and the lists EMPTY until a
    // host consumer asks: mat() downloads the entry lists the device copy keeps (DeviceInstance::ent) exactly once, whichever of any number of
    // threads asks first; it never reads the file again.  Every reader goes through mat().
    const SparseMat &mat(int k) const { if (host_lists_pending) std::call_once(host_lists_once, [this] { materialise_host_lists(); }); return M[k]; }
    mutable SparseMat M[3];                                 // (writers: instance_new, materialise_host_lists)
    bool host_lists_pending = false;                        // set once, before the instance is shared; never cleared (call_once is the gate)
    mutable std::once_flag host_lists_once;
    void materialise_host_lists() const;
    mutable std::atomic<bool> host_lists_done{false};       // set behind the download (otti_instance_host_lists_info: asking never triggers it)
    bool host_lists_materialised() const { return !host_lists_pending || host_lists_done.load(std::memory_order_acquire); }
    // how the instance came to be (otti_instance_ingest_info): the circuit file's size and the four laps of a device ingest
    bool ingested_on_device = false; uint64_t circuit_bytes = 0; double ingest_ms[4] = {0, 0, 0, 0};
    std::shared_ptr<DeviceInstance> dev;                    // uploaded lazily on the first GPU prove
    std::shared_ptr<DeviceShard> shard;                     // uploaded lazily on the first sharded prove
    // the coefficient generation (otti_instance_set_values): 0 at creation, +1 per successful replacement.  What was derived from the coefficients
    // and lives outside the instance — a witness's kept products, a computation commitment's decommitment — records the generation it was made at
    uint64_t value_gen = 0;
    double values_ms[3] = {0, 0, 0};                        // the last replacement's laps: staging, convert + validate, place
    // Fr tuple evaluation used by the verifier: (A,B,C)(rx, ry)
    void evaluate(const std::vector<Fr> &rx, const std::vector<Fr> &ry, Fr out[3]) const;
    bool is_sat(const std::vector<Fr> &vars_padded, const std::vector<Fr> &inputs) const;
};
std::unique_ptr<Instance> instance_new(size_t num_cons, size_t num_vars, size_t num_inputs, const otti_entry *A, size_t nA,
                                       const otti_entry *B, size_t nB, const otti_entry *C, size_t nC);
// THE conversion rule, for every kernel and every host loop that takes witness elements or coefficients in (F: OTTI_WIT_*): the raw word — a
// 32-byte format's eight words as they are, an integer's magnitude in words 0 and 1 with neg saying it was below zero — -> the Montgomery element.
// An integer is always a scalar; a negative one is l - |x| and so never small.  A 32-byte word >= l is refused: stored as zero, and counted as
// small as well.  small: the canonical value is below 2^128 (MONTGOMERY32: judged on fr_to_raw of the word).
HD bool fr_raw_below_2p128(const Fr &c) { return (c.v[4] | c.v[5] | c.v[6] | c.v[7]) == 0; }
template <int F> HD Fr wit_convert(Fr raw, bool neg, bool &refused, bool &small) {
    Fr out; refused = false;
    if constexpr (F == OTTI_WIT_I64 || F == OTTI_WIT_U64) {
        if (neg) raw = fr_sub(fr_zero(), raw);                                   // l - |x| (on canonical integers the field subtraction is the integer one mod l)
        small = !neg;
        out = fr_mul(raw, fr_R2());
    } else {
        small = fr_raw_below_2p128(F == OTTI_WIT_CANONICAL32 ? raw : fr_to_raw(raw));
        if (!fr_raw_is_canonical(raw.v)) { out = fr_zero(); refused = small = true; }
        else if constexpr (F == OTTI_WIT_CANONICAL32) out = fr_mul(raw, fr_R2());
        else out = raw;
    }
    return out;
}
// New coefficients for a matrix of a live instance (= otti_coo_values of the C ABI): n elements in val_format (OTTI_WIT_*), val_stride bytes apart
// (never 0 here); val == nullptr: the matrix stays as it is.  instance_set_values_host is the plain route, for an instance whose lists are on the
// host (instance_new, the host zkif load): host arrays converted by the witness rule (a negative I64 is l - |x|), the first refused coefficient in
// the order A, B, C thrown as instance_new throws it with the instance untouched, then M[k].val replaced, dev and shard dropped (rebuilt lazily)
// and the generation bumped.  Nothing in it needs a device.
struct ValuesSource { const void *val; size_t n; int val_format; size_t val_stride; };
void instance_set_values_host(Instance &I, const ValuesSource vals[3]);
// fills I.M from the device's entry lists (set by the device layer; host-only builds have no instance that needs it)
typedef void (*InstanceHostListsHook)(const Instance &I, SparseMat out[3]);
extern InstanceHostListsHook g_instance_host_lists_hook;

// ---------------------------------------------------------------------------------------------- generators
// Every MultiCommitGens upstream derives for this path comes from ONE SHAKE256 stream (label "gens_r1cs_sat"):
// stream point j is P[j].  gens_pc.gens_n = (P[0..R), h=P[R+1]); gens_pc.gens_1 = gens_sc.gens_1 = (P[R], h=P[R+1]);
// gens_sc.gens_3 = (P[0..3), h=P[3]); gens_sc.gens_4 = (P[0..4), h=P[4]).  A commitment is therefore a short list of
// (stream index, scalar) terms over one shared fixed-base table.
struct Term { uint32_t base; Fr s; };
struct GensView { std::vector<uint32_t> G; uint32_t h; };   // indices into P
struct Gens {
    size_t num_vars_padded = 0, R = 0;
    const char *stream = "gens_r1cs_sat";                   // label of the SHAKE256 stream P comes from: with R, the identity of the points P[0 .. R)
    std::vector<Pt> P;
    GensView pc_n, pc_1, sc_1, sc_3, sc_4;
    std::vector<int> small_slot;                            // P index -> slot in small_tables, or -1
    std::vector<FixedBaseTable> small_tables;               // host tables for P[0..4], P[R], P[R+1]
    std::shared_ptr<DeviceGens> dev;                        // device window table, built lazily
    mutable std::shared_ptr<struct GensDecoded> decoded;    // P in the form the variable-base sums read, in HBM (prover.cpp batch_sum_on_device): made once, kept
    Pt commit_terms(const Term *t, size_t n) const;         // host, fixed-base tables only
    PtFe commit_terms_fe(const Term *t, size_t n) const;    // the same, staying in the five-limb form of the sequential path (hostfast.h)
    void commit_terms_c(uint8_t out[32], const Term *t, size_t n) const { Pt p = commit_terms(t, n); pt_encode(out, p); }
    Pt commit_generic(const Fr *v, size_t n, const Fr &blind, const GensView &g) const;   // host MSM (verifier)
};
std::unique_ptr<Gens> gens_new(size_t num_cons, size_t num_vars, size_t num_inputs);
// sum_{i<n} s[i] * g.P[i] from g's resident device window table; false = not available (the caller computes it on the host)
typedef bool (*FixedBaseMsmHook)(const Gens &g, const Fr *s, size_t n, Pt &out);
extern FixedBaseMsmHook g_fixed_base_msm_hook;

// a DotProductProofGens inside a generator stream: gens_n.G = P[0 .. R), gens_n.h = P[h_n], gens_1 = (P[g1], h = P[h1])
struct PcView { uint32_t h_n, g1, h1; size_t R; };
std::vector<Pt> derive_generators(const char *label, size_t count);      // MultiCommitGens::new stream

std::vector<Fr> eq_evals_host(const Fr *r, size_t ell);                  // EqPolynomial::evals

// ---------------------------------------------------------------------------------------------- proof layout
typedef uint8_t Cmp[32];
struct CPoint { uint8_t b[32]; };
// PolyCommitment::append_to_transcript, for provers and verifiers of both modes alike
inline void append_poly_commitment(Transcript &tr, const char *label, const std::vector<CPoint> &C) {
    tr.append_message(label, "poly_commitment_begin", 21);
    for (auto &p : C) tr.append_point("poly_commitment_share", p.b);
    tr.append_message(label, "poly_commitment_end", 19);
}
// The verifiers' VARIABLE-base sums  sum_i s[i] * decode(C[i])  over the sqrt(V) row commitments of a polynomial commitment
// (PolyEvalProof::verify: the points come from the proof / the computation commitment, so no table exists for them).  With a device:
// begin() uploads the compressed points and starts their decompression at once — the commitments are known long before the
// scalars, which depend on the last sum-check challenges — and finish() runs the LDS-bucket Pippenger over them (k_msm.hip
// k_msm_var) and combines the windows on the host.  finish() returns 0, or OTTI_ERR_VERIFY_DECOMPRESS when a point does not decode
// (what the host path reports); either call may decline (nullptr / negative) and the caller then does the work on the host cores.
struct RowSumJob;
typedef RowSumJob *(*RowSumBeginHook)(const CPoint *C, size_t n);
typedef int (*RowSumFinishHook)(RowSumJob *job, const Fr *s, Pt &out);   // consumes the job (also on failure); s == nullptr: just drop it
extern RowSumBeginHook g_row_sum_begin_hook;
extern RowSumFinishHook g_row_sum_finish_hook;
struct DotProductProof { CPoint delta, beta; std::vector<Fr> z; Fr z_delta, z_beta; };
struct ZKSumcheckProof { std::vector<CPoint> comm_polys, comm_evals; std::vector<DotProductProof> proofs; };
struct KnowledgeProof { CPoint alpha; Fr z1, z2; };
struct ProductProof { CPoint alpha, beta, delta; Fr z[5]; };
struct EqualityProof { CPoint alpha; Fr z; };
struct DotProductProofLog { std::vector<CPoint> L_vec, R_vec; CPoint delta, beta; Fr z1, z2; };
struct NizkProof {
    std::vector<CPoint> comm_vars;
    ZKSumcheckProof sc1;
    CPoint claims_phase2[4];                                 // Az, Bz, Cz, Az*Bz
    KnowledgeProof pok; ProductProof prod;
    EqualityProof eq1;
    ZKSumcheckProof sc2;
    CPoint comm_vars_at_ry;
    DotProductProofLog polyeval;
    EqualityProof eq2;
    std::vector<Fr> rx, ry;
    std::vector<uint8_t> serialize() const;                  // bincode layout of upstream `NIZK`
    static NizkProof parse(const uint8_t *p, size_t n);      // throws Error(OTTI_ERR_MALFORMED_PROOF)
};

// ---------------------------------------------------------------------------------------------- sigma protocols (nizk/mod.rs)
KnowledgeProof knowledge_prove(CPoint &C, const Gens &g, Transcript &tr, RandomTape &tape, const Fr &x, const Fr &r);
EqualityProof equality_prove(const Gens &g, Transcript &tr, RandomTape &tape, const Fr &v1, const Fr &s1, const Fr &v2, const Fr &s2);
ProductProof product_prove(CPoint &X, CPoint &Y, CPoint &Z, const Gens &g, Transcript &tr, RandomTape &tape, const Fr &x, const Fr &rX,
                           const Fr &y, const Fr &rY, const Fr &z, const Fr &rZ);
void unipoly_from_evals(Fr *c, const Fr *e, size_t n);
Fr unipoly_eval(const Fr *c, size_t n, const Fr &r);

// One round of ZKSumcheckInstanceProof::prove_{quad,cubic_with_additive_term} after the table sums are known.
// The prover's randomness (RandomTape) is a separate transcript that depends only on the seed, so everything derived from it
// alone is drawn and committed for all rounds up front (RoundPre; one batched fixed-base MSM on the device): the per-round
// host work on the sequential Fiat-Shamir path is then 4+1+2+1 fixed-base terms instead of 5+2+2+5+2.
struct RoundPre {
    Fr d[4], r_delta, r_beta;          // DotProductProof::prove draws: d_vec, r_delta, r_beta
    Pt delta; CPoint delta_c;          // commit(d_vec, r_delta) over gens_n, and its compressed form
    Pt bp_h, be_h, rb_h;               // blinds_poly[j]*h_n, blinds_evals[j]*h_1, r_beta*h_1
    PtFe bp_fe, be_fe, rb_fe;          // the same in the host's five-limb form (RoundPre::to_fe)
    void to_fe() { bp_fe = ptfe_from(bp_h); be_fe = ptfe_from(be_h); rb_fe = ptfe_from(rb_h); }
};
struct SumcheckState { Fr claim; CPoint comm_claim; Fr blind_claim; std::vector<Fr> blinds_poly, blinds_evals; std::vector<RoundPre> pre; };
struct RoundPart1 { Fr poly[4]; size_t ne; Fr r_j; };
// draws blinds_poly, blinds_evals and every round's (d_vec, r_delta, r_beta) from the tape in upstream's order
void sumcheck_draw_tape(SumcheckState &st, ScalarSource &tape, size_t num_rounds, size_t ne);
RoundPart1 sumcheck_round_begin(ZKSumcheckProof &pf, size_t j, const Fr *evals, size_t ne, const SumcheckState &st, const Gens &g,
                                const GensView &gn, Transcript &tr);
void sumcheck_round_finish(ZKSumcheckProof &pf, size_t j, const RoundPart1 &p1, SumcheckState &st, const Gens &g, const GensView &gn,
                           Transcript &tr);

// ---------------------------------------------------------------------------------------------- verifier (lib.rs NIZK::verify)
// inst_evals: optional (A,B,C)(rx,ry) computed elsewhere (the device: the O(nnz + N + V) part of verification); NULL => host
// fetch: the values are on their way (an evaluation begun on the device before the call: device.h instance_evaluate_begin) and are
// collected through it at the point where the verifier first needs them, after both sum-checks
typedef std::function<void(Fr out[3])> InstEvalFetch;
int nizk_verify(const Instance &inst, const std::vector<Fr> &inputs, const Gens &g, const void *tlabel, size_t tlabel_len,
                const uint8_t *proof, size_t proof_len, const Fr *inst_evals = nullptr, const InstEvalFetch *fetch = nullptr);
// the same from a parsed proof: everything nizk_verify does behind the count of inputs and NizkProof::parse
int nizk_verify_parsed(const Instance &inst, const std::vector<Fr> &inputs, const Gens &g, const void *tlabel, size_t tlabel_len,
                       const NizkProof &P, const Fr *inst_evals = nullptr, const InstEvalFetch *fetch = nullptr);

// ---------------------------------------------------------------------------------------------- many proofs of one instance (verify_many.cpp)
// results[i] = what nizk_verify returns for item i alone with the same instance, generators and label — NOT a random-linear-combination batch:
// every proof is verified by the single verifier's own steps, and no verdict depends on its neighbours.  What the items share is the circuit: the
// points (rx, ry) of all proofs that parse and fit the instance are evaluated in ONE batched pass on the device (hooks below, set by prover.cpp:
// this file has no HIP in it) when the instance has at least 4096 constraints and a device is present — the rule of the single path; otherwise
// every worker evaluates on the host as nizk_verify does.  `threads` workers (0: kVerifyManyThreads; at most kVerifyManyMaxThreads; never more
// than there are proofs to walk) each walk r1cs_verify_host for their share with a Transcript and a SpinPool::Session of their own — the pool's
// workers() budget shares the helper cores out — and collect their triple once the calling thread, which queued the evaluation before the workers
// started and collects it tile by tile, has their tile's values: the device time hides behind the host rounds, as it does for one proof.  One worker runs on the calling thread itself,
// begin / rounds / finish in the single path's order.  An item whose inputs hold a scalar >= l (inputs32 are canonical bytes), whose count of inputs
// is wrong, whose proof does not parse or whose rx / ry do not fit the instance gets the single path's code for that and takes no part in the
// evaluation.  An exception in a worker becomes its item's code.  The call blocks; its workers are joined before it returns.
struct VerifyItem { const uint8_t *inputs32; size_t ninputs; const uint8_t *proof; size_t proof_len; };
constexpr unsigned kVerifyManyThreads = 4, kVerifyManyMaxThreads = 16;
typedef bool (*InstEvalManyBeginHook)(const Instance &inst, const std::vector<const NizkProof *> &proofs);   // queues on the calling thread; false: declined
typedef long (*InstEvalManyNextHook)(Fr (*out)[3]);   // same thread: waits for the next tile of points and copies its values; how many points are in `out` by now, or -1: failed
extern InstEvalManyBeginHook g_inst_eval_many_begin_hook;
extern InstEvalManyNextHook g_inst_eval_many_next_hook;
void nizk_verify_many(const Instance &inst, const Gens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count,
                      unsigned threads, int32_t *results);

// ---------------------------------------------------------------------------------------------- many proofs as one randomised batch (verify_batch.cpp)
// results[i] = what nizk_verify returns for item i alone, except that a proof the single verifier rejects is accepted with probability at most
// 2^-120 over the weights (drawn from a RandomTape: seed32, or OS entropy when null).  Item checks, parsing and the joint evaluation of A, B, C are
// nizk_verify_many's.  The workers (no background threads) walk the live proofs with a collecting sink (verify.h Deferred::equation): the transcript, the
// hashed combinations and the row sum C_LZ run as ever, every group equation that feeds nothing hashed is appended as its term list instead of run.
// A proof that fails on its walk is settled with that code; one whose rx / ry differ from the transcript's goes to the single verifier, whose
// failure order decides its code.  The calling thread gives every equation of every other proof a weight of its own and forms ONE sum: the
// identity accepts them all; otherwise one localisation pass forms each proof's own sum and only the proofs whose sum is not the identity, or
// whose points hold one that does not decode, are run through nizk_verify_parsed for their code.  The sum runs on the device through the hook
// below (prover.cpp sets it) — at every size: its launches take 0.24 - 0.30 ms whatever the batch, the host cores 1 - 10 ms — and on the host cores
// without a device, when it declines, under OTTI_VERIFY_HOST or under OTTI_VERIFY_BATCH_SUM=host (read per call: measurements, tests).
struct BatchSumSet { const uint8_t *comp32; size_t n; const Fr *scalars; const Fr *gen_scalars; };   // one proof: n distinct points and their scalars; its own generator scalars (ngens)
// localise false: sums[0] = sum over all sets + <gen_total, P>, set_bad[k] = set k holds a point that does not decode (it still contributes whatever
// the decode left).  localise true — the same thread, the same sets, right after: sums[k] = set k's own sum + <its gen_scalars, P>.  false: declined.
typedef bool (*BatchSumHook)(const Gens &g, const BatchSumSet *sets, size_t nsets, const Fr *gen_total, size_t ngens, bool localise, Pt *sums, uint8_t *set_bad, double *ms);
extern BatchSumHook g_batch_sum_hook;
// Both from profiles/verify_batch.md: eight workers are never slower than four beyond the spread and faster from K = 16 on (a worker owns no
// background threads, so eight are steady where eight of nizk_verify_many's are erratic); fewer than three live proofs of an instance of 2^16
// padded constraints or more take nizk_verify_many's path (faster there by 0.2 - 0.3 ms; at 2^12 the batch is, by as much).
constexpr unsigned kVerifyBatchThreads = 8, kVerifyBatchMinLive = 3;
constexpr size_t kVerifyBatchRouteMinCons = (size_t)1 << 16;
void nizk_verify_batch(const Instance &inst, const Gens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count,
                       unsigned threads, const uint8_t *seed32, int32_t *results, otti_verify_batch_info *info);

// ---------------------------------------------------------------------------------------------- prover (prover.cpp; GPU)
struct ProveTimings { double ms[8]; };   // polycommit, multiply_vec, sc_phase_one, eval_table_sparse, sc_phase_two, polyeval, total, (spare)

// synthetic satisfiable instance of SURVEY.md section 8(d)
void synth_r1cs(size_t n, size_t num_inputs, uint64_t seed, std::vector<otti_entry> &A, std::vector<otti_entry> &B,
                std::vector<otti_entry> &C, std::vector<uint8_t> &vars32, std::vector<uint8_t> &inputs32);

void synth_r1cs_compiler_like(size_t n, size_t num_inputs, uint64_t seed, std::vector<otti_entry> &A, std::vector<otti_entry> &B,
                              std::vector<otti_entry> &C, std::vector<uint8_t> &vars32, std::vector<uint8_t> &inputs32);

}  // namespace otti
