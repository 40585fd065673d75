// SNARK mode of the proving path: libspartan's computation commitment (SNARK::encode), R1CSEvalProof and SNARK::{prove, verify}
// [RECALL upstream src/lib.rs (SNARKGens, SNARK), src/r1csinstance.rs (R1CSCommitment, R1CSEvalProof), src/sparse_mlpoly.rs,
// src/product_tree.rs, src/sumcheck.rs (SumcheckInstanceProof::prove_cubic_batched); /root/reference/Spartan is an empty submodule].
// Reached from `spzk verify <files>` WITHOUT --nizk (the reference's run.py passes --nizk, /root/reference/run.py:58,100; BASELINE.json's
// metric names the SNARK).  Host objects and the verifier live in snark_host.cpp, the GPU prover in snark_encode.cpp (encode, attach), snark_pc.cpp (product circuits) and snark_prover.cpp (prove), its kernels in
// k_snark.hip; the R1CS satisfiability proof inside it is the same device code as NIZK mode (prover.cpp r1cs_prove_device).
#pragma once
#include "spartan.h"
#include "verify.h"
#include <algorithm>
#include <vector>
#include <system_error>
#include <functional>
#include <thread>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>

namespace otti {

struct DeviceDecomm;                                         // snark_prover.h: the dense representation resident in HBM
struct RowSumsCache;                                         // prover.cpp: a commitment's points decoded in HBM (snark_verify_many)

// lib.rs SNARKGens: gens_r1cs_sat (the NIZK generators) + gens_r1cs_eval = SparseMatPolyCommitmentGens {gens_ops, gens_mem, gens_derefs},
// three PolyCommitmentGens over ONE SHAKE256 stream (label "gens_r1cs_eval"): a set for m variables is gens_n = P[0 .. R), gens_1.G = P[R],
// h = P[R + 1] with R = 2^(m - m/2).  `eval` holds that stream (and its device window table); the views are stream indices.
struct PcSet { size_t num_vars = 0, L = 0, R = 0; uint32_t h_n = 0, g1 = 0, h1 = 0; };
struct SnarkGens {
    std::unique_ptr<Gens> sat, eval;
    PcSet ops, mem, derefs;
    size_t num_cons = 0, num_vars = 0, num_inputs = 0;       // padded, as the instance will have them
};
std::unique_ptr<SnarkGens> snark_gens_new(size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_nz_entries);

// lib.rs ComputationCommitment (+ ComputationDecommitment when made by encode)
struct CompComm {
    size_t num_cons = 0, num_vars = 0, num_inputs = 0;       // R1CSCommitment
    size_t batch_size = 3, num_ops = 0, num_mem_cells = 0;   // SparseMatPolyCommitment
    std::vector<CPoint> comm_ops, comm_mem;
    std::shared_ptr<DeviceDecomm> dec;                       // prover side only
    uint64_t dec_gen = 0;                                    // the instance's coefficient generation (Instance::value_gen) dec was last built (encode, attach) or revalued from
    // verifier side: comm_ops and comm_mem decoded in HBM for snark_verify_many's passes, built once by whichever thread first needs them
    // (under row_cache_mu), shared read-only, freed with the commitment
    mutable std::shared_ptr<RowSumsCache> row_cache; mutable std::mutex row_cache_mu;
    std::vector<uint8_t> serialize() const;                  // bincode
    static std::unique_ptr<CompComm> parse(const uint8_t *p, size_t n);
};

// sumcheck.rs SumcheckInstanceProof (CompressedUniPoly per round: c0, c2, c3) / product_tree.rs proofs
struct LayerProofBatched { std::vector<Fr> coeffs; std::vector<Fr> left, right; };     // coeffs: 3 per round
struct ProductCircuitEvalProofBatched { std::vector<LayerProofBatched> layers; std::vector<Fr> dotp_left, dotp_right, dotp_weight; };
struct Evals4 { Fr init, audit; Fr read[3], write[3]; };
// r1csinstance.rs R1CSEvalProof = sparse_mlpoly.rs SparseMatPolyEvalProof
struct EvalProof {
    std::vector<CPoint> comm_derefs;
    Evals4 eval_row, eval_col; Fr dotp_left[3], dotp_right[3];
    ProductCircuitEvalProofBatched proof_mem, proof_ops;
    Fr h_row_addr[3], h_row_read_ts[3], h_row_audit, h_col_addr[3], h_col_read_ts[3], h_col_audit, h_val[3], h_deref_row[3], h_deref_col[3];
    DotProductProofLog pe_ops, pe_mem, pe_derefs;
};
struct SnarkProof {
    NizkProof r1cs;                                          // R1CSProof (its rx, ry are not serialised in SNARK mode)
    Fr inst_evals[3];
    EvalProof eval;
    std::vector<uint8_t> serialize() const;
    static SnarkProof parse(const uint8_t *p, size_t n);     // throws Error(OTTI_ERR_MALFORMED_PROOF)
};

void snark_append_comm(Transcript &tr, const CompComm &c);  // R1CSCommitment::append_to_transcript
// transcript writers shared by the GPU prover and the host verifier (snark_host.cpp), which must hash identical transcripts
void append_unipoly(Transcript &tr, const Fr *c, size_t n);             // UniPoly::append_to_transcript
void append_evals4(Transcript &tr, const Evals4 &e, bool col);          // the four claim_{row,col}_eval_* lines
Fr reduce_evals(std::vector<Fr> v, const std::vector<Fr> &ch);          // the n-to-1 reduction of claimed evaluations: bound_poly_var_bot, last challenge first
// host verifier (snark_host.cpp): SNARK::verify
int snark_verify(const CompComm &comm, const std::vector<Fr> &inputs, const SnarkGens &g, const void *tlabel, size_t tlabel_len, const uint8_t *proof, size_t proof_len);
// R1CSEvalProof::verify as a resumable walk.  Its three variable-base row sums (PolyEvalProof::verify's C_LZ of the derefs, ops and mem
// evaluation proofs, in that order) are the seams: a step ends by NAMING its sum (points and scalars, both alive until the next step has begun) and
// the next step begins with the answer — the point, or the decompress failure, which it throws where RowSum::finish would have.  Between steps
// the object owns no thread when made with deferred_threads = 0 (its group equations then run inside after_mem).  Every step throws VerifyFail; after
// a throw the object is only good for destruction.  evalproof_verify below is begin .. after_mem in sequence with RowSum answering.
struct RowRequest { const CPoint *C = nullptr; size_t n = 0; const Fr *s = nullptr; };
struct RowAnswer { int code = 0; Pt sum; };
class EvalProofVerifier {
public:
    EvalProofVerifier(const EvalProof &E, const CompComm &c, const std::vector<Fr> &rx, const std::vector<Fr> &ry, const Fr evals[3], const SnarkGens &g, Transcript &tr,
                      int deferred_threads = -1, BtEquations *sink = nullptr);   // sink: the group equations over g.eval are stated to it and not run (no threads then)
    RowRequest begin();                                      // step 0: the product-layer and layered sum-check walk; names the sum over comm_derefs
    RowRequest after_derefs(const RowAnswer &a);             // step 1: names the sum over comm_ops
    RowRequest after_ops(const RowAnswer &a);                // step 2: names the sum over comm_mem
    void after_mem(const RowAnswer &a);                      // step 3: the hash layer's closing checks and every deferred group equation
private:
    const EvalProof &E; const CompComm &c; const SnarkGens &g; Transcript &tr;
    Deferred later;
    Fr evals[3]; size_t nm = 0;
    std::vector<Fr> rxe, rye, r_mem_check, claims_ops, claims_dotp, rand_ops, claims_mem, rand_mem;
    // the evaluation proof whose row sum is out
    const DotProductProofLog *pe_pf = nullptr; const PcSet *pe_set = nullptr; std::vector<Fr> Lv, Rv, Rpt; CPoint C_Zr;   // Rpt: the point Rv is the eq table of
    bool trace; std::chrono::steady_clock::time_point t_lap, t_sum;
    void lap(const char *what);
    RowRequest polyeval_begin(const DotProductProofLog &pf, const PcSet &s, const std::vector<Fr> &r, const Fr &Zr, const std::vector<CPoint> &comm);
    void polyeval_end(const RowAnswer &a);
    Fr joint(std::vector<Fr> ev, const char *label_evals, const char *label_ch, const char *label_joint, const std::vector<Fr> &rand, std::vector<Fr> &r_joint);
};
void evalproof_verify(const EvalProof &E, const CompComm &c, const std::vector<Fr> &rx, const std::vector<Fr> &ry, const Fr evals[3], const SnarkGens &g, Transcript &tr);

// ---------------------------------------------------------------------------------------------- many proofs of one commitment (snark_verify_many.cpp)
// results[i] = what snark_verify returns for item i alone with the same commitment, generators and label (an input >= l: OTTI_ERR_INVALID_SCALAR, as
// the C entry reports it) — NOT a random-linear-combination batch: every proof walks the single verifier's own steps and no verdict depends on its
// neighbours.  What the proofs share is their three row sums: all live proofs reach each seam of EvalProofVerifier together, and the calling thread
// sends the sums of one seam to the device in ONE pass (hook below, set by prover.cpp: that file has no HIP in it) — comm_ops and comm_mem, the same
// points for every proof, decoded once per commitment and kept on it.  Sums under kRowSumDeviceMin points, and all of them without a hook, when it
// declines or throws, or under OTTI_VERIFY_HOST, are summed on the host by the workers; the verdicts do not depend on the route.
// `threads` workers (0: kSnarkVerifyManyThreads; at most kVerifyManyMaxThreads; never more than there are proofs) run step 0 (everything snark_verify
// does before the evaluation proof, r1cs_verify_host with its own row sum included) and then each next step of every proof still alive; with one
// worker everything runs on the calling thread.  A proof parked between steps owns no thread: the threads alive depend on `threads`, not on count.
// Live proofs are bounded: the call runs in chunks of kSnarkVerifyManyChunk items (OTTI_SNARK_VERIFY_CHUNK overrides it, for the tests).
// Per chunk, host: the parsed proofs (a few hundred KB each at 2^20) and per proof two eq tables of at most 2^12 scalars; HBM, on the calling
// thread's context, grow-only: 160 bytes per comm_derefs point (chunk * L_derefs of them), 32 per scalar of every sum, 128 per (window, split)
// of a sum — about 25 MB at 2^20 (8192 rows) with 16 proofs — plus, once per commitment and for its lifetime, 96 bytes per point of comm_ops and comm_mem.
constexpr unsigned kSnarkVerifyManyThreads = 4;
constexpr size_t kSnarkVerifyManyChunk = 16, kRowSumDeviceMin = 256;
// req[i].C == comm.comm_ops.data() / comm.comm_mem.data(): the commitment's own points (cached); anything else: that request's own set.
// Runs on the calling thread's context; false: declined, nothing answered.
typedef bool (*RowSumsManyHook)(const CompComm &comm, const RowRequest *req, size_t n, RowAnswer *ans);
extern RowSumsManyHook g_row_sums_many_hook;
void snark_verify_many(const CompComm &comm, const SnarkGens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count, unsigned threads,
                       int32_t *results);
// The staging itself — chunks, the four-step walk, one device pass per seam, parked proofs that own no thread — for both callers.  With chunk_end the
// proofs state their group equations instead of running them: sat holds those over g.sat (r1cs_verify_host), eval those over g.eval (the three
// closing equations of EvalProofVerifier); generator slots are per handle, so the lists stay apart.  Both sinks take product-form runs.
// After a chunk's last step chunk_end gets, on the calling thread, every proof of the chunk whose verdict the walk has not written: walk_code 0 — it
// walked to the end —, or the code it met inside the evaluation proof (the single verifier runs the sat equations before that: it decides).
struct SnarkCollected { size_t item = 0; BtEquations sat, eval; int walk_code = OTTI_ERR_INTERNAL; bool settled = false; };
typedef std::function<void(std::vector<SnarkCollected *> &)> SnarkChunkEnd;
void snark_verify_staged(const CompComm &comm, const SnarkGens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count, unsigned threads,
                         int32_t *results, const SnarkChunkEnd *chunk_end);

// ---------------------------------------------------------------------------------------------- many proofs as one randomised batch (snark_verify_batch.cpp)
// results[i] = what snark_verify returns for item i alone, except that a proof the single verifier rejects is accepted with probability at most
// 2^-120 over the weights (drawn from a RandomTape: seed32, or OS entropy when null).  Item checks, parsing, chunks, the four-step walk and its one
// device pass per seam are snark_verify_many's (snark_verify_staged).  What is hashed stays per proof: the transcript, the sat rounds' combinations,
// the four row sums, the product-circuit walk.  Every group equation that feeds nothing hashed — the sat proof's two per round, the sigma
// equations, the four log dot-product closing equations — is stated to a collecting sink; a closing equation's n generator terms are ONE
// product-form run (batch_terms.h), so the n scalars s never exist on the host.  After a chunk's last step every equation of every collected
// proof gets a weight of its own and ONE sum is formed over the proofs' points and both generator handles: the identity accepts them all; otherwise
// one localisation pass forms each proof's own sum, and only the proofs whose sum is not the identity, or whose points hold one that does not
// decode, are run through snark_verify for their code.  A proof that fails on its walk before the evaluation proof is settled with that code;
// one that fails inside it goes to snark_verify too, which runs the sat equations first.  The sum runs on the device through the hook below
// (prover.cpp sets it: the runs are expanded there, k_msm.hip k_gen_runs) and on the host cores (bt_run_expand) without a device, when it
// declines, under OTTI_VERIFY_HOST or under OTTI_VERIFY_BATCH_SUM=host (read per call: measurements, tests).  OTTI_VERIFY_BATCH_RUNS=0 (read per
// call: measurements) collects without runs: every closing equation's n generator terms are written out on the worker, as for NIZK's batch.
// A handle's side of a sum: a dense scalar per slot of g.P (null: none) plus product-form runs over its first slots.
struct BatchGenSide { const Fr *base; const BtRun *const *runs; size_t nruns; };
struct SnarkBatchSet { const uint8_t *comp32; size_t n; const Fr *scalars; BatchGenSide gen[2]; };    // one proof: n points and scalars; its own sides over g.sat, g.eval
// localise false: sums[0] = sum over all sets + both handles under total[]; set_bad[k] = set k holds a point that does not decode.  localise true — the
// same thread, the same sets, right after: sums[k] = set k's own sum + both handles under its gen[].  false: declined.
typedef bool (*SnarkBatchSumHook)(const Gens *const g[2], const SnarkBatchSet *sets, size_t nsets, const BatchGenSide total[2], bool localise, Pt *sums, uint8_t *set_bad, double *ms);
extern SnarkBatchSumHook g_snark_batch_sum_hook;
constexpr unsigned kSnarkVerifyBatchThreads = 8;            // profiles/snark_verify_batch.md: level with four up to 4 proofs, faster from 8 on, at 2^12, 2^16 and 2^20
void snark_verify_batch(const CompComm &comm, const SnarkGens &g, const void *tlabel, size_t tlabel_len, const VerifyItem *items, size_t count, unsigned threads,
                        const uint8_t *seed32, int32_t *results, otti_verify_batch_info *info);

// GPU (snark_encode.cpp: encode, attach; snark_prover.cpp: prove)
struct SnarkTimings { double ms[10]; };                      // the six R1CSProof stages, [6] derefs commitment, [7] product circuits, [8] hash layer, [9] total
std::unique_ptr<CompComm> snark_encode_gpu(Instance &inst, SnarkGens &g);
// The prover's copy of a commitment that came as bytes: rebuilds the decommitment of `inst` in HBM (the same function SNARK::encode uses) and
// hangs it on `comm`; no commitment MSM unless verify, which recomputes both commitments and compares them with the stored points (a
// difference: Error(OTTI_ERR_BAD_ARG), comm stays as it was).  Dimensions are checked before the device is touched; a commitment that
// already has its decommitment is left alone.
void snark_attach_gpu(Instance &inst, CompComm &comm, SnarkGens &g, bool verify);
// otti_comp_comm_revalue: a commitment with its decommitment brought to the instance's CURRENT coefficients (otti_instance_set_values) without a new
// encode.  Of the 16 N + 2 M committed elements only the 3 N values of comb_ops hold coefficients: dec->part(4, k) is written again — from the lists
// the instance keeps in HBM when it keeps them, else from the host lists, upstream's zero padding kept — and the rows of comm_ops that meet them
// (value_rows.h comm_value_rows) are summed again with the bulk MSM; addresses, timestamps, comb_mem and comm_mem stay, row_cache is dropped, the
// instance's generation recorded.  comm.serialize() then equals a fresh encode's of the revalued instance.  Checks as attach: the dimensions and
// the generators, before the device is touched; a commitment without decommitment is BAD_ARG.
void snark_revalue_gpu(Instance &inst, CompComm &comm, SnarkGens &g);
// SNARK::prove's refusal of a commitment whose decommitment predates the instance's coefficients (BAD_ARG), before any device work
inline void check_comm_generation(const Instance &inst, const CompComm &comm) {
    if (comm.dec && comm.dec_gen != inst.value_gen)
        throw Error(OTTI_ERR_BAD_ARG, "the computation commitment predates the instance's coefficients (otti_instance_set_values): otti_comp_comm_revalue brings it up to date");
}
std::vector<uint8_t> snark_prove_gpu(Instance &inst, CompComm &comm, const uint8_t *vars32, size_t nvars, const std::vector<Fr> &inputs, SnarkGens &g,
                                     const void *tlabel, size_t tlabel_len, const uint8_t *seed32, SnarkTimings *tm);
struct DeviceWitness;                                        // device.h: the assignment resident in HBM (otti_witness_upload)
class ShardComm;                                             // shard.h
// sh != nullptr: this rank's part of ONE proof over the GPUs of a node (every rank passes the same inputs and gets the same bytes): the
// R1CS satisfiability proof sharded as in NIZK mode, the rows of the derefs commitment split over the ranks, the product circuits (hash layer,
// product layers, the device rounds of the batched sum-checks) by residue classes of the element index; the host rounds and the evaluation
// proofs run on every rank alike
std::vector<uint8_t> snark_prove_resident(Instance &inst, CompComm &comm, DeviceWitness &wit, SnarkGens &g, const void *tlabel, size_t tlabel_len,
                                          const uint8_t *seed32, SnarkTimings *tm, ShardComm *sh = nullptr);

}  // namespace otti
