/*
 * libottispartan — C ABI of the MI355X-native Spartan NIZK proving path for Otti.
 *
 * Drop-in boundary.  The reference reaches this path in two ways:
 *   - as a process: `spzk verify --nizk X.zkif X.inp.zkif X.wit.zkif`        [REF /root/reference/run.py:52-59, run.py:96-100]
 *   - in-process, as libspartan calls from rust-circ `--action spartan`       [REF /root/reference/run.py:147]
 * The library-level interface those callers bind is upstream libspartan's `src/lib.rs` [RECALL — the Spartan/ submodule is an
 * empty directory in the reference mount, /root/reference/.gitmodules:4-6]; every entry point below names the item it replaces.
 *
 * Conventions: plain pointers and sizes; int32 status (0 = ok, negatives mirror upstream's error enums); inputs are borrowed for
 * the duration of the call; outputs are owned by the library until the matching *_free; no exceptions cross the ABI.
 * Threads: creating, preparing and freeing a handle is single-threaded; once otti_prepare_device has run, instance, generator and
 * witness handles are read-only and any number of threads may PROVE (otti_nizk_prove, otti_nizk_prove_resident) and verify with
 * them concurrently — every calling thread gets its own device context (HIP stream, result mailbox, HBM workspace, helper threads),
 * so their proofs overlap on the GPU; a single proof is a chain of sequential rounds that leaves most of the chip idle.  (Upstream's
 * prover is likewise re-entrant: `NIZK::prove(&inst, .., &gens, ..)` borrows instance and generators immutably.)  All scalars are 32-byte canonical little-endian encodings of GF(l),
 * l = 2^252 + 27742317777372353535851937790883648493, unless a comment says "Montgomery" (the in-HBM layout: value*2^256 mod l).
 */
#ifndef OTTI_SPARTAN_H
#define OTTI_SPARTAN_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* upstream R1CSError / ProofVerifyError [RECALL src/errors.rs] */
enum {
    OTTI_OK = 0,
    OTTI_ERR_NON_POW2_CONS = -1,
    OTTI_ERR_NON_POW2_VARS = -2,
    OTTI_ERR_INVALID_NUM_INPUTS = -3,
    OTTI_ERR_INVALID_NUM_VARS = -4,
    OTTI_ERR_INVALID_SCALAR = -5,
    OTTI_ERR_INVALID_INDEX = -6,
    OTTI_ERR_VERIFY_INTERNAL = -10,       /* ProofVerifyError::InternalError */
    OTTI_ERR_VERIFY_DECOMPRESS = -11,     /* ProofVerifyError::DecompressionError */
    OTTI_ERR_MALFORMED_PROOF = -12,       /* bincode deserialisation failure */
    OTTI_ERR_NO_DEVICE = -20,             /* no gfx950 device / HIP failure: the proving path has no CPU fallback */
    OTTI_ERR_BAD_ARG = -21,
    OTTI_ERR_IO = -22,                    /* zkInterface file unreadable / malformed */
    OTTI_ERR_INTERNAL = -23
};

/* one non-zero of A, B or C: upstream `(usize, usize, [u8; 32])` tuples passed to Instance::new */
typedef struct { uint64_t row; uint64_t col; uint8_t val[32]; } otti_entry;

typedef struct otti_instance otti_instance;   /* upstream `Instance` */
typedef struct otti_gens otti_gens;           /* upstream `NIZKGens` */

/* flags for otti_nizk_prove */
#define OTTI_FLAG_GPU 0x1u                    /* required: the only proving backend */

/* Instance::new(num_cons, num_vars, num_inputs, &A, &B, &C) -> Result<Instance, R1CSError>.
   Pads cons/vars to powers of two, shifts columns >= num_vars by the padding, rejects bad indices / non-canonical scalars. */
int32_t otti_instance_new(uint64_t num_cons, uint64_t num_vars, uint64_t num_inputs,
                          const otti_entry *A, size_t nA, const otti_entry *B, size_t nB, const otti_entry *C, size_t nC,
                          otti_instance **out);
void    otti_instance_free(otti_instance *inst);
/* padded sizes as seen by the prover (Instance.inst.get_num_cons / get_num_vars / get_num_inputs) */
int32_t otti_instance_dims(const otti_instance *inst, uint64_t *num_cons, uint64_t *num_vars, uint64_t *num_inputs);
/* Instance::is_sat(&vars, &inputs) -> Result<bool, R1CSError>.  The HOST form: one thread over host byte arrays, a yes or no.  spzk does
   not call it; the check on the device, on the assignment already uploaded and with a diagnosis, is otti_witness_check_sat below. */
int32_t otti_instance_is_sat(const otti_instance *inst, const uint8_t *vars32, size_t nvars, const uint8_t *inputs32, size_t ninputs,
                             int32_t *sat);

/* NIZKGens::new(num_cons, num_vars, num_inputs) */
int32_t otti_gens_new(uint64_t num_cons, uint64_t num_vars, uint64_t num_inputs, otti_gens **out);
void    otti_gens_free(otti_gens *gens);
/* compressed generator stream P[0 .. count) (tests pin it against SURVEY App. B) */
int32_t otti_gens_points(const otti_gens *gens, uint8_t *out32, size_t count);
/* the device-side fixed-base window table of these generators, once built (otti_prepare_device or the first proof): window width c
   (OTTI_MSM_WINDOW pins it; otherwise the widest whose table fits OTTI_MSM_TABLE_GB, default 128) and its size; zeros before that.
   No reference counterpart: dalek's vartime MSM builds per-call tables. */
int32_t otti_gens_table_info(const otti_gens *gens, uint32_t *window_bits, uint64_t *table_bytes);
/* frees the device-side window table (tens of GB); it is built again by the next otti_prepare_device or proof with these generators.
 * For a process that moves between instance sizes: two wide tables do not fit one card.  Not while a proof with them is running. */
int32_t otti_gens_release_device(otti_gens *gens);
/* one device table for several generator handles: `gens` drops whatever table it has and from then on uses `donor`'s (shared ownership; a
 * donor without a table gets one built as otti_prepare_device would build it).  Every NIZKGens takes its points from one stream, P[0 .. R),
 * P[R], P[R + 1] being stream points 0 .. R + 1, and the table is laid out base by base, so the table of the longer handle holds every entry
 * a shorter one looks up.  Proof bytes do not depend on the table: a proof, a kernel entry (otti_k_*) and kept rows give the same bytes before
 * and after.  Afterwards otti_gens_table_info(gens) reports the donor's window width and bytes.  Again with the same donor: OTTI_OK, nothing done.
 * Refusals, before any device is touched: OTTI_ERR_BAD_ARG for a null handle, for gens == donor, for a donor of another stream label and for a
 * donor with fewer points than gens needs; then OTTI_ERR_NO_DEVICE.
 * Release and free: otti_gens_release_device and otti_gens_free on any sharer drop that handle's reference only; the table is freed with
 * its last reference.  A handle that released (donor or adopter) builds a table of its own the next time it needs one.  A witness's kept rows
 * belong to the points and stay valid.
 * Threads: a prepare-class call — single-threaded, and never while a proof with either handle is running.
 * SNARK generators (otti_snark_gens) share nothing. */
int32_t otti_gens_adopt_table(otti_gens *gens, otti_gens *donor);
/* *d_table: the device address of the table these generators use, NULL when there is none; *users: the number of handles holding that
 * table (0 when there is none).  Either out pointer may be NULL.  Touches no device. */
int32_t otti_gens_table_users(const otti_gens *gens, uint32_t *users, const void **d_table);
/* what building the table took, in ms: the HBM allocations (driver work: differs widely between boxes and between a fresh and a used
 * process) and the upload + fill kernels (proportional to the table); zeros before it has been built */
int32_t otti_gens_build_ms(const otti_gens *gens, double *alloc_ms, double *kernels_ms);

/* NIZK::prove(&inst, vars, &inputs, &gens, &mut Transcript::new(tlabel)) -> NIZK, bincode-serialised.
   VarsAssignment::new / InputsAssignment::new validation (InvalidScalar) happens here.
   seed32: 32 bytes seeding the prover's RandomTape (upstream uses OsRng; NULL => OS entropy).
   stage_ms: optional 8 doubles — polycommit, multiply_vec, sc_phase_one, eval_table_sparse, sc_phase_two, polyeval, total, 0. */
int32_t otti_nizk_prove(otti_instance *inst, const uint8_t *vars32, size_t nvars, const uint8_t *inputs32, size_t ninputs,
                        otti_gens *gens, const uint8_t *tlabel, size_t tlabel_len, const uint8_t *seed32, uint32_t flags,
                        uint8_t **proof, size_t *proof_len, double *stage_ms);
/* The same proof with the witness already resident in HBM (z = vars || 1 || inputs || 0.. in Montgomery form): upload once,
   prove many times.  This is the boundary bench.py times: no PCIe traffic inside otti_nizk_prove_resident except the
   per-round field elements and the compressed points of the proof itself. */
typedef struct otti_witness otti_witness;
int32_t otti_witness_upload(otti_instance *inst, const uint8_t *vars32, size_t nvars, const uint8_t *inputs32, size_t ninputs, otti_witness **out);
void    otti_witness_free(otti_witness *w);
/* ---- the resident assignment filled from where witnesses live: device memory (a solver's output, an otti_kd_* result), machine integers, and
   changed in place.  The resulting z is bit for bit what otti_witness_upload builds from the same values (vars || 0.. || 1 || inputs || 0.. in
   Montgomery form, small_fraction by the same rule: canonical value below 2^128, padding zeros small, a negative I64 not), so every proof from it
   is byte-identical.  Validation runs on the device: a CANONICAL32 / MONTGOMERY32 element whose raw value is >= l gives OTTI_ERR_INVALID_SCALAR
   (no witness is returned, *out is untouched; an update leaves the resident vector exactly as it was); the integer formats cannot fail it.
   Argument errors are reported before any device is touched: OTTI_ERR_BAD_ARG for a null inst / out / wit, a null source with a non-zero count,
   an unknown format, a non-zero stride_bytes below the element size or not a multiple of 8, a device source that is not 8-byte aligned;
   OTTI_ERR_INVALID_NUM_VARS for nvars (or first + count) above the padded num_vars; OTTI_ERR_INVALID_NUM_INPUTS; then OTTI_ERR_NO_DEVICE. */
enum { OTTI_WIT_CANONICAL32 = 0,   /* 32-byte little-endian, must be < l (as otti_witness_upload) */
       OTTI_WIT_MONTGOMERY32 = 1,  /* the in-HBM layout (value * 2^256 mod l), raw value must be < l: what otti_kd_* kernels write */
       OTTI_WIT_I64 = 2,           /* signed 64-bit: x >= 0 -> x, x < 0 -> l - |x| (INT64_MIN included) */
       OTTI_WIT_U64 = 3 };
/* vars in DEVICE memory.  stride_bytes: distance between elements (0 = packed).
   stream: the caller's hipStream_t whose queued work produces d_vars (NULL = the calling thread's library stream): the ingest is ordered after
   what is already queued there (an event recorded on it, which the library's stream waits for).
   NULL names no stream to wait for: a producer on HIP's null (legacy default) stream cannot be named, so its caller synchronises first
   (the library's streams are non-blocking and are not ordered against the null stream).
   Returns after the ingest has finished: d_vars is free again. */
int32_t otti_witness_from_device(otti_instance *inst, const void *d_vars, size_t nvars, int32_t format, size_t stride_bytes,
                                 const uint8_t *inputs32, size_t ninputs, void *stream, otti_witness **out);
/* vars as HOST integers (OTTI_WIT_I64 / OTTI_WIT_U64 only, packed): 8 bytes per variable cross PCIe, widened on the device */
int32_t otti_witness_upload_ints(otti_instance *inst, const void *vars, size_t nvars, int32_t format,
                                 const uint8_t *inputs32, size_t ninputs, otti_witness **out);
/* replaces variables [first, first + count) of a resident witness.  src is host memory (src_on_device = 0) or device memory (then stream as
   above).  Afterwards small_fraction is right again (one recount pass).  Never while a proof or check with this witness is running.
   A device source must not overlap the witness's own vector (the d_z of otti_witness_info): elements are read and written by different
   lanes in no order.  To move a range within z, copy it out first. */
int32_t otti_witness_update(otti_instance *inst, otti_witness *wit, size_t first, const void *src, size_t count, int32_t format,
                            size_t stride_bytes, int32_t src_on_device, void *stream);
/* the resident vector.  d_z holds n = 2 * padded num_vars Montgomery elements, usable with otti_kd_*.
   small_fraction is the share below 2^128 that picks the commitment's MSM variant.  Any out pointer may be NULL. */
int32_t otti_witness_info(const otti_witness *wit, const void **d_z, size_t *n, double *small_fraction);
int32_t otti_nizk_prove_resident(otti_instance *inst, otti_witness *wit, otti_gens *gens, const uint8_t *tlabel, size_t tlabel_len,
                                 const uint8_t *seed32, uint8_t **proof, size_t *proof_len, double *stage_ms);
/* Instance::is_sat on the assignment resident in HBM, with a diagnosis.  *n_unsat: number of constraints with <A_r,z>·<B_r,z> != <C_r,z>.
   rows[0 .. min(n_unsat, rows_cap)): the lowest failing row indices, ascending (indices of the caller's constraints; padding rows never fail).
   abc96 (optional, rows_cap * 96 bytes): canonical <A_r,z>, <B_r,z>, <C_r,z> for each reported row.  kernel_ms optional.
   One pass of the sparse-product kernels that writes a bit per constraint instead of Az, Bz, Cz; the bitmap only comes back when a row
   fails.  Reads the handles only: callable from any thread that may prove, concurrently with proofs.  One GPU (a sharded prover checks
   its replicated witness on its own device).  There is no CPU fallback: OTTI_ERR_NO_DEVICE without a device.
   OTTI_ERR_BAD_ARG: inst, wit or n_unsat NULL, or rows_cap > 0 with rows NULL.  OTTI_ERR_INVALID_NUM_VARS: the witness was uploaded for
   an instance of other dimensions. */
int32_t otti_witness_check_sat(otti_instance *inst, otti_witness *wit, uint64_t *n_unsat,
                               uint64_t *rows, size_t rows_cap, uint8_t *abc96, float *kernel_ms);
/* ---- one proof over several GPUs of one node (no reference counterpart: upstream `spzk` is one process
   [REF /root/reference/run.py:52-59]).  One process per GPU.  Every process calls otti_shard_init with the same segment name (a
   fresh, unique name per job: it names a POSIX shared-memory object, removed again once all ranks are attached), its rank and the
   world size (a power of two, at most the number of witness-matrix rows); then each calls otti_nizk_prove_sharded with the SAME
   instance, witness, generators, label and seed.  Every rank returns the same proof bytes, identical to otti_nizk_prove_resident's.
   While proving, ranks exchange only what the host has to hash anyway (per-round sums, row commitments, the partial L^T Z vector)
   through that segment; the witness is replicated by the caller beforehand (e.g. torch.distributed broadcast over RCCL).
   otti_shard_allgather / otti_shard_allreduce are the exchange primitives themselves (host memory; usable without a GPU). */
int32_t otti_shard_init(const char *segment_name, uint32_t rank, uint32_t world);
int32_t otti_shard_finalize(void);
/* transport of the per-round sums: 0 = node-local mailbox (default), 1 = RCCL ncclAllReduce(ncclUint64, ncclSum) over u64 lanes
   (environment OTTI_SHARD_TRANSPORT=rccl at otti_shard_init; needs the GPU) */
int32_t otti_shard_info(uint32_t *rank, uint32_t *world, uint32_t *transport);
int32_t otti_shard_allgather(const void *mine, size_t nbytes, void *out /* world * nbytes */);
int32_t otti_shard_allreduce(uint8_t *scalars32 /* canonical, in place */, size_t count);
int32_t otti_nizk_prove_sharded(otti_instance *inst, otti_witness *wit, otti_gens *gens, const uint8_t *tlabel, size_t tlabel_len,
                                const uint8_t *seed32, uint8_t **proof, size_t *proof_len, double *stage_ms);
/* NIZK::verify(&self, &inst, &inputs, &mut Transcript::new(tlabel), &gens) -> Result<(), ProofVerifyError> */
int32_t otti_nizk_verify(const otti_instance *inst, const uint8_t *inputs32, size_t ninputs, const otti_gens *gens,
                         const uint8_t *tlabel, size_t tlabel_len, const uint8_t *proof, size_t proof_len);
/* Many NIZK proofs of ONE instance verified in one call: what a verifier that holds one circuit and a pile of proofs makes, instead of one
   otti_nizk_verify per caller thread.
   Verdict rule: results[i] = what otti_nizk_verify returns for (inputs32[i], ninputs[i], proofs[i], proof_lens[i]) with the same instance,
   generators and label — 0 accepted, otherwise that call's code (a proof that does not parse: OTTI_ERR_MALFORMED_PROOF; rx / ry of other lengths
   than the instance's: OTTI_ERR_VERIFY_INTERNAL; a wrong count of inputs: OTTI_ERR_INVALID_NUM_INPUTS; an input >= l: OTTI_ERR_INVALID_SCALAR).
   This is NOT a random-linear-combination batch: every proof goes through the single verifier's own steps, no soundness argument changes and no
   verdict depends on its neighbours.  What the proofs share is the circuit: with a device and at least 4096 constraints, A, B, C are evaluated at
   the points of all proofs that parse in one batched pass, one walk over the matrices per four points (otti_k_instance_evaluate is that pass alone).
   Threading: the call blocks.  Its workers are the library's own: `threads` of them (0: the default, 4; more than 16: OTTI_ERR_BAD_ARG; never more
   than there are proofs) walk the proofs, each with its own transcript and helper session, so the host cores are shared out by the library; they
   are joined before the call returns.  threads = 1, or one proof, runs on the calling thread exactly as otti_nizk_verify does.  Several caller
   threads may call with the same handles at once.
   HBM: the batched evaluation keeps at most 8 points resident: their eq(ry) tables, 2V * 32 * 8 bytes (512 MB at V = 2^20, padded size), and the
   two factors of each eq(rx) table (at most 2^12 + 2^13 scalars: 3.1 MB together; the tables themselves, 32 N bytes per point, are never written),
   plus under 1 MB of partial sums and 96 bytes per proof of results — per calling thread, grow-only and kept across calls.  More proofs run in
   chunks of 8.  Workers that sum row commitments on the device use their own contexts' buffers, as otti_nizk_verify does.
   Returns OTTI_OK when the call ran, whatever the verdicts; *n_rejected (may be NULL) = the number of non-zero results, which otti_last_error
   also names.  OTTI_ERR_BAD_ARG, before anything is touched: a null inst, gens or results; with count > 0 a null inputs32, ninputs, proofs or
   proof_lens array or a null proofs[i] (inputs32[i] may be NULL where ninputs[i] is 0); threads > 16.  count == 0: OTTI_OK, nothing done. */
int32_t otti_nizk_verify_many(const otti_instance *inst, const otti_gens *gens, const uint8_t *tlabel, size_t tlabel_len, size_t count,
                              const uint8_t *const *inputs32, const size_t *ninputs, const uint8_t *const *proofs, const size_t *proof_lens,
                              uint32_t threads, int32_t *results, size_t *n_rejected /* may be NULL */);
/* Many NIZK proofs of ONE instance verified as ONE randomised batch: the group equations that feed nothing hashed — two per sum-check round, the
   six sigma equations and the closing equation of the log dot-product proof with its fixed-base sum over the R generators — are not checked
   proof by proof but collected as term lists  sum_j s_j P_j = identity  and summed, for all proofs at once, in one multi-scalar multiplication
   (otti_k_batch_sum is the device pass alone).  What is hashed stays per proof: the transcript, the combinations inside the rounds, the row sum.
   Verdict rule: results[i] = what otti_nizk_verify returns for item i alone with the same instance, generators and label, code for code, with ONE
   exception: a proof that otti_nizk_verify rejects is accepted with probability at most 2^-120 over the library's own randomness (the bound is
   1 / l < 2^-252 per call: each equation of each proof has a weight of its own, a full scalar, so no two defects can cancel).  A valid proof is
   never rejected.  seed32: NULL = OS entropy.  A caller's seed exists only so that tests can repeat a run: a seed the prover could know or guess
   FORFEITS SOUNDNESS — never pass one in production.
   How verdicts are reached: a proof that fails on its walk (a scalar check, a point that does not decode on the hashed path) has that code; if
   the one sum over all other proofs is the identity, all of them are accepted; if not, one localisation pass forms each proof's own sum over the
   points already decoded, and only the proofs whose sum is not the identity, or that hold an undecodable point, are run through the single
   verifier for their code (so are proofs whose rx / ry differ from the transcript's challenges).  A batch with a bad proof therefore costs one
   more sum and one single verification per culprit.
   Refusals, their order, count == 0, threads (0: the default, 8; more than 16: OTTI_ERR_BAD_ARG), *n_rejected and the otti_last_error wording
   are otti_nizk_verify_many's.  The workers own no background threads.  Several caller threads may call with the same handles at once.
   Where the sum runs: on the device when one is present (the proofs' distinct points go up once, one decode launch, one sum launch; the
   generators take part as a set decoded once per generators handle and kept on it), on the host cores otherwise or under OTTI_VERIFY_HOST.
   Decided from tools/verify_batch_probe.py on an MI355X (profiles/verify_batch.md has the tables): the default is EIGHT workers — never slower
   than four beyond the spread, faster from 16 proofs on, and steady, where eight of otti_nizk_verify_many's workers are erratic; the sum runs on
   the device at EVERY size (its launches take 0.24 - 0.30 ms from 260 points to 13 000, the host cores 1 - 10 ms; OTTI_VERIFY_BATCH_SUM=host,
   read per call, forces the host: measurements, tests); and a call with FEWER THAN THREE live proofs of an instance of at least 2^16 padded
   constraints takes otti_nizk_verify_many's path (faster there by 0.2 - 0.3 ms, while at 2^12 the batch is faster by as much;
   info.routed_to_many = 1; OTTI_VERIFY_BATCH_RULE=0, read per call, sets this routing aside).  Against
   otti_nizk_verify_many with its four workers the batch is level at 4 proofs, 1.4 - 2.0 x faster at 16 and 2.0 - 3.5 x at 64; a batch with one
   bad proof costs 2 - 6 ms more than a good one.
   HBM: per calling thread, grow-only and kept across calls: 128 bytes per distinct point (about 25 per sum-check round and proof), 32 per
   scalar (twice when a localisation pass runs), 128 per (window, split) of a job; per generators handle 96 bytes per generator.
   info (may be NULL) is filled whenever the call ran. */
typedef struct {
    uint32_t live;                  /* proofs that parsed and fit the instance */
    uint32_t equations, points;     /* group equations collected; distinct points sent to the sum (over all proofs that reached it) */
    uint32_t gen_slots;             /* generator slots that carry a merged scalar */
    uint32_t on_device;             /* 1: the sum ran on the device, 0: on the host cores */
    uint32_t accepted_first_pass;   /* 1: the one sum was the identity and every proof in it was accepted */
    uint32_t localise_passes;       /* 0 or 1 */
    uint32_t singles_rerun;         /* proofs run through the single verifier for their code */
    uint32_t workers;
    uint32_t routed_to_many;        /* 1: fewer than three live proofs of a large instance, verified on otti_nizk_verify_many's path; the sum's counters stay 0 */
    double sum_ms;                  /* device-event time of the sum's launches, both passes (0 on the host) */
} otti_verify_batch_info;
int32_t otti_nizk_verify_batch(const otti_instance *inst, const otti_gens *gens, const uint8_t *tlabel, size_t tlabel_len, size_t count,
                               const uint8_t *const *inputs32, const size_t *ninputs, const uint8_t *const *proofs, const size_t *proof_lens,
                               uint32_t threads, const uint8_t *seed32 /* may be NULL */, int32_t *results, size_t *n_rejected /* may be NULL */,
                               otti_verify_batch_info *info /* may be NULL */);
/* Many resident witnesses of ONE instance proved in one call: the prover's counterpart of otti_nizk_verify_many.  results[i], proofs[i] and
   proof_lens[i] are exactly what otti_nizk_prove_resident(inst, wits[i], gens, tlabel, tlabel_len, seeds32[i], ..) returns — with a seed, the same
   bytes; seeds32 NULL, or seeds32[i] NULL: OS entropy.  Each proof is freed with otti_buf_free; a failed item has proofs[i] = NULL, proof_lens[i] = 0.
   What the proofs share: everything a proof computes before its first challenge depends on the witness alone — the unblinded row sums of its
   commitment and Az, Bz, Cz.  The calling thread forms both for chunks of at most 16 witnesses in joint passes (the FRONT HALF): ONE fixed-base
   MSM launch over the rows of all witnesses of a chunk that do not keep rows (one per MSM variant; a joint launch may be a chip-filling one
   where each single launch is a small one), and one walk over A, B, C per four witnesses that do not keep products
   (otti_k_multiply_vec_many is that walk alone, otti_k_prove_front the front half alone).  A chunk in which fewer than two witnesses lack a
   thing gets no joint pass for it.  The sequential halves then run on the library's own workers.
   Where the joint passes run follows from measurements (profiles/prove_many.md): up to 2^16 padded variables — beyond, a proof's own launches
   hide behind its tape draws and the joint ones cost more wall time than they save — and, for the products, only where the matrices have the
   row-per-quad layout of a compiled circuit (three entries per row and matrix on average, or more).  Elsewhere each proof forms the thing
   itself, as a single proof does; OTTI_PROVE_MANY_RULE=0, read per call, sets this rule aside (measurements, tests).
   Per-item failures do not affect other items: a witness uploaded for other dimensions gives OTTI_ERR_INVALID_NUM_VARS, a wrong input count
   OTTI_ERR_INVALID_NUM_INPUTS.  Returns OTTI_OK when the call ran; *n_failed (may be NULL) = the number of non-zero results, which
   otti_last_error also names.
   Refusals before anything is touched (outputs stay as they were), in this order: OTTI_ERR_BAD_ARG for a null inst or gens; a null proofs,
   proof_lens or results; with count > 0 a null wits or wits[i]; threads > 16; generators made for another size; then OTTI_ERR_NO_DEVICE.
   count == 0: OTTI_OK, nothing done.
   Handles: the call only reads them — a witness's z, kept rows, kept products and counters are as before.  One handle may appear several times.
   Several caller threads may call with the same handles at once.
   Threads: `threads` counts the calling thread (0: the default, 4, as otti_nizk_verify_many — six and eight were faster in the median but
   showed outliers of several times the median where a process opens four hardware queues, profiles/prove_many.md; never more than count).  threads = 1 or count = 1
   runs everything on the calling thread.  Workers lease pooled device contexts and are joined before the call returns; a worker starts a proof
   once the launches that write its front buffers have completed, so the first proofs run while later tiles are still summed.
   HBM: the front half's buffers live on the calling thread's context, grow-only, kept across calls and reused chunk by chunk: 96 N bytes per
   witness lacking products, 128 L + 32 V per witness lacking rows, one tile of 256 V bytes.  OTTI_PROVE_MANY_GB (read per call; default 8; 0: no
   front half) bounds them by cutting chunks shorter; OTTI_PROVE_MANY_FRONT=0 switches the front half off (A/B runs).  A front half that cannot
   get its memory is no error: the chunk's proofs form their own rows and products (info.front_failed counts such chunks).  Bytes never depend on
   any of this.
   stage_ms[8 i ..] (count * 8 doubles, may be NULL): proof i's own stages as otti_nizk_prove_resident reports them; [0] excludes the front half,
   whose device-event times info.front_ms holds. */
typedef struct {
    uint32_t chunks, product_tiles, row_jobs, workers;
    uint32_t rows_from_front, products_from_front;   /* witnesses whose proof read the front half's rows / products */
    uint32_t front_failed;                           /* chunks whose front half gave up (proofs then formed their own) */
    int32_t  row_kernel[4];                          /* MsmKernel of the first four row jobs (0 bulk, 1 bulk-sparse, 2 small), -1 unused */
    double   front_ms[3];                            /* staging + interleave, row sums, products: device-event time */
} otti_prove_many_info;
int32_t otti_nizk_prove_many(otti_instance *inst, otti_witness *const *wits, size_t count, otti_gens *gens,
                             const uint8_t *tlabel, size_t tlabel_len,
                             const uint8_t *const *seeds32 /* NULL, or seeds32[i] NULL: OS entropy */, uint32_t threads,
                             uint8_t **proofs, size_t *proof_lens, int32_t *results, size_t *n_failed /* may be NULL */,
                             double *stage_ms /* count * 8, may be NULL */, otti_prove_many_info *info /* may be NULL */);
/* ---- SNARK mode (`spzk verify` without --nizk): upstream lib.rs SNARKGens / ComputationCommitment / SNARK [RECALL].
   otti_snark_encode = SNARK::encode (once per circuit: the commitment to A, B, C — on the GPU); otti_snark_prove = SNARK::prove
   (R1CSProof as in NIZK mode + R1CSEvalProof: memory-checking product circuits, batched cubic sum-checks, three polynomial
   evaluation proofs); otti_snark_verify = SNARK::verify, which needs the commitment only (host; sub-linear in the circuit).
   num_nz_entries: the largest number of non-zeros of A, B, C (what spartan-zkinterface passes to SNARKGens::new).
   stage_ms (otti_snark_prove): 10 doubles — the six R1CSProof stages of otti_nizk_prove, [6] derefs commitment, [7] product
   circuits, [8] hash layer, [9] total. */
typedef struct otti_snark_gens otti_snark_gens;      /* upstream `SNARKGens` */
typedef struct otti_comp_comm otti_comp_comm;        /* upstream `ComputationCommitment` (+ `ComputationDecommitment` when made by encode) */
int32_t otti_snark_gens_new(uint64_t num_cons, uint64_t num_vars, uint64_t num_inputs, uint64_t num_nz_entries, otti_snark_gens **out);
void    otti_snark_gens_free(otti_snark_gens *gens);
int32_t otti_snark_encode(otti_instance *inst, otti_snark_gens *gens, otti_comp_comm **out);
int32_t otti_comp_comm_bytes(const otti_comp_comm *comm, uint8_t **out, size_t *len);        /* bincode of the commitment; free with otti_buf_free */
/* A commitment read back from bytes is the verifier's copy: it carries no decommitment.  A prover process that did not run otti_snark_encode
   itself completes its copy with otti_comp_comm_attach below (the decommitment is never stored: rebuilding it from the instance is a few
   device passes, no commitment MSM). */
int32_t otti_comp_comm_from_bytes(const uint8_t *buf, size_t len, otti_comp_comm **out);
/* Rebuilds the decommitment of `inst` on the device and hangs it on `comm`, after which otti_snark_prove* accept it.
   flags 0: trust the caller — only the dimensions (num_cons, num_vars, num_inputs, num_ops, num_mem_cells) are compared, OTTI_ERR_BAD_ARG on a
   mismatch (reported before any device is touched); an instance of the right dimensions but other content then gives proofs the verifier rejects.
   OTTI_ATTACH_VERIFY: also recomputes comm_ops and comm_mem and compares them with the stored points; a difference returns
   OTTI_ERR_BAD_ARG (the message names the commitment) and leaves `comm` without decommitment.
   A commitment that already has its decommitment: OTTI_OK, nothing done.  No device: OTTI_ERR_NO_DEVICE.  One GPU: a sharded prover attaches
   on every rank, each on its own device. */
#define OTTI_ATTACH_VERIFY 0x1u
int32_t otti_comp_comm_attach(otti_comp_comm *comm, otti_instance *inst, otti_snark_gens *gens, uint32_t flags);
/* The sizes a commitment was made for (any out pointer may be NULL).  A verifier builds its generators from these alone:
   otti_snark_gens_new(num_cons, num_vars, num_inputs, num_ops, ..) gives the encoder's generators (they depend on log2 of num_ops only,
   and num_ops = next_pow2 of the encoder's num_nz_entries). */
int32_t otti_comp_comm_dims(const otti_comp_comm *comm, uint64_t *num_cons, uint64_t *num_vars, uint64_t *num_inputs, uint64_t *num_ops,
                            int32_t *has_decommitment);
/* the generator streams as compressed points: which = 0 gens_r1cs_sat, 1 gens_r1cs_eval.  *count receives the stream's length; out32 (room for
   cap points) may be NULL to ask for the length alone */
int32_t otti_snark_gens_points(const otti_snark_gens *gens, int32_t which, uint8_t *out32, size_t cap, size_t *count);
void    otti_comp_comm_free(otti_comp_comm *comm);
int32_t otti_snark_prove(otti_instance *inst, otti_comp_comm *comm, const uint8_t *vars32, size_t nvars, const uint8_t *inputs32, size_t ninputs,
                         otti_snark_gens *gens, const uint8_t *tlabel, size_t tlabel_len, const uint8_t *seed32, uint32_t flags,
                         uint8_t **proof, size_t *proof_len, double *stage_ms);
/* the same with the assignment already resident in HBM (otti_witness_upload): what a long-lived prover calls per proof */
int32_t otti_snark_prove_resident(otti_instance *inst, otti_comp_comm *comm, otti_witness *wit, otti_snark_gens *gens, const uint8_t *tlabel,
                                  size_t tlabel_len, const uint8_t *seed32, uint8_t **proof, size_t *proof_len, double *stage_ms);
/* this rank's part of ONE SNARK::prove over the GPUs of a node (after otti_shard_init, like otti_nizk_prove_sharded: every rank passes the
   same instance, commitment, resident witness, generators, label and seed and receives the same proof bytes): the R1CS satisfiability proof
   sharded as in NIZK mode, the rows of the derefs commitment dealt out over the ranks, the product circuits split by residue classes of the
   element index (their per-round sums cross the ranks); host rounds and evaluation proofs run on every rank alike */
int32_t otti_snark_prove_sharded(otti_instance *inst, otti_comp_comm *comm, otti_witness *wit, otti_snark_gens *gens, const uint8_t *tlabel,
                                 size_t tlabel_len, const uint8_t *seed32, uint8_t **proof, size_t *proof_len, double *stage_ms);
/* ---- kept rows: a resident witness may own the unblinded row sums of its commitment (sum_j z[i * R + j] * G[j] for the L = 2^(ell/2) rows of
   R = 2^(ell - ell/2) variables, num_vars = 2^ell), which depend on the assignment and the generator points alone.  Opt-in per witness; costs
   128 * L bytes of HBM.  Both provers use them: otti_nizk_prove_resident and otti_snark_prove_resident (whose satisfiability part commits to the
   same rows over the same points) then skip the commitment's large MSM launch and only add the blinds; sharded proofs ignore them and compute as
   without.  Proofs are byte-identical with and without kept rows.
   otti_witness_keep_rows builds the generators' window table if need be, sums every row now and returns when the sums are resident;
   _snark takes the SNARK generators' satisfiability stream (the same points for the same sizes: rows kept with either serve both provers).
   Again with generators of the same points: OTTI_OK, nothing done.  The points, not the table, are what the rows belong to: they stay valid
   across otti_gens_release_device.  The generators handle given last must outlive the kept rows (otti_witness_drop_rows / otti_witness_free):
   otti_witness_update sums the rows its range touches again (rows first / R .. (first + count - 1) / R, nothing else) over that handle's table,
   and a refused update leaves the kept rows, like the vector, as they were.  keep_rows, drop_rows and update never run beside a proof with
   this witness; proofs only read the rows, so any number of threads may prove from one witness that keeps them.
   OTTI_ERR_BAD_ARG: a null handle, or generators made for another size than the instance (both before any device is touched); then
   OTTI_ERR_NO_DEVICE; OTTI_ERR_INVALID_NUM_VARS: the witness was uploaded for an instance of other dimensions. */
int32_t otti_witness_keep_rows(otti_instance *inst, otti_witness *wit, otti_gens *gens);
int32_t otti_witness_keep_rows_snark(otti_instance *inst, otti_witness *wit, otti_snark_gens *gens);
/* frees the kept rows: from then on the witness proves as one that never kept them (none kept: OTTI_OK) */
int32_t otti_witness_drop_rows(otti_witness *wit);
/* *kept: 0 or 1; *L, *R: the geometry of the kept rows (0 when none are kept); *rows_resummed: rows summed again by updates since keep_rows.
   Any out pointer may be NULL.  A null wit is OTTI_ERR_BAD_ARG; without a device no witness exists: OTTI_ERR_NO_DEVICE, wit is not looked at. */
int32_t otti_witness_rows_info(const otti_witness *wit, int32_t *kept, size_t *L, size_t *R, uint64_t *rows_resummed);
/* ---- kept products: a resident witness may own Az, Bz, Cz — the row sums <A_r,z>, <B_r,z>, <C_r,z> of its assignment over ONE instance's matrices
   (N = padded num_cons Montgomery elements each, bit for bit what otti_k_multiply_vec gives for the resident z) — with the satisfiability verdict
   of every row (the bitmap of otti_kd_check_sat's layout) and the number of failing rows.  Opt-in per witness; costs 96 * N + N / 8 bytes of HBM.
   The sums are linear in z, and a changed variable j moves only the rows that have an entry in column j.  So once a mutator has written z it
   brings the kept products up to date by recomputing the touched rows alone — otti_witness_update by its range, otti_witness_scatter by its index
   list, otti_witness_assign by the list of elements that changed (nothing changed: nothing launched), otti_witness_set_inputs by the range
   V + 1 .. V + ninputs (inputs are columns of z too) — or, when at least a share of the N rows is touched, by the full pass again
   (profiles/witness_products.md; OTTI_PRODUCTS_FULL_SHARE, read per call, overrides the share: 0 always takes the full pass, >= 1 never).
   otti_nizk_prove_resident and otti_snark_prove_resident over that instance then copy the three vectors instead of forming them, and
   otti_witness_check_sat answers from the kept count and bitmap without a pass (kernel_ms: the report launches for failing rows, 0 if none).
   Proofs and reports are byte-identical with and without kept products.  Sharded provers ignore them (their rows are renumbered per rank), and
   a proof or check with ANOTHER instance computes as without and leaves them alone.
   otti_witness_keep_products runs the full pass now and returns when the products are resident; again for the same instance: OTTI_OK, nothing done;
   for another instance: the old products are dropped and new ones formed.  The instance must outlive the kept products
   (otti_witness_drop_products / otti_witness_free).  A mutator called with another instance than the one the products were kept for returns
   OTTI_ERR_BAD_ARG and changes nothing; any refused mutator call leaves products, bitmap, count and counters exactly as they were (every refusal is
   decided before z is written).  keep_products, drop_products and the mutators never run beside a proof or check with this witness; proofs and
   checks only read, so any number of threads may prove or check from one witness that keeps products.  If a patch cannot run (HBM is short), the
   error is returned with z updated and the products dropped.
   OTTI_ERR_BAD_ARG: a null handle, before any device is touched; then OTTI_ERR_NO_DEVICE; OTTI_ERR_INVALID_NUM_VARS: the witness was uploaded for
   an instance of other dimensions. */
int32_t otti_witness_keep_products(otti_instance *inst, otti_witness *wit);
/* frees the kept products: from then on the witness proves, checks and counts as one that never kept them (none kept: OTTI_OK) */
int32_t otti_witness_drop_products(otti_witness *wit);
/* *kept: 0 or 1; *n_rows: N (0 when none are kept); *d_Az, *d_Bz, *d_Cz: the kept vectors, device pointers usable with otti_kd_* and
   otti_dev_download (read only; NULL when none are kept); *n_unsat: the failing rows; since keep_products: *patches that recomputed listed rows,
   the *rows_recomputed by them, and *full_passes (the first one included).  Any out pointer may be NULL.  A null wit is OTTI_ERR_BAD_ARG; without
   a device no witness exists: OTTI_ERR_NO_DEVICE, wit is not looked at. */
int32_t otti_witness_products_info(const otti_witness *wit, int32_t *kept, size_t *n_rows, const void **d_Az, const void **d_Bz, const void **d_Cz,
                                   uint64_t *n_unsat, uint64_t *patches, uint64_t *rows_recomputed, uint64_t *full_passes);
/* ---- scatter update: variables idx[0 .. count) of a resident witness replaced by src[0 .. count) (format / stride_bytes as otti_witness_update).
   For a caller whose step changes scattered variables (the touched coordinates of an iterate, a handful of cells of a compiled witness): one call,
   whatever rows the indices fall in.  idx: 8-byte unsigned indices, STRICTLY ASCENDING (so none twice), each below the padded num_vars.
   on_device: idx AND src are both host memory (0) or both device memory (1; then `stream` as in otti_witness_update, and both pointers 8-byte
   aligned).  Afterwards z is bit for bit what otti_witness_upload builds from the updated values, and small_fraction is counted again in one pass,
   as by otti_witness_update: equal to a fresh upload's.  Kept rows are not summed again but PATCHED: the commitment is linear, so a changed
   variable j of row i moves the row's sum by (new - old) * G[j - i R] — one table look-up per window of the fixed-base table, count * W in all,
   against R * W for summing a row again; rows_resummed of otti_witness_rows_info does not move, and proofs stay byte-identical.
   Refusals, in this order: OTTI_ERR_BAD_ARG before any device is touched (a null inst / wit, a null idx or src with a non-zero count, an unknown
   format, a bad stride_bytes, a misaligned device pointer); OTTI_ERR_INVALID_INDEX, also before any device, for count above the padded num_vars
   and for a HOST index list that is not strictly ascending or has an element >= the padded num_vars (one pass over it); OTTI_ERR_NO_DEVICE;
   OTTI_ERR_INVALID_NUM_VARS for a witness of other dimensions; then, found on the device, OTTI_ERR_INVALID_INDEX for such a DEVICE index list and
   after it OTTI_ERR_INVALID_SCALAR for a scalar >= l.  A refused call changes nothing: z, small_fraction, the kept rows and every counter stay as
   they were.  count == 0: OTTI_OK, nothing done, no counter moved.  Never while a proof or check with this witness is running; a device source
   must not overlap the witness's own vector.  Sharded provers call it on every rank (their proofs ignore kept rows as before).  If the patch
   cannot run because the generators' table has to be rebuilt and HBM is short, the error is returned with z updated and the kept rows dropped. */
int32_t otti_witness_scatter(otti_instance *inst, otti_witness *wit, const uint64_t *idx, const void *src, size_t count,
                             int32_t format, size_t stride_bytes, int32_t on_device, void *stream);
/* since the witness was made: scatter calls that changed it, kept rows patched by them (distinct idx / R per call, summed), (index, delta) terms
   summed into kept rows; the last two move only while rows are kept.  Any out pointer may be NULL.  A null wit is OTTI_ERR_BAD_ARG; without a
   device no witness exists: OTTI_ERR_NO_DEVICE, wit is not looked at. */
int32_t otti_witness_scatter_info(const otti_witness *wit, uint64_t *calls, uint64_t *rows_patched, uint64_t *terms_patched);
/* ---- assign: variables [first, first + count) of a resident witness set from a WHOLE new vector (src, format, stride_bytes, src_on_device and
   stream as otti_witness_update), of which most elements usually have not moved: what an optimiser, an SGD loop or a re-run compiler emits each
   step.  The library compares the vector with the resident one on the device, by VALUE (-5 as an integer, l - 5 as canonical bytes and the resident
   Montgomery word are the same value), writes only the elements that changed and reports their number in *n_changed (may be NULL).  Afterwards z is
   bit for bit what otti_witness_upload builds from the new values and small_fraction is counted again in one pass: equal to a fresh upload's, so
   proofs are byte-identical.  Kept rows are brought up to date by the changes alone: PATCHED as otti_witness_scatter patches them by the same
   (index, new - old) list (rows_patched and terms_patched of otti_witness_scatter_info move as that scatter would move them; its calls do not), or,
   when so much changed that summing the touched rows again is cheaper (profiles/witness_assign.md; OTTI_ASSIGN_RESUM_SHARE, a share of the touched
   rows' elements read per call, overrides the rule: 0 always sums again, >= 1 never), rows idx_min / R .. idx_max / R are summed again as
   otti_witness_update sums them (rows_resummed of otti_witness_rows_info moves by their number).
   Refusals, in otti_witness_update's order: OTTI_ERR_BAD_ARG before any device is touched (a null inst / wit, a null src with a non-zero count, an
   unknown format, a bad stride_bytes, a misaligned device pointer); OTTI_ERR_INVALID_NUM_VARS for a range beyond the padded num_vars;
   OTTI_ERR_NO_DEVICE; OTTI_ERR_INVALID_NUM_VARS for a witness of other dimensions; then, found on the device, OTTI_ERR_INVALID_SCALAR for a scalar
   >= l.  A refused call changes nothing: z, small_fraction, the kept rows and every counter stay as they were.  count == 0: OTTI_OK, *n_changed = 0,
   no counter moved; nothing changed: OTTI_OK, *n_changed = 0, nothing written, recounted or launched beyond the comparison.
   A device source must not overlap the witness's own vector (d_z of otti_witness_info).  Never while a proof or check with this witness is running.
   Sharded provers call it on every rank (their proofs ignore kept rows as before).  If the kept rows cannot be brought up to date because the
   generators' table has to be rebuilt and HBM is short, the error is returned with z updated and the kept rows dropped, as by otti_witness_scatter. */
int32_t otti_witness_assign(otti_instance *inst, otti_witness *wit, size_t first, const void *src, size_t count, int32_t format,
                            size_t stride_bytes, int32_t src_on_device, void *stream, uint64_t *n_changed);
/* the dry form of otti_witness_assign: *n_changed = the number of elements it would change, and idx[0 .. min(*n_changed, idx_cap)) the lowest of
   their indices, ascending (idx_cap == 0: the count alone, idx may be NULL).  Writes nothing to the witness and moves no counter; it only reads the
   handles, so it may run wherever otti_witness_check_sat may.  Refusals as above, and OTTI_ERR_BAD_ARG also for a null n_changed or idx_cap > 0
   with a null idx. */
int32_t otti_witness_diff(otti_instance *inst, const otti_witness *wit, size_t first, const void *src, size_t count, int32_t format,
                          size_t stride_bytes, int32_t src_on_device, void *stream, uint64_t *n_changed, uint64_t *idx, size_t idx_cap);
/* since the witness was made: otti_witness_assign calls that were not refused (count > 0), elements they changed, and calls that summed kept rows
   again instead of patching them.  Any out pointer may be NULL.  A null wit is OTTI_ERR_BAD_ARG; without a device no witness exists:
   OTTI_ERR_NO_DEVICE, wit is not looked at. */
int32_t otti_witness_assign_info(const otti_witness *wit, uint64_t *calls, uint64_t *changed, uint64_t *resums);
/* replaces the public inputs of a resident witness (z[V + 1 .. V + 1 + ninputs), V the padded num_vars, and the host copy the transcript reads).
   Kept rows cover the variables alone and are untouched, as are small_fraction (it counts the variables) and every counter.
   OTTI_ERR_BAD_ARG: a null handle, or null inputs32 with ninputs > 0; OTTI_ERR_INVALID_NUM_INPUTS: ninputs differs from the instance's;
   OTTI_ERR_INVALID_SCALAR: an input >= l (checked on the host: the witness is unchanged) — all before OTTI_ERR_NO_DEVICE.  Same threads rule. */
int32_t otti_witness_set_inputs(otti_instance *inst, otti_witness *wit, const uint8_t *inputs32, size_t ninputs);
int32_t otti_snark_verify(const otti_comp_comm *comm, const uint8_t *inputs32, size_t ninputs, const otti_snark_gens *gens,
                          const uint8_t *tlabel, size_t tlabel_len, const uint8_t *proof, size_t proof_len);
/* Many SNARK proofs of ONE computation commitment verified in one call: what a verifier that holds one commitment and a pile of proofs makes,
   instead of one otti_snark_verify per caller thread.
   Verdict rule: results[i] = what otti_snark_verify returns for (inputs32[i], ninputs[i], proofs[i], proof_lens[i]) with the same commitment,
   generators and label — 0 accepted, otherwise that call's code (a proof that does not parse: OTTI_ERR_MALFORMED_PROOF; a wrong count of inputs:
   OTTI_ERR_INVALID_NUM_INPUTS; an input >= l: OTTI_ERR_INVALID_SCALAR; dimensions that differ from the generators': OTTI_ERR_VERIFY_INTERNAL; a
   point that does not decode: OTTI_ERR_VERIFY_DECOMPRESS; a proof with several defects gets the single verifier's one code).
   This is NOT a random-linear-combination batch: every proof goes through the single verifier's own steps, no soundness argument changes and no
   verdict depends on its neighbours.  What the proofs share is their row sums: the evaluation proof's three variable-base sums (over comm_derefs,
   comm_ops, comm_mem) are reached by all live proofs together, and with a device every sum of at least 256 points goes there in ONE pass per
   seam — one decode launch, one sum launch (otti_k_row_sum_many is that pass alone) — with comm_ops and comm_mem decoded once per commitment
   and kept on the handle until otti_comp_comm_free.  Smaller sums, and all of them without a device or under OTTI_VERIFY_HOST, are summed on
   the host; the verdicts do not depend on the route.  A proof that fails takes no part in the later passes.
   Threading: the call blocks.  Its workers are the library's own: `threads` of them, the calling thread included (0: the default, 4; more than
   16: OTTI_ERR_BAD_ARG; never more than there are proofs), run the proofs' steps; a proof waiting for its sum owns no thread, so the number of
   threads alive depends on `threads` and not on count.  They are joined before the call returns.  threads = 1, or one proof, runs everything on
   the calling thread.  Several caller threads may call with the same handles at once.
   Memory: the call runs in chunks of 16 proofs.  Per chunk, host: the parsed proofs (a few hundred KB each at 2^20 constraints) and two eq
   tables of at most 2^12 scalars per proof; HBM, on the calling thread's context, grow-only and kept across calls: 160 bytes per comm_derefs point
   of the chunk, 32 per scalar of every sum of a pass and 128 per (window, split) of a sum — about 25 MB at 2^20 with 8192 rows — plus, per commitment
   and for its lifetime, 96 bytes per point of comm_ops and comm_mem (about 1 MB at 2^20).  Workers that sum the R1CS part's row commitments on the device
   use their own contexts' buffers, as otti_snark_verify does.
   Returns OTTI_OK when the call ran, whatever the verdicts; *n_rejected (may be NULL) = the number of non-zero results, which otti_last_error
   also names.  OTTI_ERR_BAD_ARG, before anything is touched: a null comm, gens or results; with count > 0 a null inputs32, ninputs, proofs or
   proof_lens array or a null proofs[i] (inputs32[i] may be NULL where ninputs[i] is 0); threads > 16.  count == 0: OTTI_OK, nothing done. */
int32_t otti_snark_verify_many(const otti_comp_comm *comm, const otti_snark_gens *gens, const uint8_t *tlabel, size_t tlabel_len, size_t count,
                               const uint8_t *const *inputs32, const size_t *ninputs, const uint8_t *const *proofs, const size_t *proof_lens,
                               uint32_t threads, int32_t *results, size_t *n_rejected /* may be NULL */);
/* Many SNARK proofs of ONE computation commitment verified as ONE randomised batch.  The staging is otti_snark_verify_many's: chunks of 16, the
   four-step walk, one device pass per row-sum seam, parked proofs that own no thread.  What differs: the group equations that feed nothing
   hashed — the sat proof's two per round, its sigma equations, and the FOUR log dot-product closing equations (one over the sat generators, three
   over the evaluation generators, each with a fixed-base sum over up to 8192 of them) — are not checked proof by proof but collected as term
   lists and summed, for all proofs of a chunk at once, in one multi-scalar multiplication.  A closing equation's n generator scalars are a
   product form, s[i] = c * prod over the set bits t of i of f[t]: the verifier states lg n + 1 scalars and the device expands them where the sum
   reads them (otti_k_gen_runs is that expansion alone), so they never exist on the host.  What is hashed stays per proof: the transcript, the
   sat rounds' combinations, the four row sums, the product-circuit walk.
   Verdict rule: results[i] = what otti_snark_verify returns for item i alone with the same commitment, generators and label, code for code, with
   ONE exception: a proof that otti_snark_verify rejects is accepted with probability at most 2^-120 over the library's own randomness (each
   equation of each proof has a weight of its own, a full scalar, so no two defects can cancel).  A valid proof is never rejected.  seed32: NULL =
   OS entropy.  A caller's seed exists only so that tests can repeat a run: a seed the prover could know or guess FORFEITS SOUNDNESS — never pass
   one in production.
   How verdicts are reached: a proof that fails on its walk before the evaluation proof has that code; one that fails inside it is run through
   the single verifier, which checks the sat equations first; if a chunk's one sum over all other proofs is the identity, all of them are
   accepted; if not, one localisation pass forms each proof's own sum over the points already decoded, and only the proofs whose sum is not the
   identity, or that hold an undecodable point, are run through the single verifier for their code.
   Refusals, their order, count == 0, threads (0: the default, 8; more than 16: OTTI_ERR_BAD_ARG), *n_rejected and the otti_last_error wording are
   otti_snark_verify_many's.  Several caller threads may call with the same handles at once.
   Where the sum runs: on the device when one is present (each generators handle decoded once and kept on it), on the host cores otherwise, under
   OTTI_VERIFY_HOST or under OTTI_VERIFY_BATCH_SUM=host (read per call: measurements, tests); the verdicts do not depend on the route.
   info (may be NULL) is filled whenever the call ran: its counters add up over the chunks, gen_slots counts the slots of both handles,
   accepted_first_pass says that every chunk's sum was the identity, routed_to_many stays 0.
   Decided from tools/snark_verify_batch_probe.py on an MI355X (profiles/snark_verify_batch.md has the tables, 2^12, 2^16 and 2^20, 2 to 64 proofs):
   the default is EIGHT workers (level with four up to 4 proofs, faster from 8 on); there is NO routing rule, because the batch is ahead of
   otti_snark_verify_many with its four workers in every row, 2 proofs included (at 16 proofs 0.40 - 0.55 of its time); the sum runs on the device
   at every size (0.26 - 0.66 ms per pass).  A batch of 2 - 4 proofs with a bad one among them is slower than otti_snark_verify_many by 2.5 - 6 ms. */
int32_t otti_snark_verify_batch(const otti_comp_comm *comm, const otti_snark_gens *gens, const uint8_t *tlabel, size_t tlabel_len, size_t count,
                                const uint8_t *const *inputs32, const size_t *ninputs, const uint8_t *const *proofs, const size_t *proof_lens,
                                uint32_t threads, const uint8_t *seed32 /* may be NULL */, int32_t *results, size_t *n_rejected /* may be NULL */,
                                otti_verify_batch_info *info /* may be NULL */);
void    otti_buf_free(void *p);
/* copies the calling thread's last error message (NUL-terminated, truncated to cap) */
size_t  otti_last_error(char *buf, size_t cap);

/* upload instance / build the generator window table ahead of the first prove (both are otherwise lazy); with both NULL: only bring
   the HIP runtime and the device context up (a one-shot caller does this on a side thread while it parses its input) */
int32_t otti_prepare_device(otti_instance *inst, otti_gens *gens);
/* number of visible gfx950 devices (0 when none; never initialises a context) */
int32_t otti_device_count(void);
/* Self-test of the host-side fast paths that sit on the prover's sequential Fiat-Shamir path (five-limb GF(2^255-19): point
   compression, fixed-base window tables) against the generic field code and a variable-base multiplication, on `iterations`
   pseudo-random inputs.  0 = consistent.  Needs no GPU; the prover itself only runs on one, so this is how the CPU test suite
   reaches that code. */
int32_t otti_host_selftest(uint32_t iterations);
/* The host's sum of a small MSM's chunk results, as the prover adds the per-workgroup mails of k_msm_small, without a GPU.
 * otti_host_point_from_uniform: a point from 64 uniform bytes (extended coordinates X, Y, Z, T: 4 x 32 bytes little-endian).
 * otti_host_point_sum: the compressed sum of n extended points.  path 0: the generic code; 1: as mails (cached form, number and tag) summed
 * in `parts` ranges with AVX-512 IFMA where the CPU has it; 2: the same with the scalar five-limb additions; 3: as 1 with the last mail
 * left over from an earlier launch (returns OTTI_ERR_INTERNAL: the sum gives up instead of taking it).
 * otti_host_point_sum_bench: nanoseconds per mail summed, out[0] IFMA (0 without it), out[1] scalar. */
int32_t otti_host_point_from_uniform(const uint8_t b64[64], uint8_t out128[128]);
int32_t otti_host_point_sum(const uint8_t *pts128, size_t n, int32_t path, uint32_t parts, uint8_t out32[32]);
int32_t otti_host_point_sum_bench(uint32_t n, uint32_t reps, double out[2]);
/* Measurement aid: nanoseconds per operation of the host primitives on the provers' sequential path, on the calling machine:
 * [0] fixed-base scalar multiplication (8-bit windows), [1] ristretto compression, [2] Keccak-f[1600], [3] transcript append of a point
 * + challenge scalar, [4] GF(l) multiplication, [5] GF(l) inversion, [6] hand-off of an empty task to a helper thread and back,
 * [7] / [8] the two halves of one zero-knowledge sum-check round's host work (up to the challenge / after it), [9] threads used. */
int32_t otti_host_microbench(double out[10]);
/* Measurement aid, no GPU: microseconds per LAYER of the host's last sum-check rounds in SNARK mode (hosttail.h: every round's sums + fold
 * over np product instances and nd triples with tables of T elements, `threads` threads, mean of `reps` layers on random tables):
 * out[0] with the AVX-512 IFMA form (0 when the CPU lacks the instructions or OTTI_HOST_FR8=0), out[1] with the scalar form. */
int32_t otti_host_tail_bench(uint32_t np, uint32_t nd, uint64_t T, uint32_t threads, uint32_t reps, double out[2]);

/* ---- zkInterface ingest (replaces spartan-zkinterface's reader; schema zkinterface 1.x) ---- */
typedef struct {
    uint64_t num_cons, num_vars, num_inputs;
    otti_entry *A, *B, *C; size_t nA, nB, nC;
    uint8_t *vars32; size_t nvars;         /* witness assignment, canonical LE */
    uint8_t *inputs32; size_t ninputs;     /* instance (public input) assignment */
} otti_r1cs;
int32_t otti_zkif_load(const char *circuit_path, const char *inputs_path, const char *witness_path, otti_r1cs **out);
/* the public inputs alone, from the .inp.zkif file (a SNARK verifier that holds the computation commitment has no circuit file): only
   num_inputs, inputs32 and ninputs are filled */
int32_t otti_zkif_load_inputs(const char *inputs_path, otti_r1cs **out);
/* writes the three-file split the reference compiler produces [REF run.py:47-49] from an R1CS in z-order [vars | 1 | inputs] */
int32_t otti_zkif_write(const otti_r1cs *r, const char *circuit_path, const char *inputs_path, const char *witness_path);
void    otti_r1cs_free(otti_r1cs *r);
/* zkInterface files to a ready instance in one call.  *assignment: an otti_r1cs with the dimensions, nA / nB / nC, vars32 and inputs32 filled and
 * A = B = C = NULL (otti_r1cs_free accepts that); without a witness file nvars = 0, as otti_zkif_load leaves it.
 *   OTTI_INGEST_HOST:   otti_zkif_load + otti_instance_new.  Needs no device (a verifier process without a GPU).
 *   OTTI_INGEST_DEVICE: the ConstraintSystem messages are staged through pinned buffers to HBM as they are in the file; kernels walk the FlatBuffers
 *                       tables there, map variable ids to columns, validate and convert the coefficients and write the entry lists in file order,
 *                       from which both CSR copies are built as for any instance.  Headers, Witness, Command and unknown messages, the .inp.zkif
 *                       and the .wit.zkif stay on the host.  The instance comes back with its device copy made and WITHOUT host lists: the first
 *                       host consumer (otti_instance_is_sat, a verifier without a device evaluation, otti_instance_entries) downloads them from
 *                       the device, once, whichever thread asks; SNARK encode / attach and a sharded upload read the lists where they are
 *                       (otti_instance_host_lists_info tells whether the download has happened).  For that the entry lists stay in HBM
 *                       beside the CSR copies for the life of the instance: 40 bytes per entry (otti_instance_ingest_info: hbm_entry_bytes).
 *                       Without a device: OTTI_ERR_NO_DEVICE.  Its own limits, all OTTI_ERR_BAD_ARG: a circuit file of 16 GiB and more or more
 *                       than 2^30 constraints (said before the file is parsed, so before any defect of it: the host path says "too large"
 *                       only behind a clean parse), and a matrix of 2^32 entries and more (offsets in a file may alias, so a few MB can hold
 *                       that many; said behind a malformed table and before any entry is looked at; the host path has no such limit).
 *   OTTI_INGEST_AUTO:   the device when its runtime is already up in this process (the call never brings one up) and the circuit file's size lies
 *                       between a cut-over and a budget: OTTI_INGEST_MIN_MB (MiB; default 15: the smallest size probed, profiles/zkif_ingest.md)
 *                       and OTTI_INGEST_GB (GiB; default 8; 0: never), both read per call.  Otherwise the host.
 * Both paths make the same instance — the same entries in the same order (a SNARK computation commitment depends on it), the same variants in
 * otti_instance_device_info — and report the same error for the same files: a parse error first, the first in file order (OTTI_ERR_IO, an undeclared
 * variable id OTTI_ERR_INVALID_INDEX, a coefficient wider than 32 bytes OTTI_ERR_INVALID_SCALAR), then whatever the
 * inputs and witness files are refused for, then a coefficient >= l (OTTI_ERR_INVALID_SCALAR).
 * Before any device is touched: a null circuit_path, inputs_path, inst or assignment, or an unknown mode, is OTTI_ERR_BAD_ARG; a file that cannot
 * be read OTTI_ERR_IO.  On any error *inst and *assignment are untouched, and after a device-side refusal the context stays usable. */
enum { OTTI_INGEST_AUTO = 0, OTTI_INGEST_HOST = 1, OTTI_INGEST_DEVICE = 2 };
int32_t otti_instance_from_zkif(const char *circuit_path, const char *inputs_path, const char *witness_path /* may be NULL */,
                                int32_t mode, otti_instance **inst, otti_r1cs **assignment);
/* the entries of A (which = 0), B (1) or C (2) as the caller passed them to otti_instance_new, or as otti_zkif_load gives them for the files an
 * instance was ingested from: unpadded columns, canonical values, the same order.  *count (optional) receives their number; out (optional: NULL
 * asks for the count alone, which downloads nothing) needs room for cap >= that many, else OTTI_ERR_BAD_ARG.  Works for every instance. */
int32_t otti_instance_entries(otti_instance *inst, int32_t which /* 0 A, 1 B, 2 C */, otti_entry *out, size_t cap, size_t *count);
/* how an instance came to be: on_device = 1 for a device ingest; the circuit file's size (0 for otti_instance_new); the HBM its kept entry lists
 * take (0 unless on_device); and a device ingest's four laps in ms: host walk + id map, staging + copies, kernels, CSR build.  Any pointer may be NULL. */
int32_t otti_instance_ingest_info(const otti_instance *inst, int32_t *on_device, uint64_t *circuit_bytes, uint64_t *hbm_entry_bytes,
                                  double ms[4] /* host walk + id map, staging + copies, kernels, CSR build */);
/* whether the instance's host entry lists exist: materialised = 1 always for otti_instance_new and the host ingest; for a device ingest only once a
 * host consumer has downloaded them (otti_instance_is_sat, a verifier without a device evaluation, OTTI_DECOMM_HOST=1, otti_instance_entries — SNARK
 * encode / attach and a sharded upload read the lists in HBM and do not).  host_bytes: their size, 40 bytes per entry, 0 while absent.  Asking never
 * triggers the download.  Either out pointer may be NULL; a NULL inst is OTTI_ERR_BAD_ARG. */
int32_t otti_instance_host_lists_info(const otti_instance *inst, int32_t *materialised, uint64_t *host_bytes);
/* ---- an instance from where matrices live as arrays: rows, columns and coefficients of A, B and C, in device memory (a circuit generator's
 * output) or host memory (a compiler's arrays: 16 to 24 bytes per entry with integer coefficients cross PCIe, against otti_entry's 48).
 * The instance is exactly the one otti_instance_new makes from the same triples in the same order: the same padded dimensions, the same shift
 * of columns >= num_vars by the padding, the same entries in caller order (explicit zeros and duplicates kept as otti_instance_new keeps them),
 * the same otti_instance_device_info on both CSR copies, so every NIZK proof and every SNARK computation commitment from it is byte-identical.
 * Coefficients come in the witness formats (OTTI_WIT_*) and become field elements by the witness rule: a negative I64 is l - |x|, INT64_MIN included.
 * Validation runs on the device, in one pass, and reports what otti_instance_new's sequential walk over A, then B, then C meets first, within one
 * entry the row before the column before the scalar, with otti_instance_new's code and otti_last_error wording: OTTI_ERR_INVALID_INDEX for
 * row >= num_cons or col >= num_vars + 1 + num_inputs (a negative index of a signed format is out of range; a 64-bit index is compared in 64 bits
 * before it is narrowed: 2^32 + 3 is never the index 3), OTTI_ERR_INVALID_SCALAR for a CANONICAL32 / MONTGOMERY32 coefficient whose raw value is
 * >= l (the integer formats cannot fail it).  Then no instance is returned, *out is untouched, everything allocated is released and the context
 * stays usable.
 * Argument errors are reported before any device is touched: OTTI_ERR_BAD_ARG for a null mats or out, a null array with a non-zero n, an
 * unknown index or coefficient format, a non-zero val_stride_bytes below the element size or not a multiple of 8, an array (device or host:
 * host arrays are staged as they are) not aligned to its element — 4 or 8 bytes for indices, 8 for every coefficient format —, n >= 2^32, and
 * padded dimensions above 2^30; then OTTI_ERR_NO_DEVICE.
 * src_on_device = 1: the arrays are in HBM; stream as for otti_witness_from_device (the ingest is ordered behind an event recorded on it; NULL
 * names no stream to wait for).  src_on_device = 0: host memory, copied to HBM as it is; the same kernel reads it there.
 * Returns after the ingest has finished: the sources are free again.
 * The result is a device-ingested instance (see otti_instance_from_zkif, OTTI_INGEST_DEVICE): its device copy is made, its entry lists stay in
 * HBM, and the host lists are downloaded by the first host consumer (otti_instance_host_lists_info: materialised = 0 until then).
 * otti_instance_ingest_info reports on_device = 1, the source bytes read (two indices and one coefficient per entry) as circuit_bytes and the
 * laps ms[0] = 0, ms[1] = staging, ms[2] = kernel, ms[3] = CSR build. */
enum { OTTI_IDX_U32 = 0, OTTI_IDX_I32 = 1, OTTI_IDX_U64 = 2, OTTI_IDX_I64 = 3 };
typedef struct {
    const void *row, *col;       /* n indices each, packed, in index_format */
    const void *val;             /* n coefficients in val_format (OTTI_WIT_*), val_stride_bytes apart (0 = packed) */
    size_t n; int32_t index_format, val_format; size_t val_stride_bytes;
} otti_coo;
int32_t otti_instance_from_coo(uint64_t num_cons, uint64_t num_vars, uint64_t num_inputs, const otti_coo mats[3] /* A, B, C */,
                               int32_t src_on_device, void *stream, otti_instance **out);
/* the entry lists a device-ingested instance keeps in HBM, matrix `which` (0 A, 1 B, 2 C): n stored rows (u32), n padded columns (u32: a column
 * >= num_vars moved up by the padding) and n Montgomery values (32 bytes each, usable with otti_kd_*), in caller order.  An instance that keeps
 * no lists (otti_instance_new, the host ingest), and an empty matrix, answer n = 0 with NULL pointers.  The pointers are valid for the life of
 * the instance.  Any out pointer may be NULL; a NULL inst or another `which` is OTTI_ERR_BAD_ARG.  Touches no device. */
int32_t otti_instance_device_entries(const otti_instance *inst, int32_t which, const void **d_row, const void **d_col,
                                     const void **d_val, size_t *n);
/* ---- new coefficients for a live instance, in place: the structure (rows, columns, counts, padded dimensions) stays and every entry of the
 * matrices named gets a new coefficient.  For a caller that emits the same structure with new coefficients per dataset.
 * vals[k] (k = 0 A, 1 B, 2 C): val == NULL (then n must be 0) leaves matrix k as it is.  Otherwise n must equal the matrix's entry count
 * (OTTI_ERR_BAD_ARG), and element i replaces the coefficient of entry i in the order the instance was given its entries (otti_instance_entries
 * order).  Formats (OTTI_WIT_*, a negative I64 is l - |x|), strides, alignment rules, src_on_device, the stream wait and "returns when the
 * sources are free again" are exactly those of otti_instance_from_coo.
 * Errors: a refused coefficient (a CANONICAL32 / MONTGOMERY32 value >= l) is reported as otti_instance_new would report it on the new triples:
 * the first defect walking A, then B, then C, OTTI_ERR_INVALID_SCALAR with its wording.  Argument errors (a null inst or vals, a null val with a
 * non-zero n, an unknown format, a bad stride or alignment, a wrong n) come before OTTI_ERR_NO_DEVICE, which is reported when the call needs a
 * device — the instance keeps its lists in HBM, or src_on_device = 1 — and there is none.  ALL OR NOTHING: after any error the instance is bit
 * for bit what it was (everything is converted and validated into staging first, then placed).
 * On success the instance is the one otti_instance_from_coo or otti_instance_new would make from the old rows and columns with the new
 * coefficients: entries, proofs, the verifiers' evaluate and SNARK commitments are identical, and the sparse-kernel variant is decided again by
 * the same rule, so otti_instance_device_info equals the fresh instance's in both directions of a codes / no-codes flip.
 * An instance that keeps its entry lists in HBM (otti_instance_from_coo, otti_instance_from_zkif with OTTI_INGEST_DEVICE) is revalued there by two
 * streaming kernels.  Its first call also builds the slot maps (where each entry sits in the by-row and the by-column copy: 8 bytes per entry,
 * kept for the life of the instance; an instance that is never revalued pays nothing); later calls only convert and place.  The convert pass's
 * list of small-integer codes (4 bytes per entry of every matrix ever replaced) is kept with the instance likewise, so a later call allocates
 * nothing but the new value list.  The d_val pointer of
 * otti_instance_device_entries changes with every successful call (the staging list becomes the list).  Host lists that were never downloaded
 * stay so (otti_instance_host_lists_info); downloaded ones are refreshed inside the call.
 * Any other instance (otti_instance_new, the host ingest) takes the plain route: converted on the host, the device copy dropped and rebuilt
 * lazily, as after otti_instance_new.  Slow and correct; with host sources it needs no device.
 * Every instance carries a coefficient GENERATION: 0 at creation, +1 per successful call.  State derived from the coefficients follows it:
 *  - a witness's kept products (otti_witness_keep_products) made at another generation are stale: proofs form their own, mutators do not patch
 *    them, otti_witness_products_info says kept = 0, otti_witness_check_sat runs its pass, and otti_witness_keep_products recomputes.  Kept rows
 *    do not depend on the instance and stay.
 *  - a computation commitment records the generation its decommitment was last built (encode, attach) or revalued from; otti_snark_prove* refuses
 *    a commitment whose recorded generation differs from the instance's, with OTTI_ERR_BAD_ARG, before any device work.
 *  - the sharded copy is dropped and rebuilt by the next sharded proof.
 * The caller's rule: no other call on this instance may be in flight, and proofs made before the call remain proofs about the old instance. */
typedef struct { const void *val; size_t n; int32_t val_format; size_t val_stride_bytes; } otti_coo_values;
int32_t otti_instance_set_values(otti_instance *inst, const otti_coo_values vals[3] /* A, B, C */, int32_t src_on_device, void *stream);
/* the generation, whether the slot maps exist and their size (8 bytes per entry, 0 while absent), and the last successful call's laps:
 * ms[0] staging, ms[1] convert + validate, ms[2] place (the plain route: everything in ms[1]).  Any out pointer may be NULL.  Touches no device. */
int32_t otti_instance_values_info(const otti_instance *inst, uint64_t *generation, int32_t *slots_resident, uint64_t *slot_bytes,
                                  double ms[3] /* staging, convert+validate, place */);
/* A computation commitment WITH its decommitment (from otti_snark_encode, or completed by otti_comp_comm_attach) brought to the instance's current
 * coefficients without encoding again.  Of the 16 N + 2 M committed elements only the 3 N values of A, B, C depend on the coefficients: they are
 * written again (from the lists in HBM when the instance keeps them, else from the host lists) and only the rows of comm_ops that meet them are
 * summed again; addresses, timestamps and comm_mem are untouched.  Afterwards otti_comp_comm_bytes equals a fresh otti_snark_encode of the
 * revalued instance and otti_snark_prove* accepts the pair.  OTTI_ERR_BAD_ARG: a null argument, a commitment without decommitment, and the
 * dimensions and generators otti_comp_comm_attach checks — all before the device is touched. */
int32_t otti_comp_comm_revalue(otti_comp_comm *comm, otti_instance *inst, otti_snark_gens *gens);
/* .inp.zkif + .wit.zkif to a resident witness of `inst`, equal in every observable way (z, inputs, small_fraction, proof bytes) to otti_zkif_load on
 * the instance's three files followed by otti_witness_upload.  It works with every consumer and mutator of a resident witness.
 *   OTTI_INGEST_HOST:   the host loader's frame over the two files (the circuit's share left out), then the upload path.
 *   OTTI_INGEST_DEVICE: headers and the inputs file stay on the host, which also locates and checks the ids and values vectors of every Witness
 *                       message; the messages are staged through the circuit ingest's pinned buffers to HBM as they are in the file, and one kernel,
 *                       a thread per assigned variable, reads id and value there (elements of any width: narrower ones zero-extended, of wider ones
 *                       the first 32 bytes, the rest having to be zero), maps the id to its column, refuses a variable assigned twice through a
 *                       bitmap, tests the value against l, converts it by the upload's rule and writes z.  No 32-byte copy of the assignment is
 *                       made on the host.  Its own limit: a witness file of 16 GiB and more is OTTI_ERR_BAD_ARG.
 *   OTTI_INGEST_AUTO:   the device when the witness file has at least OTTI_INGEST_WIT_MIN_MB MiB (read per call; default 10: the smallest size
 *                       probed at which the device path won, profiles/zkif_witness_ingest.md), else the host.
 * The id map is rebuilt from these two files alone (the instance ids and free_variable_id of the inputs header, the witness ids); when the resulting
 * num_vars / num_inputs are not the instance's: OTTI_ERR_BAD_ARG, said behind the checks of the headers, the id map and the number of assigned
 * variables and before any value is looked at.  Every other defect of the files is reported with the code the host pair (otti_zkif_load +
 * otti_witness_upload) gives for the same two files beside a clean circuit, the first in the host pair's order: per Witness message in file order
 * a malformed table or vector (OTTI_ERR_IO), then an element wider than 32 bytes with a non-zero tail (OTTI_ERR_INVALID_SCALAR); the headers'
 * field_maximum and free_variable_id, the instance ids, a count of assigned variables other than num_vars (OTTI_ERR_IO; an instance id 0
 * OTTI_ERR_INVALID_INDEX); an inputs file or a witness message without values (OTTI_ERR_IO); the first assigned id that is 0, an instance id
 * or unknown (OTTI_ERR_INVALID_INDEX); a variable assigned twice (OTTI_ERR_IO); a public input >= l, then a witness value >= l
 * (OTTI_ERR_INVALID_SCALAR).  A refused z is never visible, and after a device-side refusal the context stays usable.
 * Before any device is touched: a null inst, path or out, or an unknown mode, is OTTI_ERR_BAD_ARG; a file that cannot be read OTTI_ERR_IO.  Without
 * a device: OTTI_ERR_NO_DEVICE in every mode (a resident witness lives on one).  On any error *out and *inputs_out are untouched.
 * *inputs_out (optional): an otti_r1cs with only num_inputs, inputs32, ninputs filled, as otti_zkif_load_inputs gives. */
int32_t otti_witness_from_zkif(otti_instance *inst, const char *inputs_path, const char *witness_path, int32_t mode, otti_witness **out,
                               otti_r1cs **inputs_out);
/* the cut-over OTTI_INGEST_AUTO applies at this moment, in MiB: OTTI_INGEST_WIT_MIN_MB when it is set to a number >= 0, else the default */
double  otti_witness_ingest_min_mb(void);
/* how a witness came to be: on_device = 1 when otti_witness_from_zkif read the file on the device; the witness file's size (0 unless it came from
 * otti_witness_from_zkif); and the device path's three laps in ms: host walk, staging + copies, kernel.  Any pointer but wit may be NULL. */
int32_t otti_witness_ingest_info(const otti_witness *wit, int32_t *on_device, uint64_t *witness_bytes, double ms[3] /* host walk, staging + copies, kernel */);
/* synthetic satisfiable R1CS: num_cons = num_vars = n, one non-zero per row per matrix */
int32_t otti_synth_r1cs(uint64_t n, uint64_t num_inputs, uint64_t seed, otti_r1cs **out);
/* second distribution of SURVEY 8d ("compiler-like"): 90 % of the witness < 2^64, 1..8 non-zeros per row, small signed coefficients,
   a heavily used constant column, one 300-entry row */
int32_t otti_synth_r1cs_compiler_like(uint64_t n, uint64_t num_inputs, uint64_t seed, otti_r1cs **out);

/* ---- kernel-level entry points (tests / bench).  h_* = host pointers; elements are 32-byte Montgomery-form Fr.
        Each call stages inputs to HBM, runs the named kernel(s) on the library's stream, and copies results back;
        kernel_ms (optional) receives the HIP-event time of the kernel launches alone. ---- */
/* Fr/Fp/point self-test kernels: out[i] = a[i] * b[i] etc.  op: 0 mul, 1 add, 2 sub */
int32_t otti_k_fr_op(int32_t op, const uint8_t *h_a, const uint8_t *h_b, uint8_t *h_out, size_t n, float *kernel_ms);
/* GF(2^255-19) on the device in one of its three forms (form: 0 the 8-word Fp, 1 nine limbs of 29 bits, 2 ten limbs of 26/25 bits), one case per lane:
   the very inline functions the MSM kernels call.  Operands: n little-endian 256-bit words each (any value: a loosely reduced element).
   op: 0 a*b, 1 a^2, 2 a+b, 3 a-b, 4 -a, 5 carry((a-b)+(c+d)) (form 0: the representative below p), 6 unpack(pack(unpack(a))), 7 (a-b)*(c+d),
   8 (a+a+a)*(b+b), 9 ((a+a)-b)*(c-d), 10 carry((a+a)-b)*((c+c)+d), 11 a^(2^252-3).  Form 1 has no op 1, 9, 11 (OTTI_ERR_BAD_ARG).
   h_out: n packed results; h_limbs: 10 words per case, the raw limbs (form 0: words) of the result before packing, the rest zero. */
int32_t otti_k_fp_op(int32_t form, int32_t op, const uint8_t *h_a, const uint8_t *h_b, const uint8_t *h_c, const uint8_t *h_d, size_t n, uint8_t *h_out,
                     uint32_t *h_limbs, float *kernel_ms);
/* GF(l) in the device's nine limbs of 29 bits (Montgomery radix 2^261), one case per lane: the very inline functions the sum-check, eq-table and sparse
   kernels call.  An operand is n 32-byte words (any 256-bit value, little-endian) or n x 9 raw uint32 limbs, as the operation demands:
   words in, limbs out: 0 unpack, 1 unpack5 (limbs of 32 a), 2 unpack10 (limbs of 1024 a; a < 2^253);
   limbs in, limbs out: 3 mul(a, b) = a b / 2^261 mod l, 4 mul(a, a) with the same registers as both inputs, 5 add, 6 norm (one carry sweep),
   7 .. 11 a - b + K l for K = 2, 4, 8, 16, 128, 12 fold_top, 13 shl5;  limbs in, word out: 14 pack_lt2l, 15 pack_lt3l, 16 canon;
   words in, word and limbs out: 17 pack_lt2l(mul(unpack5(a), unpack(b))), 18 the fold a + c (b - a) of the round kernels (c unpacked times 32): the
   stored word and the limbs handed on.  Operands an operation does not read are ignored but must not be NULL; the output it does not produce is
   zero.  Nothing checks an operation's precondition (fr9.h): that is the caller's.  Before any device work: an unknown op, a null pointer with n > 0
   or n > 2^24 is OTTI_ERR_BAD_ARG; n = 0 returns at once. */
int32_t otti_k_fr9_op(int32_t op, const void *h_a, const void *h_b, const void *h_c, size_t n, uint8_t *h_words, uint32_t *h_limbs, float *kernel_ms);
/* the point formulas on a caller's operands.  h_P: n points (X, Y, Z, T: 128 bytes; any field elements).  op: 0 p9_madd, 1 p10_madd, 3 the quad-lane mixed
   addition (h_Q: n Niels entries of 96 bytes; neg != 0: the entry negated as for a negative digit); 2 p10_add, 4 the quad-lane full addition (h_Q: n
   points); 5 k successive p9_madd of the same entry (k <= 4096).  h_out: n packed points; h_limbs: 4 x 10 words per case, the raw limbs of X, Y, Z, T.
   op 6: k_encode_points on h_P, on h_P[i] + h_Q[i] with h_Q (may be NULL); h_out: n encodings of 32 bytes.  op 7: k_decode_niels; h_P: n encodings,
   h_out: n Niels entries, *h_bad: the encodings refused (their entry: the identity's). */
int32_t otti_k_pt_op(int32_t op, const uint8_t *h_P, const uint8_t *h_Q, int32_t neg, uint32_t k, size_t n, uint8_t *h_out, uint32_t *h_limbs, uint32_t *h_bad,
                     float *kernel_ms);
/* sparse_mlpoly.rs AddrTimestamps::new for one side of the dense representation: h_addr3 = three lists of N addresses below M (k-major); walking them
   in order over one shared counter array, h_read_ts3[k * N + i] = audit[addr]++ and h_audit[0 .. M) = the counts at the end */
int32_t otti_k_addr_timestamps(const uint32_t *h_addr3, size_t N, size_t M, uint32_t *h_read_ts3, uint32_t *h_audit, float *kernel_ms);
/* one matrix of the SNARK decommitment filled from an entry list as the device does it for an instance whose lists are in HBM (a device ingest):
   position i < n is entry i; n <= i < pad_to the explicit padding (row i, column pad_col, value zero) upstream writes below two constraints
   (pad_to = n: none); the rest address 0, value zero.  Outputs of N positions each: the addresses as u32, the same as field elements, the values.
   Before any device is touched: a null pointer (the lists may be NULL when n = 0), N outside 1 .. 2^28, n > N or pad_to > N is OTTI_ERR_BAD_ARG. */
int32_t otti_k_decomm_entries(const uint32_t *h_row, const uint32_t *h_col, const uint8_t *h_val_mont32, size_t n, size_t N, size_t pad_to, uint32_t pad_col,
                              uint32_t *out_row_u32, uint32_t *out_col_u32, uint8_t *out_row_fr, uint8_t *out_col_fr, uint8_t *out_val_fr, float *kernel_ms);
/* rank's share of an entry list as a sharded prover filters a device-ingested instance (flag, scan, scatter): the entries whose row (by_col != 0:
   column) is rank mod world, in list order, that index divided by world, the other index and the value untouched.  Outputs have room for n entries;
   *out_n receives the number selected.  kernel_ms includes the read of the count between scan and scatter.  Before any device is touched: a null
   pointer (lists and outputs may be NULL when n = 0; out_n never), world not a power of two, rank >= world or n >= 2^32 is OTTI_ERR_BAD_ARG. */
int32_t otti_k_shard_filter(const uint32_t *h_row, const uint32_t *h_col, const uint8_t *h_val_mont32, size_t n, uint32_t world, uint32_t rank, int32_t by_col,
                            uint32_t *out_row, uint32_t *out_col, uint8_t *out_val, size_t *out_n, float *kernel_ms);
/* canonical LE <-> Montgomery on the device */
int32_t otti_k_fr_from_canonical(const uint8_t *h_in, uint8_t *h_out, size_t n);
int32_t otti_k_fr_to_canonical(const uint8_t *h_in, uint8_t *h_out, size_t n);
/* R1CSInstance::multiply_vec: z has 2*num_vars entries; outputs num_cons entries each */
int32_t otti_k_multiply_vec(otti_instance *inst, const uint8_t *h_z, uint8_t *h_Az, uint8_t *h_Bz, uint8_t *h_Cz, float *kernel_ms);
/* the same for K vectors through the many-vector kernels (one walk over the matrices per tile of four vectors, K = 1 included): h_zs[k] has
   2*num_vars entries; outputs K * num_cons entries each, vector k's at [k * num_cons ..), bit for bit what otti_k_multiply_vec gives for it.
   kernel_ms includes putting a tile's vectors side by side.  OTTI_ERR_BAD_ARG: a null argument or K = 0. */
int32_t otti_k_multiply_vec_many(otti_instance *inst, const uint8_t *const *h_zs, size_t K, uint8_t *h_Az, uint8_t *h_Bz, uint8_t *h_Cz, float *kernel_ms);
/* otti_nizk_prove_many's front half alone on K staged vectors (plan, budget and switches as there; small_flags[k] != 0: vector k's rows are
   summed by the MSM variant for small scalars).  h_rows32: K * L * 32 bytes, the compressed UNBLINDED row sums of vector k's variables at
   [k * L * 32 ..); h_Az, h_Bz, h_Cz: K * num_cons entries each.  What the plan leaves to a single proof is formed as that proof forms it, so the
   outputs are whole; info (may be NULL) says what ran jointly.  OTTI_ERR_BAD_ARG: a null argument, K = 0, generators made for another size. */
int32_t otti_k_prove_front(otti_instance *inst, otti_gens *gens, const uint8_t *const *h_zs, const int32_t *small_flags, size_t K, uint8_t *h_rows32,
                           uint8_t *h_Az, uint8_t *h_Bz, uint8_t *h_Cz, otti_prove_many_info *info, float *kernel_ms);
/* the patch of kept products on a caller's host state.  h_cols: ncols strictly ascending z indices below 2 * padded num_vars (else
   OTTI_ERR_INVALID_INDEX, judged on the host before anything is staged), or NULL with the range [first, first + count); the io vectors are N
   Montgomery elements each, io_bits ceil(N / 64) words, *io_unsat the count that goes with them: they are patched for z = h_z_new exactly as a
   mutator would patch kept products.  h_rows (room for n_rows_cap): the touched rows, ascending; *n_touched their number; *took_full_pass as
   decided by the rule / OTTI_PRODUCTS_FULL_SHARE. */
int32_t otti_k_products_patch(otti_instance *inst, const uint8_t *h_z_new, const uint64_t *h_cols, size_t ncols, size_t first, size_t count,
                              uint8_t *io_Az, uint8_t *io_Bz, uint8_t *io_Cz, uint64_t *io_bits, uint64_t *io_unsat,
                              uint32_t *h_rows, size_t n_rows_cap, uint64_t *n_touched, int32_t *took_full_pass, float *kernel_ms);
/* compute_eval_table_sparse x3 fused with r_A*A + r_B*B + r_C*C: eq_rx has num_cons entries, out 2*num_vars */
int32_t otti_k_eval_table_sparse(otti_instance *inst, const uint8_t *h_eq_rx, const uint8_t *h_rABC /* 3 */, uint8_t *h_out, float *kernel_ms);
/* R1CSInstance::evaluate at K points in one batched pass (the verifier's evaluation in otti_nizk_verify_many; always the many-point kernels, K = 1
   included).  out32: K x 3 scalars, A, B, C at each point; rx: K x log2(padded num_cons), ry: K x log2(2 * padded num_vars) scalars, conventions of
   otti_k_eq_evals (Montgomery words in and out, MSB first).  kernel_ms: the eq tables and the evaluation, first launch to last.  HBM as stated
   at otti_nizk_verify_many.  OTTI_ERR_BAD_ARG for a null inst, or null rx32 / ry32 / out32 with K > 0; OTTI_ERR_NO_DEVICE without a device. */
int32_t otti_k_instance_evaluate(otti_instance *inst, const uint8_t *rx32, const uint8_t *ry32, size_t K, uint8_t *out32, float *kernel_ms);
/* which of their variants the three sparse passes above and below (multiply_vec / the satisfiability pass: by_col = 0; eval_table_sparse:
   by_col != 0, rows = 2*num_vars) run on this instance.  quad: a row per four lanes (else per lane); use_small: entries are read through 4-byte
   small-integer codes; n_heavy rows whose longest list exceeds 64 entries go through n_seg segments of 2048.  Makes the device copy of the
   instance as those entries do, if it is not there yet, and launches nothing else. */
typedef struct { uint64_t rows, entries[3], n_heavy, n_seg; int32_t use_small, quad; } otti_device_info;
int32_t otti_instance_device_info(otti_instance *inst, int32_t by_col, otti_device_info *out);
/* the last successful otti_instance_set_values of an instance that keeps its lists in HBM, by HIP events: ms[0] the convert launches, ms[1] the
   place launches (the first call: the fills that record the slot maps), over all matrices of the call; zeros before any call and on the plain
   route.  Touches no device. */
int32_t otti_k_instance_values_kernel_ms(const otti_instance *inst, float ms[2]);
/* EqPolynomial::evals */
int32_t otti_k_eq_evals(const uint8_t *h_r, size_t ell, uint8_t *h_out, float *kernel_ms);
/* DensePolynomial::bound_poly_var_top / _bot (in place on a staged copy; out has len/2 entries) */
int32_t otti_k_fold_top(const uint8_t *h_Z, size_t len, const uint8_t *h_r, uint8_t *h_out, float *kernel_ms);
int32_t otti_k_fold_bot(const uint8_t *h_Z, size_t len, const uint8_t *h_r, uint8_t *h_out, float *kernel_ms);
/* one round of prove_cubic_with_additive_term's table work: (e0,e2,e3) of A*(B*C-D) over tables of length len */
int32_t otti_k_sc_cubic_round(const uint8_t *h_A, const uint8_t *h_B, const uint8_t *h_C, const uint8_t *h_D, size_t len, uint8_t *h_e3, float *kernel_ms);
/* fused fold(r) + next round's sums: tables of length len are folded to len/2 (written to h_out4, 4*len/2) and (e0,e2,e3) returned */
int32_t otti_k_sc_cubic_fold_round(const uint8_t *h_A, const uint8_t *h_B, const uint8_t *h_C, const uint8_t *h_D, size_t len,
                                   const uint8_t *h_r, uint8_t *h_out4, uint8_t *h_e3, float *kernel_ms);
/* one round of prove_quad: (e0,e2) of A*B */
int32_t otti_k_sc_quad_round(const uint8_t *h_A, const uint8_t *h_B, size_t len, uint8_t *h_e2, float *kernel_ms);
int32_t otti_k_sc_quad_fold_round(const uint8_t *h_A, const uint8_t *h_B, size_t len, const uint8_t *h_r, uint8_t *h_out2, uint8_t *h_e2, float *kernel_ms);
/* The grid of the round launches above and of the cubic3 ones below, for tests: every launch takes its grid from a plan over the table length and
   seven capacities of the device — its CUs, then the workgroups resident at once of the cubic3 evaluate, cubic3 fold, quad evaluate, quad fold,
   four-table evaluate and four-table fold kernels.  otti_k_sc_caps_override puts h_caps7 in the device's place for every later launch of this
   process (a short table then walks several items per thread, or spreads over up to 2048 workgroups); NULL restores what the device reported.
   OTTI_ERR_BAD_ARG for a zero among the seven, and while a proof is in flight.  otti_k_sc_plan: the grid and the most items any thread walks
   that a launch of `kind` (0 .. 5 in the order above) over tables of length len gets under the capacities now in force. */
int32_t otti_k_sc_caps_override(const uint32_t *h_caps7);
int32_t otti_k_sc_plan(int32_t kind, size_t len, int32_t armed, uint32_t *workgroups, uint64_t *items_per_thread);
/* DensePolynomial::commit_inner: L rows of R scalars -> L compressed points C_i = sum_j Z[iR+j] P[j] + blinds[i] P[R+1] */
/* Self-test of the "armed" launches the provers use for their small sequential rounds (a kernel queued before its challenge is known
 * and released through pinned host memory): the quadratic fold + sums round on the caller's tables (length len, a power of two >= 8),
 * plain, armed + released after hold_us microseconds, and armed + aborted.  out2 (len/2 + len/2 elements) and e2 (2 elements) are the
 * plain launch's results; any disagreement between the three ways is OTTI_ERR_INTERNAL. */
int32_t otti_k_armed_selftest(const uint8_t *A, const uint8_t *B, size_t len, const uint8_t *r, uint32_t hold_us, uint8_t *out2, uint8_t *e2);
/* The device pass of otti_nizk_verify_batch alone (dev_batch_sum: one k_decode_niels_sets launch, one k_msm_var_many launch).  Set k: points
   [set_offsets[k], set_offsets[k + 1]) of h_compressed32 (nsets + 1 ascending offsets from 0, in points).  With nsets >= 2 the LAST set plays the
   generators: it is decoded ahead, as a generators handle's set is, and takes part resident; a job may name it only alone.  Job j sums the
   job_nsets[j] consecutive sets from job_first_set[j] on with the next (those sets' points) scalars of h_scalars_mont32; jobs may overlap.
   codes[j] = 0 and out32 + 32 j the encoded sum, or OTTI_ERR_VERIFY_DECOMPRESS (32 zero bytes) exactly when one of the job's sets holds a point
   that does not decode.  kernel_ms (may be NULL): device-event time of the two launches.  No host fallback. */
int32_t otti_k_batch_sum(size_t nsets, const uint8_t *h_compressed32, const size_t *set_offsets, size_t njobs, const uint32_t *job_first_set,
                         const uint32_t *job_nsets, const uint8_t *h_scalars_mont32, uint8_t *out32, int32_t *codes, float *kernel_ms);
/* The expansion of product-form generator runs alone (one k_gen_runs launch, one thread per (job, slot)): job j is a vector of job_n[j] scalars,
   out[j][i] = base[j][i] + sum over the runs r of job j with i < 2^lg_r of  c_r * prod_{t < lg_r, bit t of i set} f_r[t]  (bit 0 the least
   significant).  A job with job_has_base[j] != 0 takes the next job_n[j] words of h_base_mont32, otherwise zeros.  Run r belongs to job
   run_job[r] (ascending), has run_lg[r] <= 20 factors — the next of h_factors_mont32 — with 2^lg <= job_n, and the coefficient h_run_c_mont32[r].
   h_out_mont32 takes the jobs' vectors one behind the other.  All scalars are 32-byte Montgomery words.  kernel_ms (may be NULL): device-event
   time of the tables' upload and the launch.  No host fallback.  OTTI_ERR_BAD_ARG before a device is touched for anything the above excludes. */
int32_t otti_k_gen_runs(size_t njobs, const size_t *job_n, const uint8_t *job_has_base, const uint8_t *h_base_mont32, size_t nruns, const uint32_t *run_job,
                        const uint32_t *run_lg, const uint8_t *h_run_c_mont32, const uint8_t *h_factors_mont32, uint8_t *h_out_mont32, float *kernel_ms);
int32_t otti_k_msm_rows(otti_gens *gens, const uint8_t *h_Z, size_t L, size_t R, const uint8_t *h_blinds, uint8_t *h_out32, float *kernel_ms);
/* A general fixed-base MSM job, as the prover's launcher takes it, for kernel-level tests: row i = sum_{j < n_dense} dense[i n_dense + j] P[j]
   + sum_{e < n_extra} extra_s[i n_extra + e] P[extra_base[e]] over the generators' R + 2 points (n_dense <= R, n_extra <= 8, extra_base[e] < R + 2;
   scalars Montgomery).  mode: 0 compressed, 1 raw, 2 kept row sums — h_out32 receives 32 compressed bytes per row in every mode.  sparse: -1 decides
   by the scalars as otti_k_msm_rows does, 0 / 1 force the plain / work-list bulk kernel.  force_bulk: the chip-filling kernel whatever the size.
   bulk_workgroups: the workgroups a bulk launch aims for (0 = the default the prover uses; 1 makes one workgroup walk a whole row in sub-chunks).
   plan5 (may be NULL) = {kernel (0 bulk, 1 bulk-sparse, 2 small), chunk, nchunks, fuse, route (0 mail, 1 flag, 2 keep, 3 raw, 4 device-encode,
   5 host-encode)} of the launch.  OTTI_ERR_BAD_ARG, before a device is touched, for a base beyond the table, n_extra > 8, n_dense > R, no term at
   all, rows outside 1 .. 65535, more than 512 raw rows, an unknown mode. */
int32_t otti_k_msm_job(otti_gens *gens, size_t rows, size_t n_dense, const uint8_t *h_dense, size_t n_extra, const uint8_t *h_extra_s,
                       const uint32_t *h_extra_base, int32_t mode, int32_t sparse, int32_t force_bulk, size_t bulk_workgroups, uint8_t *h_out32,
                       uint32_t *plan5, float *kernel_ms);
/* the kernel that patches kept rows, on L identity points: out[i] = compress(sum over {k : idx[k] in [iR, (i+1)R)} s[k] * P[idx[k] - iR]), i < L <= 4096,
   R = the generators' row length; idx strictly ascending below L*R (else OTTI_ERR_INVALID_INDEX), s Montgomery.  A row without terms is the identity. */
int32_t otti_k_msm_scatter_rows(otti_gens *gens, size_t L, const uint64_t *h_idx, const uint8_t *h_s, size_t count,
                                uint8_t *h_out32, float *kernel_ms);
/* the two passes of otti_witness_assign on a staged vector: h_old = n Montgomery elements, h_src = n elements in `format`, stride_bytes apart
   (0: packed).  h_new = the vector afterwards; h_idx = the ascending indices of the elements whose value changed and h_delta = new - old for each
   (room for n each, *n_changed filled); *chunk (may be NULL) = elements per workgroup chunk of the passes.  A scalar >= l: OTTI_ERR_INVALID_SCALAR,
   outputs untouched. */
int32_t otti_k_witness_diff(const uint8_t *h_old, size_t n, const void *h_src, int32_t format, size_t stride_bytes, uint8_t *h_new,
                            uint64_t *h_idx, uint8_t *h_delta, uint64_t *n_changed, uint32_t *chunk, float *kernel_ms);
/* PolyEvalProof::verify's C_LZ on the device [dense_mlpoly.rs PolyEvalProof::verify -> GroupElement::vartime_multiscalar_mul, RECALL]:
   out = compress(sum_i s[i] * decompress(C[i])), n >= 256 compressed ristretto255 points, scalars in Montgomery form.  Batch decompression,
   LDS-bucket Pippenger, window recombination on the host.  OTTI_ERR_VERIFY_DECOMPRESS if an encoding does not decode. */
int32_t otti_k_row_sum(const uint8_t *h_compressed32, size_t n, const uint8_t *h_scalars_mont32, uint8_t *h_out32);
/* Several such sums in ONE pass (what otti_snark_verify_many sends at each of its three seams): one decode launch over all sets with a counter
   per set, one sum launch over all jobs.  Set k = points [set_offsets[k], set_offsets[k + 1]) of h_compressed32 (nsets + 1 ascending offsets, counted
   in points); job j sums set job_set[j] with the next n(job_set[j]) scalars of h_scalars_mont32 — several jobs may name one set.  out32[32 j ..] =
   the compressed sum and codes[j] = 0, or zeros and codes[j] = OTTI_ERR_VERIFY_DECOMPRESS exactly when job j's set has an encoding that does not
   decode; the other jobs of the call are unaffected.  Sets of 1 .. 2^20 points (no floor of 256 here).  No host fallback.  OTTI_ERR_BAD_ARG: a
   null argument, nsets or njobs 0, an empty set or one of more than 2^20 points, a job_set[j] >= nsets. */
int32_t otti_k_row_sum_many(size_t nsets, const uint8_t *h_compressed32, const size_t *set_offsets, size_t njobs, const uint32_t *job_set,
                            const uint8_t *h_scalars_mont32, uint8_t *h_out32, int32_t *codes);

/* ---- the kernels the prover actually launches for phase one, the evaluation proof and the bullet reduction (host pointers, as above).
        No reference counterpart beyond the upstream functions named; these exist so that a failing proof points at a kernel. ---- */
/* eq "pyramid": level k (eq over the LAST k of the n variables, 2^k entries) at out + 2^k - 1; n <= 13; out has 2^(n+1) - 1 entries */
int32_t otti_k_eq_pyramid(const uint8_t *h_r, size_t n, uint8_t *h_out);
/* prove_cubic_with_additive_term with the eq table factored out: S_t = sum_i E[i] (B_t C_t - D_t)[i], t = 0, 2, 3, over tables of
   length len, E = EqPolynomial(h_tau[0 .. log2(len) - 1)).evals() supplied as the challenge suffix it is built from */
int32_t otti_k_sc_cubic3_round(const uint8_t *h_B, const uint8_t *h_C, const uint8_t *h_D, size_t len, const uint8_t *h_tau, uint8_t *h_e3, float *kernel_ms);
/* fused bound_poly_var_top(r) + the next round's S_t: tables of length len (>= 4) fold to len/2 (h_out3: 3 * len/2 elements);
   h_tau holds the log2(len) - 2 variables E of the folded round is built from */
int32_t otti_k_sc_cubic3_fold_round(const uint8_t *h_B, const uint8_t *h_C, const uint8_t *h_D, size_t len, const uint8_t *h_r, const uint8_t *h_tau,
                                    uint8_t *h_out3, uint8_t *h_e3, float *kernel_ms);
/* DensePolynomial::bound: out[j] = sum_i Lv[i] * Z[i*R + j] */
int32_t otti_k_poly_bound(const uint8_t *h_Z, size_t L, size_t R, const uint8_t *h_Lv, uint8_t *h_out, float *kernel_ms);
/* One BulletReductionProof::prove round on the ORIGINAL generators (k_msm.hip): state (a, b: 2*n_cur elements if fold else n_cur; s: R
   coefficients of the original generators).  If fold, the previous challenge (u, u^-1) is applied first.  Returns compressed L, R
   (64 bytes; blinds h_blinds2 = {blind_L, blind_R}) and the state the next round starts from (a, b: n_cur elements; s: R). */
int32_t otti_k_bullet_round(otti_gens *gens, size_t n_cur, int32_t fold, const uint8_t *h_u, const uint8_t *h_uinv, const uint8_t *h_a, const uint8_t *h_b,
                            const uint8_t *h_s, const uint8_t *h_blinds2, uint8_t *h_a_out, uint8_t *h_b_out, uint8_t *h_s_out, uint8_t *h_LR64, float *kernel_ms);
/* the closing fold of the reduction (length 2 -> 1): a, b of 2 elements and s of R are folded in place by (u, u^-1) */
int32_t otti_k_bullet_last_fold(size_t R, const uint8_t *h_u, const uint8_t *h_uinv, uint8_t *h_a2, uint8_t *h_b2, uint8_t *h_s);
/* ---- SNARK mode's kernels (R1CSEvalProof: product circuits, their batched sum-check, the hash layer).  A batch of ninst (1 .. 20) instances travels
        as ONE array per table kind: instance y's table at element y * len.  h_has_C[y] != 0: instance y is a dot-product triple with a third table;
        h_C holds those third tables alone, in instance order.  0: a product-circuit instance, whose third table is the shared eq table of h_tau. ---- */
/* one round of the batched cubic sum-check.  h_r == NULL: the sums of tables of length len as they are.  Otherwise the tables are folded by r first
   (bound_poly_var_top; h_out: the folded A tables, the B tables, the C tables, len / 2 elements each).  h_e: 3 * ninst sums (at 0, 2, 3), without
   the bound variable's eq factor for product-circuit instances.  Item i of a table is element i * G + rk of the eq table (a rank's residue class of a
   sharded layer); h_tau holds log2(G * len / 2) variables (len / 4 with a fold). */
int32_t otti_k_pc_round(const uint8_t *h_A, const uint8_t *h_B, const uint8_t *h_C, const uint8_t *h_has_C, size_t ninst, size_t len, const uint8_t *h_tau,
                        const uint8_t *h_r, uint32_t G, uint32_t rk, uint8_t *h_out, uint8_t *h_e, float *kernel_ms);
/* The grid of otti_k_pc_round, otti_k_dot_many and otti_k_sum3, for tests: min(ceil(items / 256), max_blocks / ninst) workgroups per instance (at
   least one), max_blocks = 2048 on the device's own account; beyond that a thread walks several items.  otti_k_pc_grid_cap_override puts
   *h_max_blocks in the place of the 2048 for every later launch of this process (a short table then walks many items per thread); NULL or 0
   restores the device's own.  OTTI_ERR_BAD_ARG above 2048, and while a proof is in flight.  otti_k_pc_plan: the workgroups per instance and the
   most items any thread walks that a launch over ninst (1 .. 64) instances of `items` items gets under the cap now in force (items = len / 2 for
   otti_k_pc_round, len / 4 with a fold, n for the other two). */
int32_t otti_k_pc_grid_cap_override(const uint32_t *h_max_blocks);
int32_t otti_k_pc_plan(size_t ninst, size_t items, uint32_t *workgroups, uint64_t *items_per_thread);
/* the hand-over of a batch's tables to the host (folded by h_fold_r first unless NULL): h_out[(3 y + t) * n_out ..) = table t of instance y
   (n_out = len, or len / 2 with a fold; the place of an absent third table is zero) */
int32_t otti_k_pc_export(const uint8_t *h_A, const uint8_t *h_B, const uint8_t *h_C, const uint8_t *h_has_C, size_t ninst, size_t len, const uint8_t *h_fold_r, uint8_t *h_out);
/* the persistent launch that plays log2(len0 / t_out) rounds with W workgroups per instance, the host answering round j with h_rs[j]: h_sums =
   [round][instance][3] sums (the eq table of h_tau, log2(len0) variables, is a real third table here), h_out as otti_k_pc_export with n_out = t_out.
   h_fold_r: the tables hold 2 * len0 elements and are folded on load.  top != 0: h_tau[0] is applied as one factor above a table of the others. */
int32_t otti_k_pc_tail(const uint8_t *h_A, const uint8_t *h_B, const uint8_t *h_C, const uint8_t *h_has_C, size_t ninst, size_t len0, uint32_t W, size_t t_out,
                       const uint8_t *h_tau, const uint8_t *h_rs, const uint8_t *h_fold_r, int32_t top, uint8_t *h_sums, uint8_t *h_out);
/* ProductCircuit::compute_layer of ninst (1 .. 16) circuits: inputs of 2 q elements each, out_left[i] = left[i] * right[i], out_right[i] = left[q + i] * right[q + i] */
int32_t otti_k_prod_layer(const uint8_t *h_left, const uint8_t *h_right, size_t ninst, size_t q, uint8_t *h_out_left, uint8_t *h_out_right, float *kernel_ms);
/* Layers::build_hash_layer: cells (init, audit) and operations (read, write) of n elements hashed with (r, gamma); rank rk of G writes the n / G
   elements of its residue class (both halves of the vector keep the indices i = rk mod G) */
int32_t otti_k_hash_mem(const uint8_t *h_eval_table, const uint8_t *h_audit_ts, size_t M, const uint8_t *h_r, const uint8_t *h_gamma, uint32_t G, uint32_t rk,
                        uint8_t *h_out_init, uint8_t *h_out_audit, float *kernel_ms);
int32_t otti_k_hash_ops(const uint8_t *h_addr, const uint8_t *h_deref, const uint8_t *h_read_ts, size_t N, const uint8_t *h_r, const uint8_t *h_gamma, uint32_t G, uint32_t rk,
                        uint8_t *h_out_read, uint8_t *h_out_write, float *kernel_ms);
/* h_out[y] = <E, P_y> for npoly (1 .. 64) polynomials of n elements; h_out[y] = sum_i A_y[i] B_y[i] C_y[i] for ninst (1 .. 20) triples */
int32_t otti_k_dot_many(const uint8_t *h_E, const uint8_t *h_Ps, size_t npoly, size_t n, uint8_t *h_out, float *kernel_ms);
int32_t otti_k_sum3(const uint8_t *h_A, const uint8_t *h_B, const uint8_t *h_C, size_t ninst, size_t n, uint8_t *h_out, float *kernel_ms);
/* DensePolynomial::bound in chunks of m rows: h_out[c * R + j] = sum_i Lv_rest[i] * Z[(c m + i) * R + j].  *launched = 0 (and h_out untouched) when
   the geometry is one the launch function declines */
int32_t otti_k_poly_bound_chunks(const uint8_t *h_Z, size_t L, size_t R, const uint8_t *h_Lv_rest, size_t m, uint8_t *h_out, int32_t *launched, float *kernel_ms);

/* ---- the same kernels on DEVICE pointers and a caller-chosen HIP stream ("host or device pointers + a stream
        handle"): nothing is staged through PCIe, so a kernel can be benchmarked or composed from outside the library.
        stream: a hipStream_t passed as void* (NULL = the calling thread's library stream).  d_* = device memory holding 32-byte
        Montgomery-form elements; h_* = small host arrays (challenges come from the transcript).  Calls that return round sums
        (h_e*) wait for that launch's result; the others only enqueue. ---- */
int32_t otti_kd_multiply_vec(otti_instance *inst, const void *d_z, void *d_Az, void *d_Bz, void *d_Cz, void *stream);
/* the same pass as otti_witness_check_sat on a caller's device vector z (2*num_vars Montgomery elements) and stream: d_bits receives
   ceil(num_cons/64) 64-bit words (bit r & 63 of word r >> 6 set: constraint r fails; every word is written).  h_n_unsat non-NULL: waits and
   returns the number of failing constraints; NULL: only enqueues. */
int32_t otti_kd_check_sat(otti_instance *inst, const void *d_z, void *d_bits, uint64_t *h_n_unsat, void *stream);
int32_t otti_kd_eval_table_sparse(otti_instance *inst, const void *d_eq_rx, const uint8_t *h_rABC, void *d_out, void *stream);
int32_t otti_kd_eq_evals(const uint8_t *h_r, size_t ell, void *d_out, void *stream);
int32_t otti_kd_fold_top(void *d_Z, size_t len, const uint8_t *h_r, void *stream);                    /* in place: len -> len/2 */
int32_t otti_kd_fold_bot(const void *d_Z, void *d_out, size_t len, const uint8_t *h_r, void *stream);
int32_t otti_kd_sc_cubic_round(const void *d_A, const void *d_B, const void *d_C, const void *d_D, size_t len, uint8_t *h_e3, void *stream);
int32_t otti_kd_sc_cubic_fold_round(void *d_A, void *d_B, void *d_C, void *d_D, size_t len, const uint8_t *h_r, uint8_t *h_e3, void *stream);   /* in place */
int32_t otti_kd_sc_quad_round(const void *d_A, const void *d_B, size_t len, uint8_t *h_e2, void *stream);
int32_t otti_kd_sc_quad_fold_round(void *d_A, void *d_B, size_t len, const uint8_t *h_r, uint8_t *h_e2, void *stream);                            /* in place */
/* compressed row commitments land in d_out32 (32 * L bytes of device memory) */
int32_t otti_kd_msm_rows(otti_gens *gens, const void *d_Z, size_t L, size_t R, const void *d_blinds, void *d_out32, void *stream);
/* plain device memory for callers without a HIP runtime of their own (ctypes tests); hipMalloc'ed buffers of any origin work as well */
int32_t otti_dev_alloc(size_t nbytes, void **d_out);
int32_t otti_dev_free(void *d);
int32_t otti_dev_upload(void *d_dst, const void *h_src, size_t nbytes);
int32_t otti_dev_download(void *h_dst, const void *d_src, size_t nbytes);
/* a HIP stream of the runtime the library itself is linked to (a caller with its own HIP code passes its hipStream_t instead) */
int32_t otti_dev_stream_create(void **stream_out);
int32_t otti_dev_stream_sync(void *stream);
int32_t otti_dev_stream_destroy(void *stream);

/* the integer-ALU roof the bulk MSM is priced against: whole-chip throughput of its mixed point addition (operands in registers,
   every CU busy), measured now (about 10 ms of GPU time) */
int32_t otti_bench_madd_peak(double *madds_per_second);
/* the second roof of the streaming kernels (sum-check rounds, sparse products, eq tables): whole-chip throughput of the Montgomery
   product in GF(l), operands in registers, measured now (about 10 ms of GPU time) */
int32_t otti_bench_fr_mul_peak(double *products_per_second);

/* per-kernel-class timing with HIP events recorded on the library's own stream around every launch of that class.
   classes: msm_rows (>= 2^16 scalars per launch: the witness commitment) msm_small msm_finish sc_cubic sc_quad spmv eq reduce poly_bound bullet other.  enable(1) also resets the counters. */
int32_t otti_stats_enable(int32_t on);
/* restrict timing to one class (call after enable): two event records per launch are not free on the latency-bound round loop */
int32_t otti_stats_select(const char *kernel_class);
int32_t otti_stats_read(const char *kernel_class, uint64_t *count, double *total_ms);
/* SNARK mode adds the classes pc_round (rounds of the batched product-circuit sum-checks) prod_layer hash_layer gather dot_many; the verifier
   decode msm_var; otti_witness_check_sat / otti_kd_check_sat sat_check. */
/* 1 when the calling thread's next proof would use armed launches (kernels queued ahead of their challenge): off under OTTI_ARMED=0,
   while a class with armed kernels (msm_small sc_cubic sc_quad pc_round) is being timed, and with several proofs in flight */
int32_t otti_armed_launches_on(int32_t *on);

/* ---- multi-GPU plumbing: sum-check partial sums travel as 8 x u32 limbs widened to u64 lanes so that a plain integer
        sum all-reduce (RCCL ncclSum/ncclUint64, or gloo in CPU tests) followed by one normalisation gives the Fr sum ---- */
void    otti_lanes_pack(const uint8_t *fr_mont32, size_t n, uint64_t *lanes /* 8n */);
void    otti_lanes_unpack(const uint64_t *lanes, size_t n, uint8_t *fr_mont32);   /* reduces each 8-lane group mod l */

#ifdef __cplusplus
}
#endif
#endif
