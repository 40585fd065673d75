// Device layer of the proving path: HBM-resident objects, the device context with its mailboxes and host waits (k_context.hip, waits.cpp;
// the mail formats themselves: mail.h) and the kernel launch functions (k_*.hip).
// Everything runs on one HIP stream owned by DevCtx; results that the Fiat-Shamir transcript needs come back through
// a small pinned buffer.  No function here falls back to the host: without a gfx950 device they throw Error(OTTI_ERR_NO_DEVICE).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include <functional>
#include <cstddef>
#include <chrono>
#include "spartan.h"
#include "mail.h"
#include "msm_plan.h"
#include "sc_plan.h"

namespace otti {

#define OTTI_HIP(expr) ::otti::hip_check((expr), #expr, __FILE__, __LINE__)
void hip_check(hipError_t e, const char *what, const char *file, int line);
struct OutOfDeviceMemory : Error { using Error::Error; };
// the persistent sum-check tail (snark_dev.h) never answered: its grid was not resident as a whole (another tenant of the GPU, a CU mask, a
// partition).  SNARK::prove catches this one, switches the tail off for the process and proves again with a launch per round.
struct TailTimeout : Error { using Error::Error; };   // hipErrorOutOfMemory: callers that can make do with less catch this one

template <class T> struct DevBuf {
    T *p = nullptr; size_t n = 0;
    DevBuf() {}
    explicit DevBuf(size_t count) { alloc(count); }
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
    ~DevBuf() { release(); }
    void alloc(size_t count) { release(); if (count) OTTI_HIP(hipMalloc((void **)&p, count * sizeof(T))); n = count; }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// three CSR matrices side by side (A, B, C), by value into kernels
struct DCsr3 { const uint32_t *ptr[3]; const uint32_t *idx[3]; const Fr *val[3]; const int32_t *small[3]; };
struct DeviceCsrSet {
    DevBuf<uint32_t> ptr[3], idx[3]; DevBuf<Fr> val[3];
    DevBuf<int32_t> small[3];                                 // per entry: the coefficient as a small signed integer, or kNotSmall (then val[] is read)
    bool use_small = false;                                   // most coefficients are small integers (a compiled circuit): the kernels read 4 bytes per entry instead of 32
    DevBuf<uint32_t> heavy;                                   // ids of rows whose longest list exceeds kHeavyRow
    DevBuf<uint32_t> seg_row, seg_no, seg_begin;              // their segments (row id, segment number), and each long row's first segment
    size_t rows = 0, n_heavy = 0, n_seg = 0;
    double avg_row = 0.0;                                     // entries per row and matrix: picks the row-per-lane or the row-per-quad kernel
    bool quad() const { return avg_row >= 3.0; }              // row per quad from three entries per row and matrix on (k_sparse.hip: the launchers' and the report's one rule)
    DCsr3 view() const { DCsr3 v; for (int k = 0; k < 3; k++) { v.ptr[k] = ptr[k].p; v.idx[k] = idx[k].p; v.val[k] = val[k].p; v.small[k] = small[k].p; } return v; }
};
// an entry list in HBM, in caller order: what both CSR copies are built from (k_sparse.hip build_csr_set).  code: the small-integer codes of
// classify_coefficients, needed while the copies are built only.
struct DeviceCoo { DevBuf<uint32_t> row, col; DevBuf<Fr> val; DevBuf<int32_t> code; size_t n = 0; };
// ent[k]: the entry lists themselves, KEPT beside the CSR copies by a device ingest (k_ingest.hip) and by nothing else — they are what
// Instance::mat() downloads when a host consumer asks for the lists.  Their cost: 40 bytes of HBM per entry (row 4, col 4, val 32) for as long as
// the instance lives; otti_instance_ingest_info reports it.  An instance uploaded from host lists keeps none (ent[k].n = 0, no buffers).
// slot_row[k], slot_col[k]: where entry i of ent[k] sits in by_row / by_col (its position in idx / val / small of that copy) — made by the first
// otti_instance_set_values of the instance and by nothing else (k_revalue.hip), kept for its life: 8 bytes per entry.  n_small[k]: how many of
// ent[k]'s coefficients have a small-integer code, counted then as well, so that the codes rule can be applied again when one matrix changes.
struct DeviceInstance {
    DeviceCsrSet by_row, by_col; size_t nnz = 0; DeviceCoo ent[3];
    DevBuf<uint32_t> slot_row[3], slot_col[3]; bool slots_resident = false; unsigned long long n_small[3] = {0, 0, 0};
    // set_values' scratch that does not become part of the instance, kept from the first call on so that later calls allocate the staging value
    // list alone: the convert pass's code lists (4 bytes per entry of every matrix ever replaced) and its four words (error key, three small counts)
    DevBuf<int32_t> values_code[3]; DevBuf<unsigned long long> values_words;
    float values_kernel_ms[2] = {0, 0};                      // the last set_values' convert and place launches by HIP events (all matrices of the call)
};
struct DevCtx;
bool classify_coefficients(DevCtx &c, DeviceCoo coo[3]);
void build_csr_set(DevCtx &c, DeviceCsrSet &d, const DeviceCoo coo[3], bool by_col, size_t rows, bool use_small);
// The tail of every device ingest (k_ingest.hip: zkInterface bytes; k_coo_ingest.hip: row / column / coefficient arrays), behind a clean pass that
// left the validated lists in d->ent in caller order: the size check, classify_coefficients, both CSR copies, the codes released, and I's fields —
// dimensions, counts, host_lists_pending, ingested_on_device, source_bytes as circuit_bytes, lap 3 (from t0, a reading of ingest_now, to the end
// of the CSR build) and the device copy itself.
struct IngestDims { size_t ncp, nvp, num_inputs, given_cons, given_vars; };
double ingest_now();                                        // ms on the steady clock
void finish_device_ingest(DevCtx &c, Instance &I, const std::shared_ptr<DeviceInstance> &d, const IngestDims &dims, uint64_t source_bytes, double t0);
// A, B or C as three arrays (= otti_coo of the C ABI): n indices each in row and col (CooIdxFormat, coo_walk.h), n coefficients in val (WitFormat),
// val_stride bytes apart (never 0 here)
struct CooSource { const void *row, *col, *val; size_t n; int index_format, val_format; size_t val_stride; };
// otti_instance_from_coo behind its argument checks (k_coo_ingest.hip): the arrays, in HBM (then ordered behind `producer`'s queued work, nullptr:
// none to wait for) or on the host (then staged as they are), to the instance instance_new makes from the same triples.  The first defect in
// instance_new's order is thrown with its code and wording; everything allocated is released and the context stays usable.  Returns when the
// sources are free again.
std::unique_ptr<Instance> instance_from_coo(size_t num_cons, size_t num_vars, size_t num_inputs, const CooSource mats[3], bool src_on_device, hipStream_t producer);
// otti_instance_set_values behind its argument checks — the counts against I.nnz among them: capi.cpp — (k_revalue.hip): new coefficients for the entries of a live instance, in the order the
// entries were given.  An instance that keeps its lists in HBM (ent) is revalued there: a convert pass into staging lists (values, codes, the small
// count, one atomicMin error word), then — only behind a clean word — a place pass through the slot maps into both CSR copies, the staging list
// swapped in as ent[k].val, the codes rule applied again (small[] allocated or released as the variant flips), materialised host lists refreshed.
// Any other instance takes instance_set_values_host (a device source is downloaded first).  A refusal throws what instance_new would on the new
// triples and leaves the instance bit for bit as it was.  Both routes drop `shard` and bump I.value_gen.  Returns when the sources are free again.
// true: the instance keeps lists in HBM, i.e. the call takes the device route and needs a device
bool instance_values_on_device(const Instance &I);
void instance_set_values(Instance &I, const ValuesSource vals[3], bool src_on_device, hipStream_t producer);
bool device_runtime_up();                                  // a device context exists in this process already (k_context.hip): asking never brings one up
// Rank k of g holds the constraint rows r = k (mod g) (renumbered r / g, columns untouched: multiply_vec output lands where the
// low-bit-sharded phase-one tables need it) and, as a second copy, the entries of columns c = k (mod g) (renumbered c / g, rows
// untouched: compute_eval_table_sparse output lands where the phase-two tables need it).  SURVEY.md 8(e).
struct DeviceShard { int rank = 0, world = 1; DeviceCsrSet by_row, by_col; };
// rank's share of an entry list that is in HBM (k_sparse.hip: flag, scan_inplace, scatter): the entries whose row (by_col: column) is rank mod world,
// in list order, that index divided by world, the other one and the value untouched.  out: n and buffers of max(1, n) elements, no codes.  flags and
// scan_levels are scratch that grows and may be handed to the next call; the scatter is only queued.
void dev_shard_filter(DevCtx &c, const uint32_t *row, const uint32_t *col, const Fr *val, size_t n, int world, int rank, bool by_col, DeviceCoo &out,
                      DevBuf<uint32_t> &flags, std::vector<DevBuf<uint32_t>> &scan_levels);

// fixed-base window table: entry (base b, window w, digit d in 1..E) = d * 2^(c*w) * P[b] in affine Niels form
struct DeviceGens {
    DevBuf<TabEntry> table; int c = 0, W = 0; size_t E = 0, nbases = 0;
    double build_ms[2] = {0, 0};                            // what building it took: allocations / upload + kernels
    const TabEntry *entry0(size_t base) const { return table.p + base * (size_t)W * E; }
};
// nbases is the number of stream points the TABLE covers, not the R + 2 of the Gens a launch is made for: a Gens may hold the table of a longer
// one of its stream (adopt_gens_table).  Launchers take row lengths and base indices from the Gens and check them against nbases.

// where a sum-check kernel's last workgroup delivers the round's totals (see finish_in_kernel)
struct Mailbox { Fr *partials; unsigned *counter; Fr *host_results; unsigned long long *host_flag; unsigned long long seq; int slot; int line_mail = 0;
                 Fr *dev_results; };   // dev_results: the totals once more in HBM (same slots), for a device-side collective over them (shard.h, RCCL transport)

// Armed launches.  The sequential rounds cost a launch + dispatch (10-15 us) on top of the kernel itself when the kernel can only be
// launched once the host knows the round's challenge.  An ARMED kernel is queued before that: its first workgroup spins on a pinned host
// word until the host publishes the value (DevCtx::go), copies it to HBM for the other workgroups, and the round starts within a PCIe
// read of the challenge being known.  Every spin has a deadline (kArmDeadlineTicks of s_memrealtime: 30 s) and an abort value, so a grid always drains.
// ONE decision per armed launch: only the launch's first workgroup watches the host word and its deadline, and what it decides (the
// value arrived / aborted / gave up) is what every other workgroup acts on (they watch dev->seq alone, with a backstop of
// the leader's deadline plus a quarter: the leader never ran) — a grid never folds in part.  A leader that gives up says so in host->timed_out, so the host fails the
// proof at once instead of waiting for a result that will not come.
// Layout: the sequence number, a tag and the first value share one 64-byte line, so a poll that finds the number it waits for has the
// value in the same batch of loads (one PCIe round trip, not two).  The tag = go_tag(seq, values) makes a batch self-validating: the
// loads of one poll may be served at different times, and a batch that mixes old and new words fails the tag and is simply polled
// again.  timed_out (written by the DEVICE) sits in a line of its own.
struct alignas(64) GoBox { unsigned long long seq, tag, pad[2]; Fr v[4]; unsigned long long timed_out, pad2[3]; };
static_assert(sizeof(GoBox) == 192 && offsetof(GoBox, v) == 32 && offsetof(GoBox, timed_out) == 160, "GoBox layout is read by hand-written loads");
// The leader's copy for the other workgroups exists kGoCopies times, kGoCopyStride bytes apart (different memory channels): with every waiting
// workgroup polling ONE line, 128 pollers kept a single HBM channel busy enough to double the latency of each poll.  Workgroup b polls copy b mod kGoCopies.
constexpr int kGoCopies = 8;
constexpr size_t kGoCopyStride = 4096;
// ---- the small MSMs' chunk mails (mail.h MsmMail), summed on the host; OTTI_SMALL_HOST_SUM=0: the last workgroup sums them on the device instead
constexpr int kMsmMailRegions = 4;                           // launches whose mails can be waiting at once (round k read while k + 1 is queued, armed)
struct PtFe;
// mails [i0, i1) of m summed into acc (hostifma.h host_sum_cached) once each carries number `want` and a fitting tag; a mail that has not
// come after max_spins polls (0: no limit) makes it return false with acc holding the sum of those before it
bool msm_mail_sum(const MsmMail *m, int i0, int i1, unsigned long long want, PtFe &acc, unsigned max_spins, bool allow_ifma);
// whether mails [0, n) all carry number `want` and a fitting tag (no waiting, no arithmetic)
bool msm_mails_whole(const MsmMail *m, int n, unsigned long long want);
struct MsmPending { unsigned long long seq = 0, order = 0; int region = 0; uint32_t rows = 0, nchunks = 0; };
struct DevCtx;
struct MsmMailbox {
    MsmMail *host = nullptr, *dev = nullptr;                  // pinned, kMsmMailRegions regions of kMsmMailCap mails; the device's address of the same
    // Launches whose mails are still to be summed, oldest first (an armed round is queued before its predecessor is read).  Launch k mails
    // to region k mod kMsmMailRegions; queueing one more than that drops the oldest entry, whose region it reuses.
    MsmPending pending[kMsmMailRegions]; int pending_n = 0;
    unsigned long long launches = 0;                          // mailing launches queued on this context (picks the region)
    unsigned long long read[8] = {0}; int read_next = 0;      // the latest tickets whose sums were read (a repeated wait_points returns at once)
    unsigned long long order = 0, h_pts_order = 0;            // small-MSM launches in queue order; the latest non-mailing one (its results replace h_pts / h_points)
    bool host_sum(const DevCtx &c) const;                     // this process's small launches mail (the switch, and coherent host memory)
    void ensure(DevCtx &c);
    void queue(unsigned long long seq, uint32_t rows, uint32_t nchunks);   // a mailing launch was queued: its pending entry
    MsmMail *region(int r) const { return host + (size_t)r * kMsmMailCap; }
};
// per-workgroup mail lines of the persistent sum-check tail (mail.h TailMail, snark_dev.h), pinned, and the device's address of the same
struct TailMailbox { TailMail *host = nullptr, *dev = nullptr; void ensure(DevCtx &c); };
struct WaitLimits;                                           // waits.cpp: cadence, time limit and failure handling of one host wait
struct Armed { GoBox *host; GoBox *dev; unsigned long long want, deadline; int relay = 1, pollers = 1; };   // relay 0: the copy's number is polled alone and the values loaded after it (OTTI_RELAY=0; A/B)   // want == 0: not armed (values come as kernel arguments); deadline in 100 MHz ticks
constexpr unsigned long long kArmDeadlineTicks = 3000000000ull;   // 30 s of s_memrealtime: longer than any host stall the prover's own 20 s result wait tolerates
constexpr int kMaxBlocks = 2048;                             // 8 workgroups per CU; grid-stride beyond that (kernels_common.h grid_for, k_snark.hip many_grid)
constexpr size_t kArmMaxLen = 65536;                         // sum-check tables up to this length fold in <= 64 workgroups: only those launches are armed

struct DevCtx {
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr; hipEvent_t ev_side = nullptr;   // a second stream for work that runs beside a latency-bound stage (SNARK mode: hash-layer evaluations beside the second batched sum-check); made on first use
    hipStream_t side_stream();
    int device = 0, num_cu = 256;
    DevBuf<Fr> partials;                                      // [kMaxBlocks][4] per-block partial sums
    DevBuf<Fr> spmv_partial;                                  // 3 partial sums per long-row segment of the SpMV in flight
    DevBuf<Fr> results;                                       // small device result slots
    Fr *h_results = nullptr;                                  // pinned mirror of `results`
    Fr *d_results_alias = nullptr;                            // device address of h_results (zero-copy stores)
    unsigned long long *h_flag = nullptr, *d_flag_alias = nullptr, seq = 0;   // host-visible completion flag of the latest mailbox launch
    DevBuf<unsigned> d_counter;                               // arrival counter of the publishing workgroups
    DevBuf<unsigned long long> d_counts;                      // two 64-bit tallies for the kernels that count (non-canonical / small scalars / failing constraints): no allocation per call
    DevBuf<unsigned long long> sat_bits;                      // dev_check_sat: one bit per constraint row (grown on demand, kept across calls)
    DevBuf<uint32_t> sat_rows; DevBuf<Fr> sat_abc;            // its report kernel's row ids and 3 sums per row (kSatReportRows of them)
    DevBuf<unsigned long long> prod_touched;                  // dev_products_patch: one bit per constraint row a changed column reaches, then (prod_cnt) the
    DevBuf<uint32_t> prod_cnt, prod_rows;                     // words' popcounts scanned in place and the touched rows, ascending (grown on demand, kept across calls)
    std::vector<DevBuf<uint32_t>> prod_scan;                  // scan_inplace's block totals for that scan
    DevBuf<unsigned long long> diff_chunks;                   // dev_witness_diff_count: a small head, changed elements per chunk, then their prefix sums (grown on demand, kept across calls)
    Mailbox next_mailbox(int slot);
    GoBox *h_go = nullptr, *d_go_alias = nullptr; DevBuf<GoBox> d_go; unsigned long long go_issued = 0, go_published = 0;
    unsigned long long arm_deadline = kArmDeadlineTicks;     // of the launches armed from now on (the self-test shortens it)
    bool host_coherent = false;                               // the words kernels spin on / mail to are fine-grained coherent host memory (else: no armed launches)
    void reset_arrival_counters();                            // after an aborted or timed-out launch: a grid may have left them non-zero (stream must be idle)
    hipEvent_t ev_order = nullptr;                            // orders a caller's stream (otti_kd_*) against this context's own
    std::vector<struct RowSumSlot *> row_slots;               // the verifier's variable-base sums in flight on this context (prover.cpp), buffers kept across proofs
    struct BatchSumScratch *batch_sum = nullptr;              // dev_batch_sum's working memory and what its last decoding pass left resident (k_msm.hip), grow-only
    struct RowSumManyScratch *row_many = nullptr;             // dev_row_sums_many's working memory (k_msm.hip), grow-only, kept across calls
    TailMailbox tail_mail;
    // ---- host waits on device mail (waits.cpp).  The one guarded spin: polls arrived() until it holds; while it does not, fails the way lim says
    // (an armed launch that gave up; a time limit counted from t0, with release-or-drain) and ends in fail(), which throws
    template <class Pred, class OnLimit> void spin_until(Pred arrived, const WaitLimits &lim, std::chrono::steady_clock::time_point t0, OnLimit fail);
    void wait_tail(int n_groups, unsigned long long seq);     // spin until every line carries seq (throws TailTimeout at its own, short limit)
    void wait_tail_sums(int n_inst, int W, unsigned long long seq, Fr *sums);   // the same for a round's mails, summing the W partials of every instance as they arrive
    Armed arm_many(int count);                                // reserves `count` consecutive go() numbers for one persistent launch; .want = the first
    bool armed_ok() const;                                    // off under OTTI_ARMED=0, while kernel classes are being timed (a waiting kernel's duration includes the host), and
                                                              // while another proof is in flight in this process (a waiting grid holds wave slots the other proof's kernels could use: measured -15 % throughput with six in flight)
    Armed arm();                                              // for the next launch; the k-th armed launch consumes the k-th go()
    void go(const Fr *v, int n);                              // publish up to four values to the oldest armed launch that has none yet
    void go_abort();                                          // release every armed launch still waiting (they exit without touching their data) and drain the stream
    void wait_ticket(unsigned long long ticket);              // spin until the launch with that sequence number has delivered
    DevBuf<Pt> msm_keep;                                      // row sums parked on the device (MSM_KEEP)
    DevBuf<Pt> msm_partial, msm_final;                        // [rows][chunks] partial sums, [rows] row sums
    Pt *h_pts = nullptr;                                      // pinned: row sums of small launches
    size_t pending_host_encode = 0;                           // how many of them sync() has to compress (the launcher's and the waits' own: k_msm.hip, waits.cpp)
    uint8_t *h_points = nullptr;                              // pinned: compressed points coming back
    uint8_t *d_points_host = nullptr;                         // the device's address of h_points: the encode kernel writes there as well (no copy engine round trip)
    DevBuf<uint8_t> d_points;
    size_t msm_partial_cap = 0, points_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    static DevCtx &get();                                     // the calling thread's context; throws Error(OTTI_ERR_NO_DEVICE) when no device is usable
    DevCtx() {} DevCtx(const DevCtx &) = delete; DevCtx &operator=(const DevCtx &) = delete;
    struct Scratch *scratch = nullptr;                        // the prover's HBM workspace (prover.cpp); travels with the context
    struct SnarkScratch *snark_scratch = nullptr;             // SNARK mode's per-proof buffers (snark_prover.h), kept across proofs like the above
    struct EvalManyScratch *eval_many = nullptr;              // the many-point instance evaluation's tables and result memory (prover.cpp), grow-only, kept likewise
    struct ProveManyScratch *prove_many = nullptr;            // nizk_prove_many's front-half buffers (prove_many.cpp), grow-only, kept likewise
    void sync();
    void wait_points(const MsmTicket &ticket);                // results of a dev_msm_rows / dev_bullet_round launch, by the ticket's route (msm_plan.h)
    void encode_pending();
    Pt *d_pts_alias = nullptr; DevBuf<unsigned> d_counter2;
    MsmMailbox msm_mail;
    void msm_host_sum(const MsmPending &p);                  // waits for every mail of the launch and leaves its row sums in h_pts[0 .. rows)
    void ensure_points(size_t rows, size_t splits);
};
struct RowSumSlot { DevBuf<uint8_t> comp; DevBuf<Niels> pts; DevBuf<Fr> sc; DevBuf<Pt> out; DevBuf<unsigned> bad; bool busy = false; };
hipStream_t bulk_masked_stream();                                    // the process's CU-masked stream for chip-filling MSM launches beside latency-bound rounds (k_context.hip); nullptr if there is none
struct ActiveProof { ActiveProof(); ~ActiveProof(); static int count(); };       // RAII around one prove call: counts the proofs in flight in this process
constexpr int kResultSlots = 8192;                          // 256 KB pinned: round sums, sum-check tails (SNARK: up to 18 x 3 tables x 128 elements)

// per-kernel-class HIP-event timing on the library's own stream (bench.py's roofline numbers come from here)
enum KClass { KC_MSM_ROWS = 0, KC_MSM_SMALL, KC_MSM_FINISH, KC_SC_CUBIC, KC_SC_QUAD, KC_SPMV, KC_EQ, KC_REDUCE, KC_BOUND, KC_BULLET, KC_OTHER,
              KC_PC_ROUND, KC_PROD_LAYER, KC_HASH_LAYER, KC_GATHER, KC_DOT_MANY /* SNARK mode (k_snark.hip) */,
              KC_DECODE, KC_MSM_VAR /* verifier (k_msm.hip) */, KC_SAT_CHECK /* dev_sat_pass (k_sparse.hip) */, KC_COUNT };
struct KStats {
    bool on = false; unsigned mask = 0xffffffffu;            // bit k set: kernel class k is timed
    std::vector<hipEvent_t> pool; std::vector<int> cls; size_t used = 0;
    double total_ms[KC_COUNT] = {0}; unsigned long long count[KC_COUNT] = {0};
    static KStats &get();
    int begin(DevCtx &c, int k);                              // returns record index or -1
    void end(DevCtx &c, int rec);
    void flush();                                             // stream must be idle
    void reset();
};
struct KScope { DevCtx &c; int rec; KScope(DevCtx &c_, int k) : c(c_), rec(KStats::get().begin(c_, k)) {} ~KScope() { KStats::get().end(c, rec); } };

enum WitFormat { WIT_CANONICAL32 = 0, WIT_MONTGOMERY32 = 1, WIT_I64 = 2, WIT_U64 = 3 };   // = OTTI_WIT_* of the C ABI
inline size_t wit_elem_bytes(int format) { return format == WIT_I64 || format == WIT_U64 ? 8 : 32; }
// witness resident in HBM: z = vars || 1 || inputs || 0..  (2 * num_vars Montgomery-form elements)
struct DeviceWitness {
    DevBuf<Fr> z; std::vector<Fr> inputs;
    double small_fraction = 0.0;                              // share of the variables below 2^128: picks the MSM variant of the commitment
    // from a source in any WitFormat: element i at src + i * stride bytes (stride 0: packed), in device memory or, src_on_device false, host memory
    // (packed 32-byte words are copied into z and converted in place; anything else is staged as it is: an integer crosses PCIe as 8 bytes and
    // is widened on the device).  Validation (InvalidScalar) and the conversion to Montgomery form happen on the device.  producer: the stream
    // whose queued work writes a device source (nullptr: none to wait for).  Returns once the source is free again.
    DeviceWitness(const Instance &I, int format, const void *src, size_t nvars, size_t stride, bool src_on_device, hipStream_t producer, const std::vector<Fr> &inputs);
    // from the Witness messages of a .wit.zkif as the host walk located them (zkif.h ZkifWitness, k_wit_ingest.hip): the messages go to HBM as they
    // are in the file and a thread per assigned variable reads, maps, checks and converts its element — the conversion rule above — straight into z.
    // z, inputs and small_fraction come out as the constructor above leaves them for the host loader's assignment of the same files; a defect
    // throws what the host pair reports for them (the smallest key), and the fresh z goes with the object.
    DeviceWitness(const Instance &I, const struct ZkifWitness &zw);
    bool from_file_on_device = false; uint64_t file_bytes = 0;   // made by the constructor above; the witness file's size (either way through otti_witness_from_zkif)
    double file_ms[3] = {0, 0, 0};                            // its laps: host walk, staging + copies, kernel
    // straight from the caller's canonical bytes on the host: the same path
    DeviceWitness(const Instance &I, const uint8_t *vars32, size_t nvars, const std::vector<Fr> &inputs) : DeviceWitness(I, WIT_CANONICAL32, vars32, nvars, 0, false, nullptr, inputs) {}
    // variables [first, first + count) replaced likewise.  A scalar >= l throws INVALID_SCALAR and leaves z as it was (the 32-byte formats are
    // converted into a staging buffer first); afterwards small_fraction is counted again.  Not while a proof or check with this witness runs.
    void update(size_t first, int format, const void *src, size_t count, size_t stride, bool src_on_device, hipStream_t producer);
    // variables idx[0 .. count) replaced by src[0 .. count) (idx: 8-byte indices, strictly ascending and below V, in host or device memory as src is).
    // z and small_fraction come out as update leaves them.  A bad device index list throws INVALID_INDEX, then a scalar >= l INVALID_SCALAR, both
    // with z, the kept rows and the counters as they were (everything is converted into a staging buffer and judged before z is written).  Kept
    // rows are PATCHED, not summed again: the commitment is linear, so row i moves by sum (new - old) * P[j - i R] over its changed variables —
    // W table look-ups per variable (k_msm.hip k_msm_scatter) against R * W for the row's full sum.  Same threads rule as update.
    void scatter(const uint64_t *idx, int format, const void *src, size_t count, size_t stride, bool on_device, hipStream_t producer);
    unsigned long long scatter_calls = 0, rows_patched = 0, terms_patched = 0;   // since the witness was made; the last two move only while rows are kept
    // variables [first, first + count) ASSIGNED from a whole new vector of which most elements have not moved (arguments, staging and producer
    // ordering as update): the source is compared with z on the device, only the changed elements are written, and the return value is their
    // number.  z and small_fraction come out as update leaves them.  A scalar >= l throws INVALID_SCALAR with z, small_fraction, the kept rows and
    // every counter as they were (the count pass writes nothing); nothing changed: returns 0, nothing written, recounted or launched after that
    // pass.  Kept rows are patched by the compacted (index, new - old) list as scatter patches them — or, when at least kAssignResumShare of the
    // touched rows' elements changed, rows idx_min / R .. idx_max / R are summed again as update sums them.  Same threads rule as update.
    size_t assign(size_t first, int format, const void *src, size_t count, size_t stride, bool src_on_device, hipStream_t producer);
    // the dry form: the number of elements assign would change, and the lowest min(that, cap) of their indices, ascending, in idx_out (host).
    // Writes nothing to the witness and moves no counter: it reads the handle only, so it may run wherever check_sat may.
    size_t diff(size_t first, int format, const void *src, size_t count, size_t stride, bool src_on_device, hipStream_t producer, uint64_t *idx_out, size_t cap) const;
    unsigned long long assign_calls = 0, assign_changed = 0, assign_resums = 0;   // assign calls that were not refused, elements they changed, calls that summed rows again
    // the public inputs replaced, in z (z[V + 1 ..)) and in `inputs`, which the transcript reads; kept rows cover the variables alone and stay
    void set_inputs(const std::vector<Fr> &new_inputs);
    // ---- kept rows (opt-in): the unblinded row sums of the commitment, sum_j z[i * R + j] * P[j] for the L = V / R rows — the group elements the
    // proof's MSM_KEEP launch leaves in DevCtx::msm_keep.  They depend on z and on the generator POINTS alone (their stream and R; not on the
    // window width of the table they were summed with: a table released and rebuilt keeps them valid).  A proof whose generators have these
    // points reads them as the addend of its blind launch and skips the MSM_KEEP launch; sharded proofs do not look at them.  Written by
    // keep_rows and update only — both never beside a proof with this witness, so proofs need no lock to read them.
    DevBuf<Pt> rows_kept; const char *rows_stream = nullptr; size_t rows_R = 0;
    Gens *rows_gens = nullptr;                                // whose table the mutators re-sum and patch with (the caller keeps it alive while rows are kept)
    unsigned long long rows_resummed = 0;                     // rows re-summed by updates since keep_rows
    bool rows_kept_for(const Gens &g) const;                  // kept, and over g's points
    void keep_rows(Gens &g);                                  // builds g's table if need be, sums every row, returns when they are resident; again with the same points: nothing
    void drop_rows();
    // ---- kept products (opt-in): Az, Bz, Cz of this z over ONE instance's matrices (N = padded num_cons canonical Montgomery words each, bit for
    // bit what dev_spmv3 writes), the verdict bitmap dev_sat_pass writes for it and the number of failing rows.  The sums are linear in z: a changed
    // variable j moves only the rows with an entry in column j, which the instance's by-column copy lists, so every mutator brings the state up to
    // date by recomputing those rows alone (dev_products_patch, from z_written) once z is written.  An unsharded proof over that instance copies the vectors into its
    // tables instead of forming them (the tables are folded in place: the kept vectors themselves never go to a folding kernel); check_sat answers
    // from count and bitmap.  Written by keep_products, drop_products and the mutators only — never beside a proof or check with this witness, so
    // readers need no lock.  The instance must outlive the kept products.
    DevBuf<Fr> prod_abc[3]; DevBuf<unsigned long long> prod_bits, prod_unsat_dev;
    Instance *prod_inst = nullptr;                            // whose matrices they were formed with
    uint64_t prod_unsat = 0;                                  // host copy of *prod_unsat_dev
    unsigned long long prod_patches = 0, prod_rows_recomputed = 0, prod_full_passes = 0;   // since keep_products: patches that recomputed listed rows, those rows, full passes (the first included)
    // The sums hold the instance's COEFFICIENTS as well: prod_gen is the instance's generation (Instance::value_gen) they were formed at, and
    // products of another generation are stale — not kept for any reader, not patched by any mutator, recomputed by the next keep_products.
    uint64_t prod_gen = 0;
    bool products_live() const { return prod_inst && prod_abc[0].p && prod_gen == prod_inst->value_gen; }
    bool products_kept_for(const Instance &I) const { return prod_inst == &I && products_live(); }
    void keep_products(Instance &I);                          // one full pass now; again for the same instance: nothing
    void drop_products();
    static void check_range(size_t V, size_t first, size_t count);   // INVALID_NUM_VARS unless [first, first + count) lies within V variables
private:
    // What a mutator wrote into z: the range [first, first + count), or (d_idx given) an ascending device list of n indices — with, when the caller has
    // them, new - old of each (a patch of kept rows reads them) and a host copy of the list.
    struct Written {
        size_t first = 0, count = 0;
        const uint64_t *d_idx = nullptr; size_t n = 0;
        const Fr *delta = nullptr; const uint64_t *h_idx = nullptr;
        bool counted = false;                                 // the list is a count pass's on this context: dev_witness_rows_touched's tally buffer exists
        bool vars = true;                                     // variables were written; false: inputs alone, which small_fraction and kept rows do not see
    };
    struct RowsPlan { enum How { NONE, PATCH, RESUM } how = NONE; size_t r0 = 0, r1 = 0; };   // what becomes of kept rows; r0 .. r1: the rows a RESUM sums again
    // the one ending of every mutator, and the one failure rule (witness.cpp): small_fraction, kept rows, kept products, counters
    void z_written(DevCtx &c, const Written &w, RowsPlan rows);
    // the dimension checks, z allocated and zeroed, 1 || inputs queued behind the variables; returns the host copy of that tail, which has to
    // outlive the next synchronise of c.stream
    std::vector<Fr> set_up(DevCtx &c, const Instance &I, size_t nvars);
};
void ensure_device_objects(Instance &I, Gens &g);          // lazily built, shared by every prover thread (guarded)
void ensure_instance_device(Instance &I);
void ensure_gens_device(Gens &g);
void release_gens_device(Gens &g);                                     // frees the window table; the next ensure_gens_device rebuilds it
void adopt_gens_table(Gens &g, Gens &donor);                            // g drops its table and shares donor's (built if need be); prover.cpp
int device_window_bits(size_t nbases);                   // window width of the fixed-base table (prover.cpp)
// R1CSInstance::evaluate on the device: (A,B,C)(rx,ry) = <eq(rx), M * eq(ry)> for M in {A,B,C}  (verifier's O(nnz + N + V) work)
constexpr int kInstEvalSlot = 16;                            // result slots of the instance evaluation (nothing a verifier launches in between writes them)
void instance_evaluate_begin(Instance &I, const std::vector<Fr> &rx, const std::vector<Fr> &ry);      // queued on the calling thread's stream
void instance_evaluate_finish(Fr out[3]);                                                              // same thread: waits, reads
void instance_evaluate_gpu(Instance &I, const std::vector<Fr> &rx, const std::vector<Fr> &ry, Fr out[3]);
// The same three values at SEVERAL points (the points of many proofs of one instance: verify_many.cpp) with one walk over the matrices per tile of
// kEvalTile points instead of one per point (k_sparse.hip dev_eval_tile); Az, Bz, Cz are never formed.  begin queues everything on the calling
// thread's stream and returns; next / finish, on the same thread, wait and copy out[i] = (A, B, C)(rx_i, ry_i), i < the count begin was given.  Result
// memory is the pass's own (pinned, K x 3 elements): kInstEvalSlot is not touched.  Every proof's rx / ry must have the instance's lengths
// (OTTI_ERR_VERIFY_INTERNAL otherwise, before anything is queued).
// HBM: working memory is grow-only, per calling context and kept across calls, as the proof workspace is.  At most kEvalChunk points are resident at
// a time: their eq(ry) tables, 2V * 32 * kEvalChunk bytes (512 MB at V = 2^20), the factors of their eq(rx) tables (at most 2^12 + 2^13 elements
// each: 3.1 MB; the tables themselves, 32 N bytes per point, are never written), the workgroups' partial sums (under 1 MB, plus 384 bytes per
// segment of a long row) and 96 bytes per point of results.  A larger K runs in chunks of kEvalChunk, queued one behind the other.
constexpr int kEvalTile = 4;                                 // KT: points per walk over the matrices (profiles/verify_many.md)
constexpr size_t kEvalChunk = 8;                             // points whose eq tables are resident at a time
void instance_evaluate_many_begin(Instance &I, const std::vector<const NizkProof *> &proofs);
size_t instance_evaluate_many_next(Fr (*out)[3]);            // same thread: waits for the next tile, copies its values; returns how many points are in `out` by now
void instance_evaluate_many_finish(Fr (*out)[3]);            // same thread: every tile that is still out
// the same with host arrays of challenges (rx: K x log2 N, ry: K x log2 2V) and the device time of the pass from first launch to last
void instance_evaluate_many(Instance &I, const Fr *rx, size_t nrx, const Fr *ry, size_t nry, size_t K, Fr (*out)[3], float *kernel_ms);
// sh == nullptr (or a world of one): the whole proof on this GPU.  Otherwise this process proves its shard of the SAME proof as the
// other ranks of sh (collective call: same instance, witness, generators, label and seed on every rank); every rank returns the
// same bytes, equal to the single-GPU proof.
class ShardComm;
struct ProveFront;
std::vector<uint8_t> nizk_prove_resident(Instance &I, DeviceWitness &wit, Gens &g, const void *tlabel, size_t tlabel_len, const uint8_t *seed32,
                                         ProveTimings *tm, ShardComm *sh = nullptr, const ProveFront *front = nullptr);
// ---- many witnesses of one instance proved in one call (prove_many.cpp; the contract: include/otti_spartan.h otti_nizk_prove_many).  Everything a
// proof computes before its first challenge depends on the witness alone: the calling thread forms it for the whole batch in joint passes (the front
// half: prove_many_plan.h says which) on its own stream, and `threads` workers, the calling thread among them, run the sequential halves.
// results[i], proofs[i], tm[i] are what nizk_prove_resident gives for item i alone.  The handles are only read.
struct ProveManyItem { DeviceWitness *wit; const uint8_t *seed32; };
constexpr unsigned kProveManyThreads = 4, kProveManyMaxThreads = 16;      // the default is verify_many's: a process here opens four hardware queues
void nizk_prove_many(Instance &I, Gens &g, const void *tlabel, size_t tlabel_len, const ProveManyItem *items, size_t count, unsigned threads,
                     std::vector<uint8_t> *proofs, int32_t *results, ProveTimings *tm /* count, may be null */, otti_prove_many_info &info);
// the front half alone on staged vectors (otti_k_prove_front): zs[k] 2V elements in HBM, small[k] the MSM variant of vector k; rows: K * L points,
// abc[j]: K * N elements.  Synchronises.
void prove_front_staged(Instance &I, Gens &g, const Fr *const *zs, const int32_t *small, size_t K, Pt *rows, Fr *const abc[3], otti_prove_many_info &info);
// hooks: called on the proving thread the moment the first (rx) / second (ry) sum-check's challenges are complete — SNARK mode starts the
// work that depends on them alone (the two halves of the dereferenced polynomial and their commitment rows) on another stream while the
// R1CS proof goes on through its latency-bound rounds
struct R1csHooks { std::function<void(const std::vector<Fr> &)> on_rx, on_ry; std::function<void()> on_idle; };   // on_idle: from here on the proof is short rounds only (the chip is idle between them)
// What somebody else has formed of a proof's witness-only work, resident and complete before the proof starts (prove_many.cpp: the front half of a
// batch): the L unblinded row sums of the commitment over the proof's generators, and Az, Bz, Cz (N canonical Montgomery words each, bit for bit
// what dev_spmv3 writes).  A null member: the proof has its own way to that thing, as ever.  Read only; an unsharded proof alone looks at it.
struct ProveFront { const Pt *rows = nullptr; const Fr *abc[3] = {nullptr, nullptr, nullptr}; };
void r1cs_prove_device(Instance &I, DeviceWitness &wit, Gens &g, Transcript &tr, RandomTape &tape, NizkProof &P, ProveTimings &T, ShardComm *sh, const R1csHooks *hooks = nullptr,
                       const ProveFront *front = nullptr);
std::shared_ptr<DeviceShard> upload_instance_shard(const Instance &I, int rank, int world);
// DotProductProofLog::prove on the device (prover.cpp): generator stream indices of (gens_n.h, gens_1.G[0], gens_1.h) and the row length
struct PeBufs { Fr *LZ, *Rv, *a, *s, *b2, *s2, *rows, *extras; };      // R elements each (rows: 2 R, extras: 4 (log2 R + 1))
DotProductProofLog dplog_prove_device(DevCtx &c, const DeviceGens &DG, const Gens &g, const PcView &v, const PeBufs &B, const Fr &LZ_blind, const Fr *y_known,
                                      const Fr &blind_y, CPoint &Cy_out, Transcript &tr, RandomTape &tape);
// VarsAssignment::new on the device, from device memory in any WitFormat (k_field.hip): element i read at src + i * stride bytes, written in
// Montgomery form to z[dst_off + i]; src is either disjoint from the destination or is the destination itself, packed (conversion in place).
// Returns the number of non-canonical scalars (stored as zero); n_small: how many are below 2^128.  Synchronises.
size_t dev_witness_ingest_from(DevCtx &c, int format, const void *src, size_t stride, size_t n, Fr *z, size_t dst_off, size_t *n_small = nullptr);
// DeviceWitness's constructor from a .wit.zkif (k_wit_ingest.hip): z[col] written for every assigned variable of zw; returns the smallest error key
// (zkif_wit_walk.h; zw.seed when nothing sorts before it), *n_small as above; ms[1], ms[2]: staging + copies, kernel.  Synchronises.
uint64_t dev_witness_from_zkif(DevCtx &c, const struct ZkifWitness &zw, Fr *z, size_t *n_small, double ms[3]);
// DeviceWitness::scatter's two element-wise launches (k_field.hip).  check: conv[i] = element i of src in Montgomery form (the rules of
// dev_witness_ingest_from, src disjoint from conv or conv itself, packed); *bad_scalars counts those >= l, *bad_indices the i with idx[i] >= V or idx[i] <= idx[i - 1]; writes nothing else;
// synchronises.  apply (V: the length of z's first half, beyond which nothing is stored): z[idx[i]] = conv[i], and with delta given delta[i] = conv[i] - (what z[idx[i]] held); only queues.
void dev_witness_scatter_check(DevCtx &c, int format, const void *src, size_t stride, const uint64_t *d_idx, size_t n, size_t V, Fr *conv,
                               size_t *bad_scalars, size_t *bad_indices);
void dev_witness_scatter_apply(DevCtx &c, const uint64_t *d_idx, const Fr *conv, size_t n, size_t V, Fr *z, Fr *delta);
// DeviceWitness::assign / diff's launches (k_field.hip).  z: the resident range's first element.  count: the source elements whose Montgomery form
// differs from z[i] (their number, the first and the last of them; chunk by chunk into c.diff_chunks, then scanned there) and those >= l; writes
// nothing else; synchronises.  apply (behind a count over the same arguments): the changed elements once more, in ascending order — for the k-th,
// k < cap, d_idx[k] = first + i (d_idx given), delta[k] = new - old (delta given), z[i] = new (write_z); never a store beyond slot min(count, cap)
// or outside the range, whatever has become of the source since; only queues.  rows_touched (behind a count on this context): the rows of R that an
// ascending device list touches; only queues: *h_rows is filled once c.stream has been synchronised.
struct WitDiff { size_t n_changed = 0, bad_scalars = 0, lo = 0, hi = 0; };   // lo, hi: positions in the range, meaningful when n_changed > 0
size_t dev_witness_diff_chunk();                             // elements per workgroup of both passes
WitDiff dev_witness_diff_count(DevCtx &c, int format, const void *src, size_t stride, size_t n, const Fr *z);
void dev_witness_diff_apply(DevCtx &c, int format, const void *src, size_t stride, size_t n, Fr *z, size_t first, size_t cap, uint64_t *d_idx, Fr *delta, bool write_z);
void dev_witness_rows_touched(DevCtx &c, const uint64_t *d_idx, size_t n, size_t R, uint64_t *h_rows);
void dev_gather_strided(DevCtx &c, const Fr *in, size_t stride, size_t offset, Fr *out, size_t n);   // out[i] = in[i*stride + offset]

std::shared_ptr<DeviceInstance> upload_instance(const Instance &I);
std::shared_ptr<DeviceGens> build_device_gens(const Gens &g, int window_bits);

// ---- element-wise / conversion
void dev_fr_op(DevCtx &c, int op, const Fr *a, const Fr *b, Fr *out, size_t n);
// GF(2^255-19) and point formulas on a test's operands (k_curve_ops.hip): the inline functions of field.h / fp9.h / fp10.h, one case per lane (quad
// forms: four).  limbs: kFpOpLimbStride words per field element (the raw limbs of the unpacked result), four elements per point.  Only queue.
enum FpForm { FPFORM_FP8 = 0, FPFORM_F9, FPFORM_F10 };
enum FpOp { FPOP_MUL = 0, FPOP_SQR, FPOP_ADD, FPOP_SUB, FPOP_NEG, FPOP_CARRY, FPOP_REPACK, FPOP_MUL_SUB_ADD, FPOP_MUL_3A_2B, FPOP_MUL_F_E, FPOP_MUL_CARRIED_F_G, FPOP_POW22523, FPOP_COUNT };
enum PtOp { PTOP_P9_MADD = 0, PTOP_P10_MADD, PTOP_P10_ADD, PTOP_Q10_MADD, PTOP_Q10_ADD, PTOP_P9_CHAIN, PTOP_ENCODE, PTOP_DECODE, PTOP_COUNT };
constexpr int kFpOpLimbStride = 10;
void dev_fp_op(DevCtx &c, int form, int op, const Fp *a, const Fp *b, const Fp *cc, const Fp *d, Fp *out, uint32_t *limbs, size_t n);
void dev_pt_op(DevCtx &c, int op, const Pt *P, const void *Q, bool neg, uint32_t k, size_t n, Pt *out, uint32_t *limbs);
// GF(l) in nine limbs on a test's operands (k_curve_ops.hip): the inline functions of fr9.h and fold9 of kernels_common.h, one case per lane.  An
// operation reads 32-byte words (aw, bw, cw) or raw limbs (al, bl: kFr9OpLimbs words per case), whichever fr9_op_words_in / fr9_op_limbs_in say,
// and writes a word, limbs, or both; the output it does not produce is left alone.  Only queues.
enum Fr9Op { FR9OP_UNPACK = 0, FR9OP_UNPACK5, FR9OP_UNPACK10, FR9OP_MUL, FR9OP_MUL_SELF, FR9OP_ADD, FR9OP_NORM, FR9OP_SUB_KL2, FR9OP_SUB_KL4, FR9OP_SUB_KL8,
             FR9OP_SUB_KL16, FR9OP_SUB_KL128, FR9OP_FOLD_TOP, FR9OP_SHL5, FR9OP_PACK_LT2L, FR9OP_PACK_LT3L, FR9OP_CANON, FR9OP_MUL9, FR9OP_FOLD9, FR9OP_COUNT };
constexpr int kFr9OpLimbs = 9;
constexpr int fr9_op_words_in(int op) { return op <= FR9OP_UNPACK10 ? 1 : op == FR9OP_MUL9 ? 2 : op == FR9OP_FOLD9 ? 3 : 0; }
constexpr int fr9_op_limbs_in(int op) {
    return fr9_op_words_in(op) ? 0 : (op == FR9OP_MUL || op == FR9OP_ADD || (op >= FR9OP_SUB_KL2 && op <= FR9OP_SUB_KL128)) ? 2 : 1;
}
void dev_fr9_op(DevCtx &c, int op, const Fr *aw, const Fr *bw, const Fr *cw, const uint32_t *al, const uint32_t *bl, Fr *out, uint32_t *limbs, size_t n);
void dev_from_canonical(DevCtx &c, const Fr *in, Fr *out, size_t n);      // raw LE integer -> Montgomery (must be < l)
void dev_to_canonical(DevCtx &c, const Fr *in, Fr *out, size_t n);
void dev_fill_zero(DevCtx &c, Fr *p, size_t n);
// ---- K1 / K6: sparse products.  combine == false: out[k][r] = sum_p val_k[p] * x[idx_k[p]];  true: out[0][r] = sum_k coef[k] * (...)
void dev_spmv3(DevCtx &c, const DeviceCsrSet &m, const Fr *x, Fr *out0, Fr *out1, Fr *out2, bool combine, const Fr coef[3]);
// ---- A, B, C at a tile of nt <= kEvalTile points in one walk over the by-row set m (k_sparse.hip; every variant dev_spmv3 has: lane / quad, codes
// on / off, segmented long lists).  ey_il: the tile's eq(ry) tables interleaved, ey_il[col * kEvalTile + t] (2V * kEvalTile elements);
// dev_eval_point_y writes point t's table there straight from its two factors (dev_eq_factors: eq(r)[i] = hi[i >> lo_bits] * lo[i & (2^lo_bits - 1)],
// lo_bits = min(ell, 12)).  eq(rx_t) is read as its FACTORS, interleaved likewise: xlo[j * kEvalTile + t] (2^lo_bits * kEvalTile elements),
// xhi[h * kEvalTile + t] (2^hi_bits * kEvalTile); dev_eval_point_x puts point t's there.  r: host arrays, ell <= 25; scratch: 4096 + 8192 elements.
// dev_eval_tile: partial: 3 * kEvalTile * dev_eval_partial_slots(m) elements, seg_partial: 3 * kEvalTile * m.n_seg; out[t * 3 + k] (device memory),
// t < nt.  Slots t >= nt are neither read nor written.  All only queue.
struct EvalFactors { int lo_bits, hi_bits; };
EvalFactors eval_factors(size_t ell);
struct EvalTables { const Fr *xlo, *xhi, *ey_il; int xlo_bits; };
size_t dev_eval_partial_slots(const DeviceCsrSet &m);
void dev_eval_point_x(DevCtx &c, const Fr *r_host, size_t ell, int t, Fr *xlo_il, Fr *xhi_il, Fr *scratch);
void dev_eval_point_y(DevCtx &c, const Fr *r_host, size_t ell, int t, Fr *ey_il, Fr *scratch);
void dev_eval_tile(DevCtx &c, const DeviceCsrSet &m, const EvalTables &tab, int nt, Fr *partial, Fr *seg_partial, Fr *out);
// ---- dev_spmv3 for a tile of nt <= kEvalTile vectors in ONE walk over the by-row set (k_sparse.hip k_spmv3_many_*: every variant dev_spmv3 has).
// z_il: the tile's vectors interleaved, z_il[col * kEvalTile + t] over all 2V columns (dev_interleave_slot writes vector t there), so one gather of a
// column brings all the tile's values in one 128-byte run.  out.o[k][t]: matrix k's product with vector t, rows elements, canonical words bit for
// bit as dev_spmv3 writes them; slots t >= nt are neither read nor written.  seg_partial: 3 * kEvalTile * m.n_seg elements.  Both only queue.
struct SpmvManyOut { Fr *o[3][4]; };
void dev_interleave_slot(DevCtx &c, const Fr *src, size_t n, Fr *dst_il, int t);
void dev_spmv3_many(DevCtx &c, const DeviceCsrSet &m, const Fr *z_il, int nt, const SpmvManyOut &out, Fr *seg_partial);
// ---- Instance::is_sat on the device (k_sparse.hip): per constraint row r the three sums of dev_spmv3 and <A_r,z> <B_r,z> == <C_r,z>; Az, Bz, Cz
// are never written.  dev_sat_pass only queues: bits[r >> 6] bit (r & 63) is set for every FAILING row (all (rows + 63) / 64 words are written: no
// zeroing beforehand), c.d_counts[0] holds their number.  dev_check_sat runs it into the context's own bitmap, reads the count through the pinned
// result buffer and — only when it is non-zero — downloads the bitmap, lists the lowest min(count, max_rows) failing rows in ascending order
// and, with_values, recomputes their three sums (canonical little-endian bytes, 96 per row).  Reads z and the instance; writes scratch of the
// CALLER's context alone, so any thread that may prove may check.
constexpr int kSatCountSlot = 24;                            // result slot the count is copied to (clear of the rounds' and the instance evaluation's)
constexpr size_t kSatReportRows = 64;                        // rows per launch of the report kernel (one workgroup each)
struct SatReport { uint64_t n_unsat = 0; std::vector<uint64_t> rows; std::vector<uint8_t> abc96; float kernel_ms = 0; };
void dev_sat_pass(DevCtx &c, const DeviceCsrSet &m, const Fr *z, unsigned long long *bits);
uint64_t dev_sat_count(DevCtx &c);                           // waits for the pass queued last on c.stream and returns its count
SatReport dev_check_sat(DevCtx &c, DeviceInstance &d, const Fr *z, size_t max_rows, bool with_values);
// ---- kept products (k_sparse.hip): Az, Bz, Cz (N canonical Montgomery words each), the verdict bitmap of dev_sat_pass's layout and the failing count
// *d_unsat that go with them are brought up to date for a z of which the listed columns have changed.  Three steps: the by-column lists of the
// changed columns MARK their rows in c.prod_touched (zeroed first; atomicOr), the bitmap is COMPACTED into the ascending row list c.prod_rows
// (popcount per word, scan_inplace; the length comes back through the pinned result slot: one synchronise), and the listed rows are RECOMPUTED from
// the by-row set — sums, verdict bit, and the count moved by the difference.  From full_share * N touched rows on, the full pass runs instead:
// dev_spmv3 into the vectors, then every verdict from them (dev_products_full).  Every index followed comes from the instance's own CSR copies or
// from d_cols, which the CALLER has checked (ascending, below 2 * num_vars).  Returns with the stream idle.
constexpr int kProdCountSlot = 26;                           // result slots 26, 27: the touched count and the failing count
// The share of the N rows from which the full pass replaces the patch.  Measured, profiles/witness_products.md (tools/witness_products_probe.py, 2^20,
// device time): the smallest probed share at which the patch was no longer shorter than dev_spmv3 + dev_sat_pass, as the code without kept products
// runs them, was 0.33 on the uniform instance and 0.57 on the compiler-like one; the lower of the two, rounded down to a power of two (toward the
// full pass).  OTTI_PRODUCTS_FULL_SHARE, read per call, overrides it: 0 always takes the full pass, a value >= 1 never does.
constexpr double kProductsFullShare = 0.25;
double products_full_share();
struct ProductsPatch { size_t n_touched = 0; bool full = false; uint64_t n_unsat = 0; float kernel_ms = 0; };   // kernel_ms: first launch to last, the host's read of n_touched in between included
void dev_products_full(DevCtx &c, const DeviceInstance &d, const Fr *z, Fr *Az, Fr *Bz, Fr *Cz, unsigned long long *bits, unsigned long long *d_unsat);   // only queues
ProductsPatch dev_products_patch(DevCtx &c, const DeviceInstance &d, const Fr *z, const uint64_t *d_cols, size_t ncols, size_t first, size_t count,
                                 Fr *Az, Fr *Bz, Fr *Cz, unsigned long long *bits, unsigned long long *d_unsat);
// the failing rows of a bitmap whose count is known, listed and (with_values) recomputed as dev_check_sat reports them; kernel_ms: the report launches
void dev_sat_report(DevCtx &c, DeviceInstance &d, const Fr *z, const unsigned long long *d_bits, size_t max_rows, bool with_values, bool timed, SatReport &rep);
// ---- K2: eq tables.  r is a HOST array (challenges come from the transcript)
void dev_eq_evals(DevCtx &c, const Fr *r_host, size_t ell, Fr *out, Fr *scratch /* >= 3 * 4096 elements; 5 * 4096 for ell = 25 */);
void dev_eq_evals2(DevCtx &c, const Fr *r0_host, size_t ell0, Fr *out0, const Fr *r1_host, size_t ell1, Fr *out1, Fr *scratch);   // both in one launch when each has at most 13 variables
void dev_eq_factors(DevCtx &c, const Fr *r_host, size_t ell, size_t lo_bits, Fr *lo /* 2^lo_bits */, Fr *hi /* 2^(ell - lo_bits) */);   // eq(r)[i] = hi[i >> lo_bits] * lo[i & (2^lo_bits - 1)]: the factors alone, one launch
// ---- K3/K4/K5/K7: sum-check rounds.  Results land in c.h_results[slot .. slot+k)
// each returns a ticket: c.wait_ticket(ticket) returns once h_results[slot..] hold that launch's sums (no stream synchronise)
unsigned long long dev_sc_cubic_eval(DevCtx &c, const Fr *A, const Fr *B, const Fr *C, const Fr *D, size_t len, int slot);
unsigned long long dev_sc_cubic_fold_eval(DevCtx &c, Fr *A, Fr *B, Fr *C, Fr *D, size_t len, const Fr &r, int slot);   // len >= 4; folds to len/2, sums over the folded tables
// phase one with the eq table factored out (see k_sumcheck.hip): E[i] = hi ? hi[i >> lo_bits] * lo[i & (2^lo_bits - 1)] : lo[i]
struct EqSrc { const Fr *hi, *lo; int lo_bits;
               uint32_t stride = 1, offset = 0;      // table index of a kernel's item i is i * stride + offset (a rank's residue class of a sharded table; 1, 0 otherwise)
               // one more variable ABOVE the tabulated ones (eq_at only): E[i] = (bit top_bit of i ? top : 1 - top) * table[i mod 2^top_bit].  The product
               // circuits' pyramids leave a layer's first variable out — it is the last challenge to be drawn, and without it they are built ahead of time
               int top_bit = -1; Fr top; };
void dev_eq_pyramid(DevCtx &c, const Fr *r_host, size_t n, Fr *out /* 2^(n+1) - 1 elements: level k at out + 2^k - 1 */);
void dev_eq_pyramid2(DevCtx &c, const Fr *r0_host, size_t n0, Fr *out0, const Fr *r1_host, size_t n1, Fr *out1);   // two in one launch (out1 may be null)
unsigned long long dev_sc_cubic3_eval(DevCtx &c, const Fr *B, const Fr *C, const Fr *D, size_t len, const EqSrc &E, int slot);
unsigned long long dev_sc_cubic3_fold_eval(DevCtx &c, Fr *B, Fr *C, Fr *D, size_t len, const Fr &r, const EqSrc &E, int slot);
// armed variants (see Armed above): the fold challenge is the next value published with c.go()
unsigned long long dev_sc_cubic3_fold_eval_armed(DevCtx &c, Fr *B, Fr *C, Fr *D, size_t len, const EqSrc &E, int slot);
unsigned long long dev_sc_quad_fold_eval_armed(DevCtx &c, Fr *A, Fr *B, size_t len, int slot);
unsigned long long dev_sc_quad_eval(DevCtx &c, const Fr *A, const Fr *B, size_t len, int slot);
unsigned long long dev_sc_quad_fold_eval(DevCtx &c, Fr *A, Fr *B, size_t len, const Fr &r, int slot);
const ScCaps &sc_caps(DevCtx &c);                   // what sc_plan() (sc_plan.h) is told about this device: it sets the grid of every launch above
void sc_caps_override(const ScCaps *caps);          // tests only: capacities sc_caps() returns in the device's place until nullptr takes them back; refused while a proof is in flight
void dev_fold_top(DevCtx &c, Fr *Z, size_t len, const Fr &r);
void dev_fold_bot(DevCtx &c, const Fr *Z, Fr *out, size_t len, const Fr &r);
void dev_fetch(DevCtx &c, const Fr *src, int slot, size_t n);              // async copy of n elements into h_results[slot..]
// ---- K8: fixed-base MSM rows.  Row i: sum_j dense[i*n_dense + j] * P[j] (j < n_dense) + sum_e extra_s[i*n_extra+e] * P[extra_base[e]]
// Compressed results land in c.h_points[32*i ..] after c.sync(); those of more than kHostEncodeRows rows, or with an addend, also stay in c.d_points.
// What to sum, filled with designated initialisers at the call site.  The row stride of `dense` is n_dense.
struct MsmJob {
    const Fr *dense = nullptr; size_t n_dense = 0, rows = 0;
    const Fr *extra_s = nullptr; const uint32_t *extra_base = nullptr /* host */; size_t n_extra = 0;
    int mode = MSM_COMPRESSED;                                // msm_plan.h
    const Pt *addend = nullptr;
    // sparse: the dense scalars are mostly small numbers (more than kSparseWitness of them, DeviceWitness::small_fraction) — bulk launches then
    // compact the non-zero (term, window) pairs into a work list instead of giving every pair a lane.  Results are identical either way.
    bool sparse = false;
    Pt *keep_dst = nullptr; bool force_bulk = false;
    size_t bulk_workgroups = kMsmBulkWorkgroups;              // msm_plan.h MsmShape: only otti_k_msm_job (the tests) sets another value
};
constexpr double kSparseWitness = 0.25;                      // above this share of small scalars a commitment uses the work-list MSM variant
// returns a ticket: c.wait_points(ticket) returns once the compressed points are in c.h_points
MsmTicket dev_msm_rows(DevCtx &c, const DeviceGens &g, const MsmJob &job);
MsmPlan dev_msm_plan(DevCtx &c, const DeviceGens &g, const MsmJob &job);   // the plan dev_msm_rows takes for this job (the same call of msm_plan())
double dev_small_fraction(DevCtx &c, const Fr *z, size_t n);               // share of scalars below 2^128 (synchronises the stream)
// MSM_RAW: skip compression; after c.sync() the extended row sums are in c.h_pts[0..rows).
// MSM_KEEP: no output; the row sums stay on the device in c.msm_keep (to be passed as `addend` of a later launch, which then
// compresses (row sum + addend)).  Lets the host draw the blinds while the device already sums the witness terms.
// keep_dst (MSM_KEEP only): row i's sum goes to keep_dst[i] instead, c.msm_keep is left alone (DeviceWitness::rows_kept: the caller offsets it
// to the first of the rows to sum, as it does `dense`).  force_bulk: the chip-filling kernel whatever the size (a run of re-summed rows).
// ---- (index, scalar) lists summed into row sums that stay on the device (k_msm.hip k_msm_scatter; DeviceWitness::scatter):
// rows[i] += sum over {k : d_idx[k] in [i R, (i + 1) R)} d_s[k] * P[d_idx[k] - i R] for i < L.  d_idx: strictly ascending, below L * R (the
// CALLER has checked that: the kernel takes a term's table column from it); d_s Montgomery.  One workgroup per row; a row without terms is not
// touched.  Only queues.
void dev_msm_scatter(DevCtx &c, const DeviceGens &g, const uint64_t *d_idx, const Fr *d_s, size_t count, size_t R, Pt *rows, size_t L);
void dev_encode_points(DevCtx &c, const Pt *pts, size_t n, uint8_t *d_out32, const Pt *addend = nullptr);   // RFC 9496 encodings of n extended points, of pts[i] + addend[i] with an addend (only queues)
// ---- K9: LZ[j] = sum_i Lv[i] * Z[i*R + j]
void dev_poly_bound(DevCtx &c, const Fr *Z, size_t L, size_t R, const Fr *Lv, Fr *out, Fr *scratch /* >= 64*R */);
// chunk sums of the same bound over eq(rest) alone (k_sumcheck.hip): out = (L / m) x R; false (nothing launched) when the geometry does not allow it
bool dev_poly_bound_chunks(DevCtx &c, const Fr *Z, size_t L, size_t R, const Fr *Lv_rest, size_t m, Fr *out, Fr *scratch /* >= 64*R */);
// dot product of two device vectors -> h_results[slot]
void dev_dot(DevCtx &c, const Fr *a, const Fr *b, size_t n, int slot);
// ---- K10: bullet reduction bookkeeping on the ORIGINAL generators (see prover.cpp)
// One launch per round.  If fold_first, a and b (length 2*n_cur) are folded to n_cur with (u, u_inv) and s is updated; then, for
// n_cur >= 2, the next round's c_L, c_R go to extra_out[0], extra_out[2] and the dense scalar rows sL, sR (length R each) to rows[0..2R).
void dev_bullet_step(DevCtx &c, Fr *a, Fr *b, Fr *s, size_t R, size_t n_cur, bool fold_first, const Fr &u, const Fr &u_inv, Fr *rows, Fr *extra_out);
void dev_bullet_finish(DevCtx &c, Fr *a, Fr *b, Fr *s, size_t R, const Fr &u, const Fr &u_inv, const Fr &d, Fr *rows, int slot_a);   // last fold (2 -> 1), a, b to result slots slot_a, slot_a + 1, rows = d s
// One bullet-reduction round as ONE launch: applies the previous challenge (fold), derives the scalars of L and R from the round state
// and sums both rows (fused finish; compressed L, R arrive in c.h_points[0..64) after c.wait_points(ticket)).  extra_s: 4 scalars
// {unused, blind_L, unused, blind_R} (the c_L / c_R terms are computed in the kernel); extra_base: {Q, H}.
// armed (device.h): u and u_inv are not known yet; the launch takes {u, u_inv, raw(u), raw(u_inv)} from the next c.go()
struct BulletRound {
    size_t R, n_cur; bool fold; Fr u, u_inv;
    const Fr *a_in, *b_in, *s_in; Fr *a_out, *b_out, *s_out;
    const Fr *extra_s; const uint32_t *extra_base; bool armed = false;
};
MsmTicket dev_bullet_round(DevCtx &c, const DeviceGens &g, const BulletRound &round);
// ---- verifier: decompression of n ristretto255 points into affine Niels form (bad: count of encodings that do not decode), and the
// variable-base MSM over them: out[w * splits + s] = sum over the points of split s of digit_w(scalar) * point — window sums the host
// combines (253 doublings: a sequential chain a host core runs 30 x faster than a GPU lane).  Returns the window width c it used.
void dev_decode_niels(DevCtx &c, const uint8_t *compressed_dev, size_t n, Niels *out, unsigned *bad);
int dev_msm_var(DevCtx &c, const Niels *pts, const Fr *scalars, size_t n, Pt *out, size_t out_cap, int *n_windows, int *n_splits);
// ---- several such sums in one pass (k_msm.hip k_decode_niels_sets, k_msm_var_many): what the staged SNARK verifier (snark_verify_many.cpp) sends
// for all its live proofs at one of its three seams.  A set is n compressed points in HOST memory, decoded in the pass with a counter of its own,
// or — `decoded` given — n points already in HBM in the form the sums read (a commitment's, decoded once: dev_decode_set), with what that decode
// found.  A job is a set and n scalars (host, Montgomery); several jobs may name one set, and sets of different n share the launch: every job
// takes the c, W and splits dev_msm_var takes for its n.  Queues one upload each of points, scalars and tables, one decode launch (counted under
// `decode`), one sum launch (`msm_var`) and the copies back on c.stream, waits, and recombines each job's windows on the host as the single
// row sum does: out[j] = {0, the sum} or {OTTI_ERR_VERIFY_DECOMPRESS} exactly when job j's set has a point that does not decode — its neighbours
// are untouched.  OTTI_ERR_BAD_ARG (nothing queued): no sets or jobs, a set of fewer than 1 or more than kRowSumMaxPoints points, a job naming no set.
// HBM: grow-only per context, 160 bytes per point to decode, 32 per scalar, 128 per (window, split) — at most 51 * ceil(n / 2048) per job.
constexpr size_t kRowSumMaxPoints = (size_t)1 << 20;
struct RowSumSetIn { const uint8_t *comp32 = nullptr; size_t n = 0; const Niels *decoded = nullptr; bool decoded_bad = false; };
struct RowSumJobIn { size_t set = 0; const Fr *scalars = nullptr; };
struct RowSumOut { int code = 0; Pt sum; };
void dev_row_sums_many(DevCtx &c, const RowSumSetIn *sets, size_t nsets, const RowSumJobIn *jobs, size_t njobs, RowSumOut *out);
// ---- the weighted sum of a batch of proofs' group equations (verify_batch.cpp; the same two kernels): nsets sets of compressed points in HOST
// memory, one behind the other (set k: points [set_off[k], set_off[k + 1]), nsets + 1 ascending offsets from 0) — one set per proof — go up once and
// are decoded by ONE launch with a counter per set; the generators take part as one more set, index nsets, already in HBM in the form the sums read
// (decoded once per generators handle).  A job sums `nsets` CONSECUTIVE sets from first_set on — they are contiguous in HBM, so a job over all of
// them is the whole batch's sum and a job over one set is one proof's — or the generator set alone (first_set == in.nsets, nsets == 1), with one
// scalar per point (host, Montgomery); jobs may overlap and name a set several times.  ONE k_msm_var_many launch forms all jobs' sums; out[j] is
// {0, the sum} or {OTTI_ERR_VERIFY_DECOMPRESS} exactly when one of job j's sets holds a point that does not decode.  reuse: a second pass over the
// sets the context's LAST pass decoded (the same offsets, or OTTI_ERR_INTERNAL): nothing goes up or is decoded again, and a job over uploaded sets
// may leave scalars null to take those its points got from the first job of that pass, if that job spanned all sets — the localisation pass sends
// only the generator scalars.  ms (may be null): device-event time of the launches.  Waits; recombines the windows on the host as the row sums do.
// HBM: grow-only per context, 32 + 96 bytes per point, 32 per scalar (twice for a second pass), 128 per (window, split) — at most 51 * ceil(n / 2048) per job.
// A SNARK batch has two generator handles: a second resident set, gens2, is set index nsets + 1.  A job on a generator set carries either host
// scalars, as above, or — scalars null — {base, runs}: its scalars are formed in HBM by k_gen_runs, launched on the same stream just ahead of the
// sums, straight into the slice the job's sum reads: sc[i] = base[i] + sum over the runs r with i < 2^lg_r of c_r * prod_{bit t of i set} f_r[t].
// base: n dense scalars (host, Montgomery) or null for zeros.  A run of more slots than its set has points is OTTI_ERR_BAD_ARG.
struct GenRunIn { Fr c; uint32_t lg = 0; const Fr *f = nullptr; };         // host: coefficient, lg factors (Montgomery)
struct BatchSumIn {
    const uint8_t *comp32 = nullptr; const size_t *set_off = nullptr; size_t nsets = 0; const Niels *gens = nullptr; size_t ngens = 0; bool gens_bad = false, reuse = false;
    const Niels *gens2 = nullptr; size_t ngens2 = 0; bool gens2_bad = false;
};
struct BatchSumJobIn { size_t first_set = 0, nsets = 1; const Fr *scalars = nullptr; const Fr *base = nullptr; const GenRunIn *runs = nullptr; size_t nruns = 0; };
// The expansion alone (k_msm.hip k_gen_runs, one thread per (job, slot), the runs' factors staged in LDS a tile at a time, no atomics): job j writes
// n scalars to out_dev, which is device memory.  Queues the tables' upload and the launch on c.stream and returns; `keep` holds the host and
// device staging, so it must live until the stream has drained.  Throws OTTI_ERR_BAD_ARG before anything is queued: no jobs, a job of no slots or
// more than kRowSumMaxPoints, a run with 2^lg > n or without its factors.
constexpr uint32_t kGenRunMaxLg = 20, kGenRunTile = 8;
struct GenRunsJobIn { size_t n = 0; const Fr *base = nullptr; const GenRunIn *runs = nullptr; size_t nruns = 0; Fr *out_dev = nullptr; };
struct GenRunDev { Fr c; uint32_t lg, f_off, job, pad; };
struct GenRunsJobDev { Fr *out; const Fr *base; uint32_t n, run_first, run_count, pad; };
struct GenRunsStaging {
    DevBuf<Fr> base, fac; DevBuf<GenRunDev> runs; DevBuf<GenRunsJobDev> jobs; DevBuf<uint32_t> first;
    std::vector<Fr> h_base, h_fac; std::vector<GenRunDev> h_runs; std::vector<GenRunsJobDev> h_jobs; std::vector<uint32_t> h_first;
};
void dev_gen_runs(DevCtx &c, const GenRunsJobIn *jobs, size_t njobs, GenRunsStaging &keep);
void dev_batch_sum(DevCtx &c, const BatchSumIn &in, const BatchSumJobIn *jobs, size_t njobs, RowSumOut *out, float *ms);
const unsigned *dev_batch_sum_bad(DevCtx &c);                              // per set of the last decoding pass: how many of its points did not decode
struct DecodedSet { DevBuf<Niels> pts; size_t n = 0; bool bad = false; };      // bad: some encoding did not decode (the identity stands in its place)
void dev_decode_set(DevCtx &c, const uint8_t *comp32, size_t n, DecodedSet &out);   // host bytes -> HBM; synchronises
double dev_madd_peak(DevCtx &c);                                          // mixed point additions per second, whole chip (the MSM's ALU roof)
// v[i] (times *factor when given: a device-resident scalar is not needed, it travels by value) as 8 u32 limbs widened to u64 lanes, on `st`
void dev_fr_to_lanes(hipStream_t st, const Fr *d_src, const Fr *factor, unsigned long long *d_lanes, size_t n);
double dev_fr_mul_peak(DevCtx &c);                                        // Montgomery products in GF(l) per second, whole chip (the streaming kernels' second roof)
void dev_scale(DevCtx &c, const Fr *in, const Fr &k, Fr *out, size_t n);
void dev_fill_one(DevCtx &c, Fr *p, size_t n);

}  // namespace otti
