// The witness resident in HBM (device.h DeviceWitness): how z is made from a caller's source, the four mutators (update, scatter, assign, set_inputs),
// assign's dry form, and the derived state a witness may keep — row sums of the commitment, Az / Bz / Cz — which every mutator brings along through
// ONE ending, z_written.  The provers read wit.z, rows_kept_for and products_kept_for and nothing else of this file.
#include "device.h"
#include "zkif.h"
#include <cstring>

namespace otti {

namespace {
// Where dev_witness_ingest_from reads a source: a device source as it is, once the context's stream waits for the producer's queued work (an event
// recorded there, as the otti_kd_* calls order a caller's stream against the context's own); a host source from a copy on the device — packed
// 32-byte words straight in `dst` when the caller names one (they are converted in place there: no staging allocation), anything else in a
// staging copy of its span.
struct WitSource {
    DevBuf<uint8_t> staged; const void *p = nullptr; size_t stride = 0;
    WitSource(DevCtx &c, int format, const void *src, size_t n, size_t stride_, bool on_device, hipStream_t producer, Fr *dst) {
        const size_t eb = wit_elem_bytes(format);
        stride = stride_ ? stride_ : eb; p = src;
        if (!n) return;
        if (on_device) {
            if (producer && producer != c.stream) {
                if (!c.ev_order) OTTI_HIP(hipEventCreateWithFlags(&c.ev_order, hipEventDisableTiming));
                OTTI_HIP(hipEventRecord(c.ev_order, producer)); OTTI_HIP(hipStreamWaitEvent(c.stream, c.ev_order, 0));
            }
            return;
        }
        const size_t span = (n - 1) * stride + eb;
        if (dst && eb == sizeof(Fr) && stride == eb) p = dst;
        else { staged.alloc(span); p = staged.p; }
        OTTI_HIP(hipMemcpyAsync(const_cast<void *>(p), src, span, hipMemcpyHostToDevice, c.stream));
    }
};
}  // namespace

void DeviceWitness::check_range(size_t V, size_t first, size_t count) {
    if (first > V || count > V - first) throw Error(OTTI_ERR_INVALID_NUM_VARS, "the range ends beyond the instance's variables");
}

std::vector<Fr> DeviceWitness::set_up(DevCtx &c, const Instance &I, size_t nvars) {
    const size_t V = I.num_vars;
    if (nvars > V) throw Error(OTTI_ERR_INVALID_NUM_VARS, "more variables than the instance has");
    if (inputs.size() != I.num_inputs) throw Error(OTTI_ERR_INVALID_NUM_INPUTS, "wrong number of inputs");
    z.alloc(2 * V);
    OTTI_HIP(hipMemsetAsync(z.p, 0, 2 * V * sizeof(Fr), c.stream));
    // z = vars || 1 || inputs || 0...   (r1csproof.rs: "append input to variables to create a single vector z")
    std::vector<Fr> tail(1 + inputs.size()); tail[0] = fr_one();
    for (size_t i = 0; i < inputs.size(); i++) tail[1 + i] = inputs[i];
    OTTI_HIP(hipMemcpyAsync(z.p + V, tail.data(), tail.size() * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
    return tail;
}

DeviceWitness::DeviceWitness(const Instance &I, int format, const void *src, size_t nvars, size_t stride, bool src_on_device, hipStream_t producer,
                             const std::vector<Fr> &inputs_) : inputs(inputs_) {
    DevCtx &c = DevCtx::get();
    const size_t V = I.num_vars;
    const std::vector<Fr> tail = set_up(c, I, nvars);
    WitSource s(c, format, src, nvars, stride, src_on_device, producer, z.p);    // a fresh z may be written before the check: a refusal throws it away
    size_t n_small = 0;
    const size_t bad = dev_witness_ingest_from(c, format, s.p, s.stride, nvars, z.p, 0, &n_small);   // synchronises: `tail`, the staging copy and the caller's buffer are free again
    if (!nvars) OTTI_HIP(hipStreamSynchronize(c.stream));
    if (bad) throw Error(OTTI_ERR_INVALID_SCALAR, "non-canonical scalar in assignment");
    small_fraction = V ? (double)(n_small + (V - nvars)) / (double)V : 0.0;        // the padding zeros count as small
}

DeviceWitness::DeviceWitness(const Instance &I, const ZkifWitness &zw) : inputs(zw.inputs) {
    DevCtx &c = DevCtx::get();
    const size_t V = I.num_vars, nvars = zw.have_witness ? zw.num_vars : 0;
    if (zw.witness_bytes >= ((size_t)1 << 34)) throw Error(OTTI_ERR_BAD_ARG, "witness file too large for the device ingest (16 GiB)");
    const std::vector<Fr> tail = set_up(c, I, nvars);
    size_t n_small = 0;
    const uint64_t key = dev_witness_from_zkif(c, zw, z.p, &n_small, file_ms);   // synchronises: `tail` is free again; a fresh z is thrown away on a refusal
    if (key != kZwNoError) zkif_witness_refuse(zw, key);
    small_fraction = V ? (double)(n_small + (V - nvars)) / (double)V : 0.0;        // the padding zeros count as small
    from_file_on_device = true; file_bytes = zw.witness_bytes;
}

// ---- kept rows.  Rows [r0, r1] of z summed over g's table into their slots of rows_kept, by the launch the proof's own commitment would make for
// them: up to two rows the latency-bound kernel (as every launch of at most two rows), a longer run one chip-filling launch with the proof's
// sparse rule.  Returns once they are resident: the next proof may run on another thread's stream.
static void sum_rows_into(DevCtx &c, DeviceWitness &w, Gens &g, size_t r0, size_t r1, bool whole) {
    ensure_gens_device(g);
    const DeviceGens &DG = *g.dev;
    const size_t R = w.rows_R, n = r1 - r0 + 1;
    // the whole vector goes the way the proof's MSM_KEEP launch goes (same size rule); a run of dirty rows is bulk from three rows on
    dev_msm_rows(c, DG, {.dense = w.z.p + r0 * R, .n_dense = R, .rows = n, .mode = MSM_KEEP, .sparse = w.small_fraction > kSparseWitness,
                         .keep_dst = w.rows_kept.p + r0, .force_bulk = !whole && n > 2});
    OTTI_HIP(hipStreamSynchronize(c.stream));
}

// ---- the one ending of every mutator: z holds the new values `w` describes, and the derived state follows, in this order (the order is behaviour):
//   1. kept rows, PATCH: the table made sure of, the patch (k_msm.hip k_msm_scatter: n * W table look-ups) and the count of touched rows — a host list
//      is counted on the host, a count pass's list by dev_witness_rows_touched (its tally lives in that pass's buffer), any other device list is read
//      back into this frame — all queued before
//   2. the recount of small_fraction when variables were written: one pass over them, never incremental; synchronises;
//   3. kept rows, RESUM: rows r0 .. r1 summed again behind the recount, because the launch picks its sparse variant by the new share; synchronises;
//   4. kept products: the rows the written columns reach recomputed (dev_products_patch; synchronises);
//   5. the counters, which therefore move only when all of it went through.
// Patch, re-sum or neither is the caller's decision (`rows`; NONE when no rows are kept).
// THE FAILURE RULE, for every mutator: z has been written, so whatever throws from here on, the context's stream is synchronised first — nothing
// queued here or by the caller then still reads the caller's buffers (conv, delta, idx, a staged index list, a WitSource's staging copy: all owned by
// the caller's frame, which outlives this call) or writes this frame's — then whichever derived state, rows or products, was not brought up to date
// is dropped, because it no longer belongs to z, and the error goes on to the caller.
void DeviceWitness::z_written(DevCtx &c, const Written &w, RowsPlan rows) {
    bool rows_ok = rows.how == RowsPlan::NONE, products_ok = false;
    uint64_t touched = 0; std::vector<uint64_t> back; ProductsPatch p;
    try {
        if (rows.how == RowsPlan::PATCH) {
            ensure_gens_device(*rows_gens);
            dev_msm_scatter(c, *rows_gens->dev, w.d_idx, w.delta, w.n, rows_R, rows_kept.p, rows_kept.n);
            if (w.counted) dev_witness_rows_touched(c, w.d_idx, w.n, rows_R, &touched);
            else if (!w.h_idx) { back.resize(w.n); OTTI_HIP(hipMemcpyAsync(back.data(), w.d_idx, w.n * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream)); }
        }
        if (w.vars) small_fraction = dev_small_fraction(c, z.p, z.n / 2);        // the padding zeros count as small
        if (rows.how == RowsPlan::RESUM) sum_rows_into(c, *this, *rows_gens, rows.r0, rows.r1, false);
        rows_ok = true;
        if (products_live()) p = dev_products_patch(c, *prod_inst->dev, z.p, w.d_idx, w.n, w.first, w.count, prod_abc[0].p, prod_abc[1].p, prod_abc[2].p, prod_bits.p, prod_unsat_dev.p);
        products_ok = true;
    } catch (...) {
        (void)hipStreamSynchronize(c.stream);
        if (!rows_ok) drop_rows();
        if (!products_ok) drop_products();
        throw;
    }
    if (rows.how == RowsPlan::PATCH) {
        if (!w.counted) { const uint64_t *ix = w.h_idx ? w.h_idx : back.data(); for (size_t i = 0; i < w.n; i++) touched += i == 0 || ix[i] / rows_R != ix[i - 1] / rows_R; }
        rows_patched += touched; terms_patched += w.n;
    }
    if (rows.how == RowsPlan::RESUM) rows_resummed += rows.r1 - rows.r0 + 1;
    if (products_live()) {
        prod_unsat = p.n_unsat;
        if (p.full) prod_full_passes++;
        else if (p.n_touched) { prod_patches++; prod_rows_recomputed += p.n_touched; }
    }
}

void DeviceWitness::update(size_t first, int format, const void *src, size_t count, size_t stride, bool src_on_device, hipStream_t producer) {
    DevCtx &c = DevCtx::get();
    check_range(z.n / 2, first, count);
    if (!count) return;
    // every integer is a scalar: straight into place.  A 32-byte range is converted in `conv` (a packed host one is copied there and converted
    // in place), and z is written only once the whole range has passed the check
    const bool ints = format == WIT_I64 || format == WIT_U64;
    DevBuf<Fr> conv(ints ? 0 : count);
    WitSource s(c, format, src, count, stride, src_on_device, producer, conv.p);
    if (ints) dev_witness_ingest_from(c, format, s.p, s.stride, count, z.p, first);
    else {
        if (dev_witness_ingest_from(c, format, s.p, s.stride, count, conv.p, 0)) throw Error(OTTI_ERR_INVALID_SCALAR, "non-canonical scalar in the update: the witness is unchanged");
        OTTI_HIP(hipMemcpyAsync(z.p + first, conv.p, count * sizeof(Fr), hipMemcpyDeviceToDevice, c.stream));
    }
    // kept rows: the rows the range touches are summed again (a refused scalar threw above, with z and the kept rows as they were)
    z_written(c, {.first = first, .count = count}, rows_kept.p ? RowsPlan{RowsPlan::RESUM, first / rows_R, (first + count - 1) / rows_R} : RowsPlan{});
}

// ---- scatter update.  Behind the same staging and producer-stream ordering as update (host indices are staged like host values), the check
// (everything converted into `conv`, bad indices and scalars counted: one synchronise, and a refusal has written nothing), the apply (z, and the deltas
// when rows are kept), and the ending, which patches kept rows.
void DeviceWitness::scatter(const uint64_t *idx, int format, const void *src, size_t count, size_t stride, bool on_device, hipStream_t producer) {
    DevCtx &c = DevCtx::get();
    const size_t V = z.n / 2;
    if (count > V) throw Error(OTTI_ERR_INVALID_INDEX, "more indices than the instance has variables");
    if (!count) return;
    DevBuf<Fr> conv(count), delta;
    WitSource s(c, format, src, count, stride, on_device, producer, conv.p);   // a device source: the one event orders the producer of both lists
    DevBuf<uint64_t> idx_staged; const uint64_t *d_idx = idx;
    if (!on_device) {
        idx_staged.alloc(count); d_idx = idx_staged.p;
        OTTI_HIP(hipMemcpyAsync(idx_staged.p, idx, count * sizeof(uint64_t), hipMemcpyHostToDevice, c.stream));
    }
    const bool patch = rows_kept.p != nullptr;
    if (patch) delta.alloc(count);
    size_t bad_scalars = 0, bad_indices = 0;
    dev_witness_scatter_check(c, format, s.p, s.stride, d_idx, count, V, conv.p, &bad_scalars, &bad_indices);
    if (bad_indices) throw Error(OTTI_ERR_INVALID_INDEX, "the indices are not strictly ascending below the padded num_vars: the witness is unchanged");
    if (bad_scalars) throw Error(OTTI_ERR_INVALID_SCALAR, "non-canonical scalar in the scatter: the witness is unchanged");
    dev_witness_scatter_apply(c, d_idx, conv.p, count, V, z.p, patch ? delta.p : nullptr);
    z_written(c, {.d_idx = d_idx, .n = count, .delta = delta.p, .h_idx = on_device ? nullptr : idx}, patch ? RowsPlan{RowsPlan::PATCH} : RowsPlan{});
    scatter_calls++;
}

// ---- assign: a whole new vector of which most elements have not moved.  Behind the same staging and producer-stream ordering as update (a host
// source is staged as it is, never converted into a copy: both passes convert on the fly): the count pass (changed elements per chunk, scalars >= l;
// and the first and last changed element; one synchronise, and a refusal or "nothing changed" ends here with nothing written), the apply pass (z, and
// for a patch the ascending list of changed indices and their deltas), and the ending — kept rows patched by the list as scatter patches them, or, from
// kAssignResumShare of the touched rows' elements on, rows idx_min / R .. idx_max / R summed again as update sums them.
// The share of touched_rows * R changed elements from which summing the touched rows again replaces the patch (a value >= 1: never).  Measured,
// profiles/witness_assign.md (tools/witness_assign_probe.py, 2^20, kept rows): the smallest probed share at which a round trip with the patch forced
// was no longer shorter than one with the re-sum of the same range forced, on the same witness, was 1/2 (at 1/8 the patch still won clearly), for small
// int64 numbers and for uniform canonical bytes alike.
constexpr double kAssignResumShare = 0.5;
// OTTI_ASSIGN_RESUM_SHARE, read per call, overrides it: 0 sums again whenever anything changed, a value >= 1 never does (tests pin both paths with it)
static double assign_resum_share() {
    if (const char *e = getenv("OTTI_ASSIGN_RESUM_SHARE")) { char *end = nullptr; const double v = strtod(e, &end); if (end != e && v >= 0) return v; }
    return kAssignResumShare;
}
size_t DeviceWitness::assign(size_t first, int format, const void *src, size_t count, size_t stride, bool src_on_device, hipStream_t producer) {
    DevCtx &c = DevCtx::get();
    check_range(z.n / 2, first, count);
    if (!count) return 0;
    WitSource s(c, format, src, count, stride, src_on_device, producer, nullptr);
    const WitDiff d = dev_witness_diff_count(c, format, s.p, s.stride, count, z.p + first);
    if (d.bad_scalars) throw Error(OTTI_ERR_INVALID_SCALAR, "non-canonical scalar in the assignment: the witness is unchanged");
    assign_calls++;
    const size_t n_changed = d.n_changed;
    if (!n_changed) return 0;
    assign_changed += n_changed;
    // kept rows: patched, or rows r0 .. r1 summed again — known before anything is written, so only a patch pays for the list and the deltas
    RowsPlan rows;
    if (rows_kept.p) {
        rows.r0 = (first + d.lo) / rows_R; rows.r1 = (first + d.hi) / rows_R;
        const double share = assign_resum_share();
        rows.how = share < 1.0 && (double)n_changed >= share * (double)((rows.r1 - rows.r0 + 1) * rows_R) ? RowsPlan::RESUM : RowsPlan::PATCH;
    }
    DevBuf<uint64_t> idx; DevBuf<Fr> delta;
    if (rows.how == RowsPlan::PATCH) { idx.alloc(n_changed); delta.alloc(n_changed); }
    else if (products_live()) idx.alloc(n_changed);                     // kept products are patched by the list of changed columns, whatever becomes of kept rows
    dev_witness_diff_apply(c, format, s.p, s.stride, count, z.p + first, first, n_changed, idx.p, delta.p, true);
    z_written(c, {.d_idx = idx.p, .n = n_changed, .delta = delta.p, .counted = true}, rows);
    if (rows.how == RowsPlan::RESUM) assign_resums++;
    return n_changed;
}
size_t DeviceWitness::diff(size_t first, int format, const void *src, size_t count, size_t stride, bool src_on_device, hipStream_t producer, uint64_t *idx_out,
                           size_t cap) const {
    DevCtx &c = DevCtx::get();
    check_range(z.n / 2, first, count);
    if (!count) return 0;
    WitSource s(c, format, src, count, stride, src_on_device, producer, nullptr);
    const WitDiff d = dev_witness_diff_count(c, format, s.p, s.stride, count, z.p + first);
    if (d.bad_scalars) throw Error(OTTI_ERR_INVALID_SCALAR, "non-canonical scalar in the assignment");
    const size_t n_changed = d.n_changed, k = std::min(n_changed, cap);
    if (k) {
        DevBuf<uint64_t> idx(k);
        dev_witness_diff_apply(c, format, s.p, s.stride, count, z.p + first, first, k, idx.p, nullptr, false);
        OTTI_HIP(hipMemcpyAsync(idx_out, idx.p, k * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipStreamSynchronize(c.stream));
    }
    return n_changed;
}
void DeviceWitness::set_inputs(const std::vector<Fr> &new_inputs) {
    DevCtx &c = DevCtx::get();
    if (new_inputs.size() != inputs.size()) throw Error(OTTI_ERR_INVALID_NUM_INPUTS, "wrong number of inputs");
    const size_t V = z.n / 2;
    if (!new_inputs.empty()) {
        OTTI_HIP(hipMemcpyAsync(z.p + V + 1, new_inputs.data(), new_inputs.size() * sizeof(Fr), hipMemcpyHostToDevice, c.stream));
        OTTI_HIP(hipStreamSynchronize(c.stream));
    }
    inputs = new_inputs;
    if (!new_inputs.empty()) z_written(c, {.first = V + 1, .count = new_inputs.size(), .vars = false}, RowsPlan{});   // inputs are columns of z too
}
// ---- kept products (device.h).  keep: the full pass, once; every mutator's ending patches them once z holds the new values.
void DeviceWitness::keep_products(Instance &I) {
    DevCtx &c = DevCtx::get();
    if (I.num_vars * 2 != z.n) throw Error(OTTI_ERR_INVALID_NUM_VARS, "the witness was uploaded for an instance of other dimensions");
    if (products_kept_for(I)) return;
    ensure_instance_device(I);
    drop_products();
    const size_t N = I.num_cons;
    try {
        for (int k = 0; k < 3; k++) prod_abc[k].alloc(N);
        prod_bits.alloc((N + 63) >> 6); prod_unsat_dev.alloc(1);
        prod_inst = &I; prod_gen = I.value_gen;
        dev_products_full(c, *I.dev, z.p, prod_abc[0].p, prod_abc[1].p, prod_abc[2].p, prod_bits.p, prod_unsat_dev.p);
        unsigned long long n = 0;
        OTTI_HIP(hipMemcpyAsync(&n, prod_unsat_dev.p, sizeof n, hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipStreamSynchronize(c.stream));
        prod_unsat = n; prod_full_passes = 1;
    } catch (...) { (void)hipStreamSynchronize(c.stream); drop_products(); throw; }
}
void DeviceWitness::drop_products() {
    for (int k = 0; k < 3; k++) prod_abc[k].release();
    prod_bits.release(); prod_unsat_dev.release();
    prod_inst = nullptr; prod_gen = 0; prod_unsat = 0; prod_patches = prod_rows_recomputed = prod_full_passes = 0;
}
bool DeviceWitness::rows_kept_for(const Gens &g) const { return rows_kept.p && rows_R == g.R && rows_stream && !strcmp(rows_stream, g.stream); }
void DeviceWitness::keep_rows(Gens &g) {
    DevCtx &c = DevCtx::get();
    const size_t V = z.n / 2;
    if (g.num_vars_padded != V || !g.R || V % g.R) throw Error(OTTI_ERR_BAD_ARG, "generators were made for a different instance size");
    if (rows_kept_for(g)) { rows_gens = &g; return; }
    drop_rows();
    rows_kept.alloc(V / g.R); rows_stream = g.stream; rows_R = g.R; rows_gens = &g; rows_resummed = 0;
    try { sum_rows_into(c, *this, g, 0, V / g.R - 1, true); } catch (...) { drop_rows(); throw; }
}
void DeviceWitness::drop_rows() { rows_kept.release(); rows_stream = nullptr; rows_R = 0; rows_gens = nullptr; rows_resummed = 0; }

}  // namespace otti
