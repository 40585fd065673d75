// extern "C" surface of libottispartan (include/otti_spartan.h).  No exception crosses this boundary.
#include "capi_common.h"

otti_r1cs *otti_r1cs_from(size_t nc, size_t nv, size_t ni, const std::vector<otti_entry> &A, const std::vector<otti_entry> &B,
                          const std::vector<otti_entry> &C, const std::vector<uint8_t> &vars, const std::vector<uint8_t> &inputs);
otti_r1cs *zkif_load_impl(const char *circuit_path, const char *inputs_path, const char *witness_path);
void zkif_write_impl(const otti_r1cs *r, const char *circuit_path, const char *inputs_path, const char *witness_path);
otti_r1cs *zkif_load_inputs_impl(const char *inputs_path);
namespace otti { otti_r1cs *instance_from_zkif_device(const char *circuit_path, const char *inputs_path, const char *witness_path, std::unique_ptr<Instance> &inst); }   // k_ingest.hip
#include "zkif.h"
#include "coo_walk.h"
#include <sys/stat.h>
#include <unistd.h>
// otti_instance_from_zkif(OTTI_INGEST_AUTO): the circuit sizes between which the device path is taken (OTTI_INGEST_MIN_MB, OTTI_INGEST_GB override them
// per call; OTTI_INGEST_GB=0: never).  Where they come from: profiles/zkif_ingest.md.
constexpr double kIngestMinMB = 15.0;                       // MiB: the smallest probed circuit (2^16 uniform, 15.2 MiB) — the device path's median beat the host path's beyond both spreads at every probed size
// otti_witness_from_zkif(OTTI_INGEST_AUTO): the witness file's size from which the device path is taken (OTTI_INGEST_WIT_MIN_MB overrides it per call).
// Where it comes from: profiles/zkif_witness_ingest.md.
constexpr double kIngestWitMinMB = 10.0;                   // MiB: 2^18 variables (10.0 MiB) — the smallest probed size at which the device path's median beat the host path's beyond both spreads; at 2^16 (2.5 MiB) it did not
constexpr double kIngestGB = 8.0;                            // image + 40-byte entries + both CSR copies of such a file stay far below one card's HBM

thread_local std::string g_last_error;
// VarsAssignment::new + pad, InputsAssignment::new
static void load_assignment(const Instance &I, const uint8_t *vars32, size_t nvars, const uint8_t *inputs32, size_t ninputs, std::vector<Fr> &vars, std::vector<Fr> &inputs) {
    if (nvars > I.num_vars) throw Error(OTTI_ERR_INVALID_NUM_VARS, "more variables than the instance has");
    if (ninputs != I.num_inputs) throw Error(OTTI_ERR_INVALID_NUM_INPUTS, "wrong number of inputs");
    vars = scalars_from_bytes(vars32, nvars); vars.resize(I.num_vars, fr_zero());
    inputs = scalars_from_bytes(inputs32, ninputs);
}

// ---- a witness from host bytes, from device memory, from host integers, and changed in place (device.h WitFormat, k_field.hip k_witness_ingest_from).  Everything
// that can be said about the arguments alone is said before DevCtx::get() brings a device up.
static void check_wit_source(const void *src, size_t count, int32_t format, size_t stride_bytes, bool on_device) {
    if (format < OTTI_WIT_CANONICAL32 || format > OTTI_WIT_U64) throw Error(OTTI_ERR_BAD_ARG, "unknown witness format");
    if (!src && count) throw Error(OTTI_ERR_BAD_ARG, "null source with a non-zero count");
    if (stride_bytes && (stride_bytes < wit_elem_bytes(format) || stride_bytes % 8)) throw Error(OTTI_ERR_BAD_ARG, "stride_bytes below the element size or not a multiple of 8");
    if (on_device && ((uintptr_t)src & 7)) throw Error(OTTI_ERR_BAD_ARG, "a device source must be 8-byte aligned");
}
// a witness that keeps products (device.h DeviceWitness::prod_abc) is changed through the instance they were formed with, and no other: said before
// z is written, so the refusal changes nothing
static void check_products_instance(const otti_witness *wit, const Instance &I) {
    if (wit->w->prod_inst && wit->w->prod_inst != &I) throw Error(OTTI_ERR_BAD_ARG, "the witness keeps products for another instance: the witness is unchanged");
}
// ---- the entries that change or compare a resident witness.  ONE ladder of refusals, in the order the header states for each of them: a null handle or
// pointer (BAD_ARG), then `early` — everything the arguments alone say: the source (check_wit_source), the range or the index list as far as the host can
// see it; it returns false to end the call there with OTTI_OK (an empty range is answered before a device is asked for) — then a missing device, said
// before the witness handle is looked at, the witness's dimensions, for a mutator the instance its products were kept for, and the body.
template <class Early, class Body>
static int32_t witness_entry(otti_instance *inst, const otti_witness *wit, bool pointers_ok, bool mutates, Early early, Body body) {
    return guarded([&] {
        if (!inst || !wit || !pointers_ok) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (!early(inst->I->num_vars)) return OTTI_OK;
        DevCtx::get();
        check_witness_dims(wit, *inst->I);
        if (mutates) check_products_instance(wit, *inst->I);
        body(*wit->w);
        return OTTI_OK;
    });
}
// the entries that only read a handle or free what it keeps: null, no device (then no witness handle can exist: wit is not looked at), the body
template <class Body> static int32_t witness_read(const otti_witness *wit, Body body) {
    return guarded([&] {
        if (!wit) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (otti_device_count() < 1) throw Error(OTTI_ERR_NO_DEVICE, "no device: no witness handle can exist");
        body(*wit->w);
        return OTTI_OK;
    });
}

extern "C" {

size_t otti_last_error(char *buf, size_t cap) {
    if (buf && cap) { size_t n = std::min(cap - 1, g_last_error.size()); memcpy(buf, g_last_error.data(), n); buf[n] = 0; }
    return g_last_error.size();
}
void otti_buf_free(void *p) { free(p); }

int32_t otti_device_count(void) {
    // asked once: on a host without a GPU every hipGetDeviceCount call re-probes the driver (~0.2 s of system time)
    static const int count = [] { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }();
    return count;
}

int32_t otti_instance_new(uint64_t nc, uint64_t nv, uint64_t ni, const otti_entry *A, size_t nA, const otti_entry *B, size_t nB,
                          const otti_entry *C, size_t nC, otti_instance **out) {
    return guarded([&] {
        if (!out) throw Error(OTTI_ERR_BAD_ARG, "null out pointer");
        return adopt(out, instance_new(nc, nv, ni, A, nA, B, nB, C, nC));
    });
}
void otti_instance_free(otti_instance *p) { delete p; }
int32_t otti_instance_dims(const otti_instance *inst, uint64_t *nc, uint64_t *nv, uint64_t *ni) {
    if (!inst) return OTTI_ERR_BAD_ARG;
    if (nc) *nc = inst->I->num_cons; if (nv) *nv = inst->I->num_vars; if (ni) *ni = inst->I->num_inputs;
    return OTTI_OK;
}
int32_t otti_instance_is_sat(const otti_instance *inst, const uint8_t *vars32, size_t nvars, const uint8_t *inputs32, size_t ninputs, int32_t *sat) {
    return guarded([&] {
        if (!inst || !sat) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        std::vector<Fr> vars, inputs; load_assignment(*inst->I, vars32, nvars, inputs32, ninputs, vars, inputs);
        *sat = inst->I->is_sat(vars, inputs) ? 1 : 0; return OTTI_OK;
    });
}

int32_t otti_gens_new(uint64_t nc, uint64_t nv, uint64_t ni, otti_gens **out) {
    return guarded([&] {
        if (!out) throw Error(OTTI_ERR_BAD_ARG, "null out pointer");
        return adopt(out, gens_new(nc, nv, ni));
    });
}
void otti_gens_free(otti_gens *p) { delete p; }
int32_t otti_gens_table_info(const otti_gens *gens, uint32_t *window_bits, uint64_t *table_bytes) {
    return guarded([&] {
        if (!gens) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        const DeviceGens *d = gens->g->dev.get();
        if (window_bits) *window_bits = d ? (uint32_t)d->c : 0;
        if (table_bytes) *table_bytes = d ? (uint64_t)d->table.n * sizeof(TabEntry) : 0;
        return OTTI_OK;
    });
}
int32_t otti_gens_build_ms(const otti_gens *gens, double *alloc_ms, double *kernels_ms) {
    return guarded([&] {
        if (!gens) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        const DeviceGens *d = gens->g->dev.get();
        if (alloc_ms) *alloc_ms = d ? d->build_ms[0] : 0.0;
        if (kernels_ms) *kernels_ms = d ? d->build_ms[1] : 0.0;
        return OTTI_OK;
    });
}
int32_t otti_gens_release_device(otti_gens *gens) {
    return guarded([&] {
        if (!gens) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        release_gens_device(*gens->g);
        return OTTI_OK;
    });
}
int32_t otti_gens_adopt_table(otti_gens *gens, otti_gens *donor) {
    return guarded([&] {
        if (!gens || !donor) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (gens == donor) throw Error(OTTI_ERR_BAD_ARG, "a handle cannot adopt its own table");
        Gens &g = *gens->g, &d = *donor->g;
        if (strcmp(g.stream, d.stream)) throw Error(OTTI_ERR_BAD_ARG, "the donor's points come from another generator stream");
        if (d.P.size() < g.P.size()) throw Error(OTTI_ERR_BAD_ARG, "the donor has fewer points than these generators need");
        adopt_gens_table(g, d);
        return OTTI_OK;
    });
}
int32_t otti_gens_table_users(const otti_gens *gens, uint32_t *users, const void **d_table) {
    return guarded([&] {
        if (!gens) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        const std::shared_ptr<DeviceGens> &d = gens->g->dev;
        if (users) *users = d ? (uint32_t)d.use_count() : 0;
        if (d_table) *d_table = d ? (const void *)d->table.p : nullptr;
        return OTTI_OK;
    });
}
int32_t otti_gens_points(const otti_gens *gens, uint8_t *out32, size_t count) {
    return guarded([&] {
        if (!gens || count > gens->g->P.size()) throw Error(OTTI_ERR_BAD_ARG, "count exceeds the generator stream");
        for (size_t i = 0; i < count; i++) pt_encode(out32 + 32 * i, gens->g->P[i]);
        return OTTI_OK;
    });
}

int32_t otti_prepare_device(otti_instance *inst, otti_gens *gens) {
    return guarded([&] {
        if (inst) ensure_instance_device(*inst->I);
        if (inst && gens) ensure_device_objects(*inst->I, *gens->g);
        else if (gens) ensure_gens_device(*gens->g);
        else if (!inst) DevCtx::get();                              // neither: just bring the HIP runtime and this process's device context up
        return OTTI_OK;
    });
}

int32_t otti_nizk_prove(otti_instance *inst, const uint8_t *vars32, size_t nvars, const uint8_t *inputs32, size_t ninputs, otti_gens *gens,
                        const uint8_t *tlabel, size_t tlabel_len, const uint8_t *seed32, uint32_t flags, uint8_t **proof, size_t *proof_len,
                        double *stage_ms) {
    return guarded([&] {
        if (!inst || !gens || !proof || !proof_len) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (!(flags & OTTI_FLAG_GPU)) throw Error(OTTI_ERR_BAD_ARG, "OTTI_FLAG_GPU is the only proving backend; there is no CPU path");
        if (ninputs != inst->I->num_inputs) throw Error(OTTI_ERR_INVALID_NUM_INPUTS, "wrong number of inputs");
        std::vector<Fr> inputs = scalars_from_bytes(inputs32, ninputs);
        ProveTimings tm{};
        DeviceWitness w(*inst->I, vars32, nvars, inputs);          // VarsAssignment::new (InvalidScalar) is checked on the device
        std::vector<uint8_t> pf = nizk_prove_resident(*inst->I, w, *gens->g, tlabel, tlabel_len, seed32, &tm);
        return emit_proof(pf, tm, proof, proof_len, stage_ms);
    });
}
void otti_witness_free(otti_witness *w) { delete w; }
static int32_t witness_from(otti_instance *inst, const void *src, size_t nvars, int32_t format, size_t stride_bytes, bool on_device, const uint8_t *inputs32,
                            size_t ninputs, void *stream, otti_witness **out) {
    return guarded([&] {
        if (!inst || !out || (!inputs32 && ninputs)) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        check_wit_source(src, nvars, format, stride_bytes, on_device);
        if (nvars > inst->I->num_vars) throw Error(OTTI_ERR_INVALID_NUM_VARS, "more variables than the instance has");
        if (ninputs != inst->I->num_inputs) throw Error(OTTI_ERR_INVALID_NUM_INPUTS, "wrong number of inputs");
        std::vector<Fr> inputs = scalars_from_bytes(inputs32, ninputs);
        return adopt(out, std::make_unique<DeviceWitness>(*inst->I, format, src, nvars, stride_bytes, on_device, (hipStream_t)stream, inputs));
    });
}
int32_t otti_witness_upload(otti_instance *inst, const uint8_t *vars32, size_t nvars, const uint8_t *inputs32, size_t ninputs, otti_witness **out) {
    return witness_from(inst, vars32, nvars, OTTI_WIT_CANONICAL32, 0, false, inputs32, ninputs, nullptr, out);
}
int32_t otti_witness_from_device(otti_instance *inst, const void *d_vars, size_t nvars, int32_t format, size_t stride_bytes, const uint8_t *inputs32, size_t ninputs,
                                 void *stream, otti_witness **out) {
    return witness_from(inst, d_vars, nvars, format, stride_bytes, true, inputs32, ninputs, stream, out);
}
int32_t otti_witness_upload_ints(otti_instance *inst, const void *vars, size_t nvars, int32_t format, const uint8_t *inputs32, size_t ninputs, otti_witness **out) {
    if (format != OTTI_WIT_I64 && format != OTTI_WIT_U64) return guarded([&]() -> int32_t { throw Error(OTTI_ERR_BAD_ARG, "otti_witness_upload_ints takes OTTI_WIT_I64 or OTTI_WIT_U64"); });
    return witness_from(inst, vars, nvars, format, 0, false, inputs32, ninputs, nullptr, out);
}
int32_t otti_witness_update(otti_instance *inst, otti_witness *wit, size_t first, const void *src, size_t count, int32_t format, size_t stride_bytes,
                            int32_t src_on_device, void *stream) {
    return witness_entry(inst, wit, true, true,
        [&](size_t V) { check_wit_source(src, count, format, stride_bytes, src_on_device != 0); DeviceWitness::check_range(V, first, count); return true; },
        [&](DeviceWitness &w) { w.update(first, format, src, count, stride_bytes, src_on_device != 0, (hipStream_t)stream); });
}
// ---- scatter update (device.h DeviceWitness::scatter).  `early`: the arguments (BAD_ARG), then the index list as far as the host can see it (INVALID_INDEX:
// its length, and a host list itself in one pass); on the device a bad device index list is refused before a scalar >= l.
int32_t otti_witness_scatter(otti_instance *inst, otti_witness *wit, const uint64_t *idx, const void *src, size_t count, int32_t format, size_t stride_bytes,
                             int32_t on_device, void *stream) {
    return witness_entry(inst, wit, true, true,
        [&](size_t V) {
            check_wit_source(src, count, format, stride_bytes, on_device != 0);
            if (!idx && count) throw Error(OTTI_ERR_BAD_ARG, "null index list with a non-zero count");
            if (on_device && ((uintptr_t)idx & 7)) throw Error(OTTI_ERR_BAD_ARG, "a device index list must be 8-byte aligned");
            if (count > V) throw Error(OTTI_ERR_INVALID_INDEX, "more indices than the instance has variables");
            if (!on_device)
                for (size_t i = 0; i < count; i++)
                    if (idx[i] >= V || (i && idx[i] <= idx[i - 1])) throw Error(OTTI_ERR_INVALID_INDEX, "the indices are not strictly ascending below the padded num_vars");
            return true;
        },
        [&](DeviceWitness &w) { w.scatter(idx, format, src, count, stride_bytes, on_device != 0, (hipStream_t)stream); });
}
int32_t otti_witness_scatter_info(const otti_witness *wit, uint64_t *calls, uint64_t *rows_patched, uint64_t *terms_patched) {
    return witness_read(wit, [&](const DeviceWitness &w) {
        if (calls) *calls = w.scatter_calls;
        if (rows_patched) *rows_patched = w.rows_patched;
        if (terms_patched) *terms_patched = w.terms_patched;
    });
}
// ---- assign and its dry form (device.h DeviceWitness::assign / diff): otti_witness_update's order of refusals, and an empty range ends in `early`
int32_t otti_witness_assign(otti_instance *inst, otti_witness *wit, size_t first, const void *src, size_t count, int32_t format, size_t stride_bytes,
                            int32_t src_on_device, void *stream, uint64_t *n_changed) {
    return witness_entry(inst, wit, true, true,
        [&](size_t V) {
            check_wit_source(src, count, format, stride_bytes, src_on_device != 0); DeviceWitness::check_range(V, first, count);
            if (n_changed) *n_changed = 0;
            return count != 0;
        },
        [&](DeviceWitness &w) {
            const size_t n = w.assign(first, format, src, count, stride_bytes, src_on_device != 0, (hipStream_t)stream);
            if (n_changed) *n_changed = n;
        });
}
int32_t otti_witness_diff(otti_instance *inst, const otti_witness *wit, size_t first, const void *src, size_t count, int32_t format, size_t stride_bytes,
                          int32_t src_on_device, void *stream, uint64_t *n_changed, uint64_t *idx, size_t idx_cap) {
    return witness_entry(inst, wit, n_changed && (idx || !idx_cap), false,
        [&](size_t V) {
            check_wit_source(src, count, format, stride_bytes, src_on_device != 0); DeviceWitness::check_range(V, first, count);
            *n_changed = 0;
            return count != 0;
        },
        [&](const DeviceWitness &w) { *n_changed = w.diff(first, format, src, count, stride_bytes, src_on_device != 0, (hipStream_t)stream, idx, idx_cap); });
}
int32_t otti_witness_assign_info(const otti_witness *wit, uint64_t *calls, uint64_t *changed, uint64_t *resums) {
    return witness_read(wit, [&](const DeviceWitness &w) {
        if (calls) *calls = w.assign_calls;
        if (changed) *changed = w.assign_changed;
        if (resums) *resums = w.assign_resums;
    });
}
int32_t otti_witness_set_inputs(otti_instance *inst, otti_witness *wit, const uint8_t *inputs32, size_t ninputs) {
    std::vector<Fr> inputs;
    return witness_entry(inst, wit, inputs32 || !ninputs, true,
        [&](size_t) {
            if (ninputs != inst->I->num_inputs) throw Error(OTTI_ERR_INVALID_NUM_INPUTS, "wrong number of inputs");
            inputs = scalars_from_bytes(inputs32, ninputs);       // INVALID_SCALAR: a host check, the witness is not touched
            return true;
        },
        [&](DeviceWitness &w) { w.set_inputs(inputs); });
}
int32_t otti_witness_info(const otti_witness *wit, const void **d_z, size_t *n, double *small_fraction) {
    return guarded([&] {
        if (!wit) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (d_z) *d_z = wit->w->z.p;
        if (n) *n = wit->w->z.n;
        if (small_fraction) *small_fraction = wit->w->small_fraction;
        return OTTI_OK;
    });
}
// ---- kept rows (device.h DeviceWitness::rows_kept).  As with the calls above, the arguments are judged first, a missing device is reported next,
// and only then is the witness handle looked at (none can exist without a device).
static int32_t witness_keep_rows(otti_instance *inst, otti_witness *wit, Gens *g) {
    return witness_entry(inst, wit, g != nullptr, false,
        [&](size_t V) { if (g->num_vars_padded != V) throw Error(OTTI_ERR_BAD_ARG, "generators were made for a different instance size"); return true; },
        [&](DeviceWitness &w) { w.keep_rows(*g); });
}
int32_t otti_witness_keep_rows(otti_instance *inst, otti_witness *wit, otti_gens *gens) { return witness_keep_rows(inst, wit, gens ? gens->g.get() : nullptr); }
int32_t otti_witness_keep_rows_snark(otti_instance *inst, otti_witness *wit, otti_snark_gens *gens) { return witness_keep_rows(inst, wit, gens ? gens->g->sat.get() : nullptr); }
int32_t otti_witness_drop_rows(otti_witness *wit) { return witness_read(wit, [](DeviceWitness &w) { w.drop_rows(); }); }
int32_t otti_witness_rows_info(const otti_witness *wit, int32_t *kept, size_t *L, size_t *R, uint64_t *rows_resummed) {
    return witness_read(wit, [&](const DeviceWitness &w) {
        if (kept) *kept = w.rows_kept.p ? 1 : 0;
        if (L) *L = w.rows_kept.n;
        if (R) *R = w.rows_R;
        if (rows_resummed) *rows_resummed = w.rows_resummed;
    });
}
// ---- kept products (device.h DeviceWitness::prod_abc), in the order of the kept-rows calls: the arguments, a missing device, the witness's dimensions
int32_t otti_witness_keep_products(otti_instance *inst, otti_witness *wit) {
    return witness_entry(inst, wit, true, false, [](size_t) { return true; }, [&](DeviceWitness &w) { w.keep_products(*inst->I); });
}
int32_t otti_witness_drop_products(otti_witness *wit) { return witness_read(wit, [](DeviceWitness &w) { w.drop_products(); }); }
int32_t otti_witness_products_info(const otti_witness *wit, int32_t *kept, size_t *n_rows, const void **d_Az, const void **d_Bz, const void **d_Cz,
                                   uint64_t *n_unsat, uint64_t *patches, uint64_t *rows_recomputed, uint64_t *full_passes) {
    return witness_read(wit, [&](const DeviceWitness &w) {
        if (kept) *kept = w.products_live() ? 1 : 0;                 // (products of an earlier coefficient generation are not kept: device.h prod_gen)
        if (n_rows) *n_rows = w.prod_abc[0].n;
        if (d_Az) *d_Az = w.prod_abc[0].p;
        if (d_Bz) *d_Bz = w.prod_abc[1].p;
        if (d_Cz) *d_Cz = w.prod_abc[2].p;
        if (n_unsat) *n_unsat = w.prod_unsat;
        if (patches) *patches = w.prod_patches;
        if (rows_recomputed) *rows_recomputed = w.prod_rows_recomputed;
        if (full_passes) *full_passes = w.prod_full_passes;
    });
}
int32_t otti_nizk_prove_resident(otti_instance *inst, otti_witness *wit, otti_gens *gens, const uint8_t *tlabel, size_t tlabel_len,
                                 const uint8_t *seed32, uint8_t **proof, size_t *proof_len, double *stage_ms) {
    return guarded([&] {
        if (!inst || !wit || !gens || !proof || !proof_len) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        ProveTimings tm{};
        std::vector<uint8_t> pf = nizk_prove_resident(*inst->I, *wit->w, *gens->g, tlabel, tlabel_len, seed32, &tm);
        return emit_proof(pf, tm, proof, proof_len, stage_ms);
    });
}
// Instance::is_sat on the resident assignment, with a diagnosis (device.h dev_check_sat).  No host fallback: without a device DevCtx::get throws.
int32_t otti_witness_check_sat(otti_instance *inst, otti_witness *wit, uint64_t *n_unsat, uint64_t *rows, size_t rows_cap, uint8_t *abc96, float *kernel_ms) {
    return guarded([&] {
        if (!inst || !wit || !n_unsat || (rows_cap && !rows)) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        Instance &I = *inst->I;
        check_witness_dims(wit, I);
        DevCtx &c = DevCtx::get(); ensure_instance_device(I);
        SatReport rep;
        // a witness that keeps its products for this instance is answered from their count and bitmap: no pass; failing rows are reported as ever
        if (wit->w->products_kept_for(I)) { rep.n_unsat = wit->w->prod_unsat; dev_sat_report(c, *I.dev, wit->w->z.p, wit->w->prod_bits.p, rows_cap, abc96 != nullptr, true, rep); }
        else rep = dev_check_sat(c, *I.dev, wit->w->z.p, rows_cap, abc96 != nullptr);
        *n_unsat = rep.n_unsat;
        for (size_t i = 0; i < rep.rows.size(); i++) rows[i] = rep.rows[i];
        if (abc96 && !rep.abc96.empty()) memcpy(abc96, rep.abc96.data(), rep.abc96.size());
        if (kernel_ms) *kernel_ms = rep.kernel_ms;
        return OTTI_OK;
    });
}
int32_t otti_shard_init(const char *segment_name, uint32_t rank, uint32_t world) {
    return guarded([&] {
        if (!segment_name) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        shard_comm_set(nullptr);
        shard_comm_set(new ShardComm(segment_name, (int)rank, (int)world));
        return OTTI_OK;
    });
}
int32_t otti_shard_info(uint32_t *rank, uint32_t *world, uint32_t *transport) {
    return guarded([&] {
        need_shard();
        if (rank) *rank = (uint32_t)shard_comm()->rank(); if (world) *world = (uint32_t)shard_comm()->world();
        if (transport) *transport = (uint32_t)shard_comm()->transport();
        return OTTI_OK;
    });
}
int32_t otti_shard_finalize(void) { return guarded([&] { shard_comm_set(nullptr); return OTTI_OK; }); }
int32_t otti_shard_allgather(const void *mine, size_t nbytes, void *out) {
    return guarded([&] {
        need_shard();
        if (!mine || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        shard_comm()->allgather(mine, nbytes, out); return OTTI_OK;
    });
}
int32_t otti_shard_allreduce(uint8_t *scalars32, size_t count) {
    return guarded([&] {
        need_shard();
        std::vector<Fr> v = scalars_from_bytes(scalars32, count);
        shard_comm()->allreduce_fr(v.data(), count);
        for (size_t i = 0; i < count; i++) fr_to_bytes(scalars32 + 32 * i, v[i]);
        return OTTI_OK;
    });
}
int32_t otti_nizk_prove_sharded(otti_instance *inst, otti_witness *wit, otti_gens *gens, const uint8_t *tlabel, size_t tlabel_len,
                                const uint8_t *seed32, uint8_t **proof, size_t *proof_len, double *stage_ms) {
    return guarded([&] {
        if (!inst || !wit || !gens || !proof || !proof_len) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        need_shard();
        if (!seed32) throw Error(OTTI_ERR_BAD_ARG, "a sharded proof needs an explicit random-tape seed (the same on every rank)");
        ProveTimings tm{};
        std::vector<uint8_t> pf = nizk_prove_resident(*inst->I, *wit->w, *gens->g, tlabel, tlabel_len, seed32, &tm, shard_comm());
        return emit_proof(pf, tm, proof, proof_len, stage_ms);
    });
}
int32_t otti_nizk_verify(const otti_instance *inst, const uint8_t *inputs32, size_t ninputs, const otti_gens *gens, const uint8_t *tlabel,
                         size_t tlabel_len, const uint8_t *proof, size_t proof_len) {
    return guarded([&] {
        if (!inst || !gens || !proof) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        std::vector<Fr> inputs = scalars_from_bytes(inputs32, ninputs);
        // The verifier is host code (as in the reference); only its O(nnz + N + V) step — evaluating A, B, C at (rx, ry) — goes to the
        // device when one is present.  (Verification is not the proving hot path: without a device it simply stays on the host.)
        // The evaluation is QUEUED here (its point is in the proof) and collected where the verifier needs it, after the sum-check rounds.
        bool queued = false;
        if (inst->I->num_cons >= 4096 && otti_device_count() > 0) {
            try {
                NizkProof P = NizkProof::parse(proof, proof_len);
                instance_evaluate_begin(*const_cast<Instance *>(inst->I.get()), P.rx, P.ry); queued = true;
            } catch (const Error &) { queued = false; }
        }
        const InstEvalFetch fetch = [](Fr out[3]) { instance_evaluate_finish(out); };
        int rc = nizk_verify(*inst->I, inputs, *gens->g, tlabel, tlabel_len, proof, proof_len, nullptr, queued ? &fetch : nullptr);
        if (rc) g_last_error = "proof rejected";
        return rc;
    });
}
int32_t otti_nizk_verify_many(const otti_instance *inst, const otti_gens *gens, const uint8_t *tlabel, size_t tlabel_len, size_t count,
                              const uint8_t *const *inputs32, const size_t *ninputs, const uint8_t *const *proofs, const size_t *proof_lens,
                              uint32_t threads, int32_t *results, size_t *n_rejected) {
    return guarded([&] {
        if (!inst || !gens || !results) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (threads > kVerifyManyMaxThreads) throw Error(OTTI_ERR_BAD_ARG, "more than 16 worker threads");
        if (count && (!inputs32 || !ninputs || !proofs || !proof_lens)) throw Error(OTTI_ERR_BAD_ARG, "a null array with count > 0");
        for (size_t i = 0; i < count; i++) if (!proofs[i] || (ninputs[i] && !inputs32[i])) throw Error(OTTI_ERR_BAD_ARG, "a null proof, or null inputs with a non-zero count");
        if (n_rejected) *n_rejected = 0;
        if (!count) return OTTI_OK;
        std::vector<VerifyItem> items(count);
        for (size_t i = 0; i < count; i++) items[i] = {inputs32[i], ninputs[i], proofs[i], proof_lens[i]};
        nizk_verify_many(*inst->I, *gens->g, tlabel, tlabel_len, items.data(), count, threads, results);
        size_t bad = 0;
        for (size_t i = 0; i < count; i++) bad += results[i] != OTTI_OK;
        if (n_rejected) *n_rejected = bad;
        if (bad) g_last_error = std::to_string(bad) + " of " + std::to_string(count) + " proofs rejected";
        return OTTI_OK;
    });
}
int32_t otti_nizk_verify_batch(const otti_instance *inst, const otti_gens *gens, const uint8_t *tlabel, size_t tlabel_len, size_t count,
                               const uint8_t *const *inputs32, const size_t *ninputs, const uint8_t *const *proofs, const size_t *proof_lens,
                               uint32_t threads, const uint8_t *seed32, int32_t *results, size_t *n_rejected, otti_verify_batch_info *info) {
    return guarded([&] {
        if (!inst || !gens || !results) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (threads > kVerifyManyMaxThreads) throw Error(OTTI_ERR_BAD_ARG, "more than 16 worker threads");
        if (count && (!inputs32 || !ninputs || !proofs || !proof_lens)) throw Error(OTTI_ERR_BAD_ARG, "a null array with count > 0");
        for (size_t i = 0; i < count; i++) if (!proofs[i] || (ninputs[i] && !inputs32[i])) throw Error(OTTI_ERR_BAD_ARG, "a null proof, or null inputs with a non-zero count");
        if (n_rejected) *n_rejected = 0;
        if (info) memset(info, 0, sizeof *info);
        if (!count) return OTTI_OK;
        std::vector<VerifyItem> items(count);
        for (size_t i = 0; i < count; i++) items[i] = {inputs32[i], ninputs[i], proofs[i], proof_lens[i]};
        nizk_verify_batch(*inst->I, *gens->g, tlabel, tlabel_len, items.data(), count, threads, seed32, results, info);
        size_t bad = 0;
        for (size_t i = 0; i < count; i++) bad += results[i] != OTTI_OK;
        if (n_rejected) *n_rejected = bad;
        if (bad) g_last_error = std::to_string(bad) + " of " + std::to_string(count) + " proofs rejected";
        return OTTI_OK;
    });
}
// Many resident witnesses of ONE instance in one call (device.h nizk_prove_many; the contract: include/otti_spartan.h).  Everything the arguments
// alone say is said before the handles are looked into, the generators' size before a device is asked for, and no output is written before that.
int32_t otti_nizk_prove_many(otti_instance *inst, otti_witness *const *wits, size_t count, otti_gens *gens, const uint8_t *tlabel, size_t tlabel_len,
                             const uint8_t *const *seeds32, uint32_t threads, uint8_t **proofs, size_t *proof_lens, int32_t *results, size_t *n_failed,
                             double *stage_ms, otti_prove_many_info *info) {
    return guarded([&] {
        if (!inst || !gens) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (!proofs || !proof_lens || !results) throw Error(OTTI_ERR_BAD_ARG, "a null output array");
        if (count && !wits) throw Error(OTTI_ERR_BAD_ARG, "a null witness array with count > 0");
        for (size_t i = 0; i < count; i++) if (!wits[i]) throw Error(OTTI_ERR_BAD_ARG, "a null witness handle");
        if (threads > kProveManyMaxThreads) throw Error(OTTI_ERR_BAD_ARG, "more than 16 worker threads");
        if (!count) { if (n_failed) *n_failed = 0; return OTTI_OK; }
        Instance &I = *inst->I; Gens &g = *gens->g;
        {   const size_t ell = ilog2(I.num_vars);
            if (g.num_vars_padded != I.num_vars || g.R != ((size_t)1 << (ell - ell / 2))) throw Error(OTTI_ERR_BAD_ARG, "generators were made for a different instance size"); }
        if (otti_device_count() < 1) throw Error(OTTI_ERR_NO_DEVICE, "no device");
        std::vector<ProveManyItem> items(count);
        for (size_t i = 0; i < count; i++) items[i] = {wits[i]->w.get(), seeds32 ? seeds32[i] : nullptr};
        std::vector<std::vector<uint8_t>> pf(count); std::vector<ProveTimings> tm(count);
        otti_prove_many_info inf{};
        nizk_prove_many(I, g, tlabel, tlabel_len, items.data(), count, threads, pf.data(), results, tm.data(), inf);
        size_t bad = 0;
        for (size_t i = 0; i < count; i++) {
            if (results[i] == OTTI_OK) proofs[i] = to_malloc(pf[i], &proof_lens[i]); else { proofs[i] = nullptr; proof_lens[i] = 0; bad++; }
            if (stage_ms) memcpy(stage_ms + 8 * i, tm[i].ms, sizeof tm[i].ms);
        }
        if (n_failed) *n_failed = bad;
        if (info) *info = inf;
        if (bad) g_last_error = std::to_string(bad) + " of " + std::to_string(count) + " proofs failed";
        return OTTI_OK;
    });
}

// ------------------------------------------------------------------------------------------------ SNARK mode
int32_t otti_snark_gens_new(uint64_t nc, uint64_t nv, uint64_t ni, uint64_t nnz, otti_snark_gens **out) {
    return guarded([&] {
        if (!out) throw Error(OTTI_ERR_BAD_ARG, "null out pointer");
        return adopt(out, snark_gens_new(nc, nv, ni, nnz));
    });
}
void otti_snark_gens_free(otti_snark_gens *p) { delete p; }
int32_t otti_snark_encode(otti_instance *inst, otti_snark_gens *gens, otti_comp_comm **out) {
    return guarded([&] {
        if (!inst || !gens || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        return adopt(out, snark_encode_gpu(*inst->I, *gens->g));
    });
}
int32_t otti_comp_comm_bytes(const otti_comp_comm *comm, uint8_t **out, size_t *len) {
    return guarded([&] { if (!comm || !out || !len) throw Error(OTTI_ERR_BAD_ARG, "null argument"); *out = to_malloc(comm->c->serialize(), len); return OTTI_OK; });
}
int32_t otti_comp_comm_from_bytes(const uint8_t *buf, size_t len, otti_comp_comm **out) {
    return guarded([&] {
        if (!buf || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        return adopt(out, CompComm::parse(buf, len));
    });
}
void otti_comp_comm_free(otti_comp_comm *p) { delete p; }
int32_t otti_comp_comm_attach(otti_comp_comm *comm, otti_instance *inst, otti_snark_gens *gens, uint32_t flags) {
    return guarded([&] {
        if (!comm || !inst || !gens) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (flags & ~(uint32_t)OTTI_ATTACH_VERIFY) throw Error(OTTI_ERR_BAD_ARG, "unknown attach flag");
        snark_attach_gpu(*inst->I, *comm->c, *gens->g, (flags & OTTI_ATTACH_VERIFY) != 0); return OTTI_OK;
    });
}
int32_t otti_comp_comm_dims(const otti_comp_comm *comm, uint64_t *num_cons, uint64_t *num_vars, uint64_t *num_inputs, uint64_t *num_ops, int32_t *has_decommitment) {
    return guarded([&] {
        if (!comm) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        const CompComm &c = *comm->c;
        if (num_cons) *num_cons = c.num_cons;
        if (num_vars) *num_vars = c.num_vars;
        if (num_inputs) *num_inputs = c.num_inputs;
        if (num_ops) *num_ops = c.num_ops;
        if (has_decommitment) *has_decommitment = c.dec ? 1 : 0;
        return OTTI_OK;
    });
}
int32_t otti_snark_gens_points(const otti_snark_gens *gens, int32_t which, uint8_t *out32, size_t cap, size_t *count) {
    return guarded([&] {
        if (!gens || (which != 0 && which != 1)) throw Error(OTTI_ERR_BAD_ARG, "null generators, or a stream other than 0 (gens_r1cs_sat) and 1 (gens_r1cs_eval)");
        const std::vector<Pt> &P = (which ? gens->g->eval : gens->g->sat)->P;
        if (count) *count = P.size();
        if (out32) { if (cap < P.size()) throw Error(OTTI_ERR_BAD_ARG, "room for fewer points than the stream has"); for (size_t i = 0; i < P.size(); i++) pt_encode(out32 + 32 * i, P[i]); }
        return OTTI_OK;
    });
}
int32_t otti_snark_prove(otti_instance *inst, otti_comp_comm *comm, const uint8_t *vars32, size_t nvars, const uint8_t *inputs32, size_t ninputs, otti_snark_gens *gens,
                         const uint8_t *tlabel, size_t tlabel_len, const uint8_t *seed32, uint32_t flags, uint8_t **proof, size_t *proof_len, double *stage_ms) {
    return guarded([&] {
        if (!inst || !comm || !gens || !proof || !proof_len) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (!(flags & OTTI_FLAG_GPU)) throw Error(OTTI_ERR_BAD_ARG, "OTTI_FLAG_GPU is the only proving backend; there is no CPU path");
        if (ninputs != inst->I->num_inputs) throw Error(OTTI_ERR_INVALID_NUM_INPUTS, "wrong number of inputs");
        std::vector<Fr> inputs = scalars_from_bytes(inputs32, ninputs);
        SnarkTimings tm{};
        std::vector<uint8_t> pf = snark_prove_gpu(*inst->I, *comm->c, vars32, nvars, inputs, *gens->g, tlabel, tlabel_len, seed32, &tm);
        return emit_proof(pf, tm, proof, proof_len, stage_ms);
    });
}
int32_t otti_snark_prove_resident(otti_instance *inst, otti_comp_comm *comm, otti_witness *wit, otti_snark_gens *gens, const uint8_t *tlabel, size_t tlabel_len,
                                  const uint8_t *seed32, uint8_t **proof, size_t *proof_len, double *stage_ms) {
    return guarded([&] {
        if (!inst || !comm || !wit || !gens || !proof || !proof_len) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        SnarkTimings tm{};
        std::vector<uint8_t> pf = snark_prove_resident(*inst->I, *comm->c, *wit->w, *gens->g, tlabel, tlabel_len, seed32, &tm);
        return emit_proof(pf, tm, proof, proof_len, stage_ms);
    });
}
int32_t otti_snark_prove_sharded(otti_instance *inst, otti_comp_comm *comm, otti_witness *wit, otti_snark_gens *gens, const uint8_t *tlabel, size_t tlabel_len,
                                 const uint8_t *seed32, uint8_t **proof, size_t *proof_len, double *stage_ms) {
    return guarded([&] {
        if (!inst || !comm || !wit || !gens || !proof || !proof_len) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        need_shard();
        if (!seed32) throw Error(OTTI_ERR_BAD_ARG, "a sharded proof needs an explicit random-tape seed (the same on every rank)");
        SnarkTimings tm{};
        std::vector<uint8_t> pf = snark_prove_resident(*inst->I, *comm->c, *wit->w, *gens->g, tlabel, tlabel_len, seed32, &tm, shard_comm());
        return emit_proof(pf, tm, proof, proof_len, stage_ms);
    });
}
int32_t otti_snark_verify(const otti_comp_comm *comm, const uint8_t *inputs32, size_t ninputs, const otti_snark_gens *gens, const uint8_t *tlabel, size_t tlabel_len,
                          const uint8_t *proof, size_t proof_len) {
    return guarded([&] {
        if (!comm || !gens || !proof) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        std::vector<Fr> inputs = scalars_from_bytes(inputs32, ninputs);
        int rc = snark_verify(*comm->c, inputs, *gens->g, tlabel, tlabel_len, proof, proof_len);
        if (rc) g_last_error = "proof rejected";
        return rc;
    });
}
// Many SNARK proofs of ONE computation commitment in one call (snark.h snark_verify_many; the contract: include/otti_spartan.h).
// Bounds per chunk of kSnarkVerifyManyChunk = 16 proofs.  Host: the parsed proofs and, per proof, the eq tables of the evaluation proof whose
// row sum is out (at most 2 x 2^12 scalars).  HBM, on the calling thread's context, grow-only and kept across calls: 160 bytes per comm_derefs
// point of the chunk, 32 per scalar of every sum of a pass, 128 per (window, split) of a job — 25 MB at 2^20 constraints with 8192 rows — and, once
// per commitment and for its lifetime, 96 bytes per point of comm_ops and comm_mem (1 MB at 2^20).  Threads: `threads` - 1 beside the caller.
int32_t otti_snark_verify_many(const otti_comp_comm *comm, const otti_snark_gens *gens, const uint8_t *tlabel, size_t tlabel_len, size_t count,
                               const uint8_t *const *inputs32, const size_t *ninputs, const uint8_t *const *proofs, const size_t *proof_lens,
                               uint32_t threads, int32_t *results, size_t *n_rejected) {
    return guarded([&] {
        if (!comm || !gens || !results) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (threads > kVerifyManyMaxThreads) throw Error(OTTI_ERR_BAD_ARG, "more than 16 worker threads");
        if (count && (!inputs32 || !ninputs || !proofs || !proof_lens)) throw Error(OTTI_ERR_BAD_ARG, "a null array with count > 0");
        for (size_t i = 0; i < count; i++) if (!proofs[i] || (ninputs[i] && !inputs32[i])) throw Error(OTTI_ERR_BAD_ARG, "a null proof, or null inputs with a non-zero count");
        if (n_rejected) *n_rejected = 0;
        if (!count) return OTTI_OK;
        std::vector<VerifyItem> items(count);
        for (size_t i = 0; i < count; i++) items[i] = {inputs32[i], ninputs[i], proofs[i], proof_lens[i]};
        snark_verify_many(*comm->c, *gens->g, tlabel, tlabel_len, items.data(), count, threads, results);
        size_t bad = 0;
        for (size_t i = 0; i < count; i++) bad += results[i] != OTTI_OK;
        if (n_rejected) *n_rejected = bad;
        if (bad) g_last_error = std::to_string(bad) + " of " + std::to_string(count) + " proofs rejected";
        return OTTI_OK;
    });
}
// The same proofs as one randomised batch (snark.h snark_verify_batch; the contract: include/otti_spartan.h).  Refusals, their order and count == 0
// are otti_snark_verify_many's; the bounds per chunk are its too, plus per collected proof a dense scalar per generator of either handle.
int32_t otti_snark_verify_batch(const otti_comp_comm *comm, const otti_snark_gens *gens, const uint8_t *tlabel, size_t tlabel_len, size_t count,
                                const uint8_t *const *inputs32, const size_t *ninputs, const uint8_t *const *proofs, const size_t *proof_lens,
                                uint32_t threads, const uint8_t *seed32, int32_t *results, size_t *n_rejected, otti_verify_batch_info *info) {
    return guarded([&] {
        if (!comm || !gens || !results) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (threads > kVerifyManyMaxThreads) throw Error(OTTI_ERR_BAD_ARG, "more than 16 worker threads");
        if (count && (!inputs32 || !ninputs || !proofs || !proof_lens)) throw Error(OTTI_ERR_BAD_ARG, "a null array with count > 0");
        for (size_t i = 0; i < count; i++) if (!proofs[i] || (ninputs[i] && !inputs32[i])) throw Error(OTTI_ERR_BAD_ARG, "a null proof, or null inputs with a non-zero count");
        if (n_rejected) *n_rejected = 0;
        if (info) memset(info, 0, sizeof *info);
        if (!count) return OTTI_OK;
        std::vector<VerifyItem> items(count);
        for (size_t i = 0; i < count; i++) items[i] = {inputs32[i], ninputs[i], proofs[i], proof_lens[i]};
        snark_verify_batch(*comm->c, *gens->g, tlabel, tlabel_len, items.data(), count, threads, seed32, results, info);
        size_t bad = 0;
        for (size_t i = 0; i < count; i++) bad += results[i] != OTTI_OK;
        if (n_rejected) *n_rejected = bad;
        if (bad) g_last_error = std::to_string(bad) + " of " + std::to_string(count) + " proofs rejected";
        return OTTI_OK;
    });
}

// ------------------------------------------------------------------------------------------------ zkInterface / synthetic
int32_t otti_zkif_load(const char *c, const char *i, const char *w, otti_r1cs **out) {
    return guarded([&] { if (!c || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument"); *out = zkif_load_impl(c, i, w); return OTTI_OK; });
}
int32_t otti_zkif_load_inputs(const char *i, otti_r1cs **out) {
    return guarded([&] { if (!i || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument"); *out = zkif_load_inputs_impl(i); return OTTI_OK; });
}
int32_t otti_zkif_write(const otti_r1cs *r, const char *c, const char *i, const char *w) {
    return guarded([&] { if (!r || !c || !i || !w) throw Error(OTTI_ERR_BAD_ARG, "null argument"); zkif_write_impl(r, c, i, w); return OTTI_OK; });
}
void otti_r1cs_free(otti_r1cs *r) { if (!r) return; free(r->A); free(r->B); free(r->C); free(r->vars32); free(r->inputs32); free(r); }

// ---- zkInterface files to a ready instance (zkif.h, k_ingest.hip).  Everything the arguments and the files' readability say is said before a
// device is asked for; the outputs are written last, so any error leaves them as they were.
int32_t otti_instance_from_zkif(const char *circuit_path, const char *inputs_path, const char *witness_path, int32_t mode, otti_instance **inst,
                                otti_r1cs **assignment) {
    return guarded([&] {
        if (!circuit_path || !inputs_path || !inst || !assignment) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (mode != OTTI_INGEST_AUTO && mode != OTTI_INGEST_HOST && mode != OTTI_INGEST_DEVICE) throw Error(OTTI_ERR_BAD_ARG, "unknown ingest mode");
        uint64_t circuit_bytes = 0;
        for (const char *path : {circuit_path, inputs_path, witness_path}) {
            if (!path) continue;
            struct stat st;
            if (access(path, R_OK) != 0 || stat(path, &st) != 0 || !S_ISREG(st.st_mode)) throw Error(OTTI_ERR_IO, std::string("cannot read ") + path);
            if (path == circuit_path) circuit_bytes = (uint64_t)st.st_size;
        }
        bool on_device = mode == OTTI_INGEST_DEVICE;
        if (on_device && otti_device_count() < 1) throw Error(OTTI_ERR_NO_DEVICE, "OTTI_INGEST_DEVICE without a device");
        if (mode == OTTI_INGEST_AUTO) {
            // the device, when its runtime is up in this process already (asking brings nothing up) and the file lies between the cut-over and the budget
            double min_mb = kIngestMinMB, max_gb = kIngestGB;
            if (const char *e = getenv("OTTI_INGEST_MIN_MB")) min_mb = atof(e);
            if (const char *e = getenv("OTTI_INGEST_GB")) max_gb = atof(e);
            const double bytes = (double)circuit_bytes;
            on_device = max_gb > 0 && device_runtime_up() && bytes >= min_mb * 1048576.0 && bytes <= max_gb * 1073741824.0;
        }
        std::unique_ptr<Instance> I; otti_r1cs *r = nullptr;
        if (on_device) r = instance_from_zkif_device(circuit_path, inputs_path, witness_path, I);
        else {
            r = zkif_load_impl(circuit_path, inputs_path, witness_path);
            struct Guard { otti_r1cs *r; ~Guard() { if (r) otti_r1cs_free(r); } } guard{r};
            I = instance_new(r->num_cons, r->num_vars, r->num_inputs, r->A, r->nA, r->B, r->nB, r->C, r->nC);
            free(r->A); free(r->B); free(r->C); r->A = r->B = r->C = nullptr;        // the counts stay
            I->circuit_bytes = circuit_bytes;
            guard.r = nullptr;
        }
        *inst = new otti_instance{std::move(I)}; *assignment = r;
        return OTTI_OK;
    });
}
int32_t otti_instance_entries(otti_instance *inst, int32_t which, otti_entry *out, size_t cap, size_t *count) {
    return guarded([&] {
        if (!inst || which < 0 || which > 2 || (!out && !count)) throw Error(OTTI_ERR_BAD_ARG, "null argument, or a matrix other than 0 (A), 1 (B), 2 (C)");
        const Instance &I = *inst->I;
        if (count) *count = I.nnz[which];
        if (!out) return OTTI_OK;
        if (cap < I.nnz[which]) throw Error(OTTI_ERR_BAD_ARG, "room for fewer entries than the matrix has");
        const SparseMat &m = I.mat(which);                     // (a device-made instance downloads its lists here, once)
        const size_t shift = I.num_vars - I.given_vars;
        for (size_t i = 0; i < m.val.size(); i++) {
            out[i].row = m.row[i]; out[i].col = m.col[i] >= I.num_vars ? m.col[i] - shift : m.col[i];
            fr_to_bytes(out[i].val, m.val[i]);
        }
        return OTTI_OK;
    });
}
int32_t otti_instance_ingest_info(const otti_instance *inst, int32_t *on_device, uint64_t *circuit_bytes, uint64_t *hbm_entry_bytes, double ms[4]) {
    return guarded([&] {
        if (!inst) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        const Instance &I = *inst->I;
        if (on_device) *on_device = I.ingested_on_device ? 1 : 0;
        if (circuit_bytes) *circuit_bytes = I.circuit_bytes;
        if (hbm_entry_bytes) {
            *hbm_entry_bytes = 0;
            if (I.ingested_on_device && I.dev) for (int k = 0; k < 3; k++) *hbm_entry_bytes += (uint64_t)I.dev->ent[k].n * 40;
        }
        if (ms) for (int k = 0; k < 4; k++) ms[k] = I.ingest_ms[k];
        return OTTI_OK;
    });
}
int32_t otti_instance_host_lists_info(const otti_instance *inst, int32_t *materialised, uint64_t *host_bytes) {
    return guarded([&] {
        if (!inst) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        const Instance &I = *inst->I;
        const bool have = I.host_lists_materialised();         // (asks, never downloads)
        if (materialised) *materialised = have ? 1 : 0;
        if (host_bytes) {
            *host_bytes = 0;
            if (have) for (int k = 0; k < 3; k++) *host_bytes += (uint64_t)I.M[k].val.size() * 40;
        }
        return OTTI_OK;
    });
}
// ---- row / column / coefficient arrays to a ready instance (device.h instance_from_coo, k_coo_ingest.hip).  Everything the arguments alone say is
// said before a device is asked for, in the witness section's terms (check_wit_source); *out is written last.
int32_t otti_instance_from_coo(uint64_t num_cons, uint64_t num_vars, uint64_t num_inputs, const otti_coo mats[3], int32_t src_on_device, void *stream,
                               otti_instance **out) {
    return guarded([&] {
        if (!mats || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        CooSource src[3];
        for (int k = 0; k < 3; k++) {
            const otti_coo &m = mats[k];
            if (m.index_format < OTTI_IDX_U32 || m.index_format > OTTI_IDX_I64) throw Error(OTTI_ERR_BAD_ARG, "unknown index format");
            // (a host source is staged as it is, so it has to sit on its element's grid as a device source has to)
            check_wit_source(m.val, m.n, m.val_format, m.val_stride_bytes, true);
            if ((!m.row || !m.col) && m.n) throw Error(OTTI_ERR_BAD_ARG, "null index array with a non-zero count");
            const size_t ib = coo_index_bytes(m.index_format);
            if (((uintptr_t)m.row | (uintptr_t)m.col) & (ib - 1)) throw Error(OTTI_ERR_BAD_ARG, "an index array must be aligned to its element");
            if ((uint64_t)m.n >= kCooMaxEntries) throw Error(OTTI_ERR_BAD_ARG, "a matrix with 2^32 entries or more");
            src[k] = CooSource{m.row, m.col, m.val, m.n, m.index_format, m.val_format, m.val_stride_bytes ? m.val_stride_bytes : wit_elem_bytes(m.val_format)};
        }
        // instance_new's limit on the padded dimensions, which are powers of two: said on the given ones
        if (num_cons > ((uint64_t)1 << 30) || num_vars > ((uint64_t)1 << 30) || num_inputs >= ((uint64_t)1 << 30))
            throw Error(OTTI_ERR_BAD_ARG, "instance too large for 32-bit indices");
        if (otti_device_count() < 1) throw Error(OTTI_ERR_NO_DEVICE, "no device: the arrays are ingested on one");
        return adopt(out, instance_from_coo(num_cons, num_vars, num_inputs, src, src_on_device != 0, (hipStream_t)stream));
    });
}
int32_t otti_instance_device_entries(const otti_instance *inst, int32_t which, const void **d_row, const void **d_col, const void **d_val, size_t *n) {
    return guarded([&] {
        if (!inst || which < 0 || which > 2) throw Error(OTTI_ERR_BAD_ARG, "null argument, or a matrix other than 0 (A), 1 (B), 2 (C)");
        const std::shared_ptr<DeviceInstance> d = inst->I->dev;
        const DeviceCoo *e = d && d->ent[which].n ? &d->ent[which] : nullptr;
        if (d_row) *d_row = e ? e->row.p : nullptr;
        if (d_col) *d_col = e ? e->col.p : nullptr;
        if (d_val) *d_val = e ? e->val.p : nullptr;
        if (n) *n = e ? e->n : 0;
        return OTTI_OK;
    });
}
// ---- new coefficients for a live instance (device.h instance_set_values, k_revalue.hip).  Everything the arguments alone say — the counts against
// the instance's included — is said before a device is asked for; a device is asked for only when the call needs one.
int32_t otti_instance_set_values(otti_instance *inst, const otti_coo_values vals[3], int32_t src_on_device, void *stream) {
    return guarded([&] {
        if (!inst || !vals) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        Instance &I = *inst->I;
        ValuesSource src[3];
        for (int k = 0; k < 3; k++) {
            const otti_coo_values &m = vals[k];
            check_wit_source(m.val, m.n, m.val_format, m.val_stride_bytes, true);
            if (m.val && m.n != I.nnz[k]) throw Error(OTTI_ERR_BAD_ARG, "set_values: a matrix's count differs from its number of entries");
            src[k] = ValuesSource{m.val, m.n, m.val_format, m.val_stride_bytes ? m.val_stride_bytes : wit_elem_bytes(m.val_format)};
        }
        if ((src_on_device || instance_values_on_device(I)) && otti_device_count() < 1) throw Error(OTTI_ERR_NO_DEVICE, "no device: the coefficients are replaced on one");
        instance_set_values(I, src, src_on_device != 0, (hipStream_t)stream);
        return OTTI_OK;
    });
}
int32_t otti_instance_values_info(const otti_instance *inst, uint64_t *generation, int32_t *slots_resident, uint64_t *slot_bytes, double ms[3]) {
    return guarded([&] {
        if (!inst) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        const Instance &I = *inst->I;
        const std::shared_ptr<DeviceInstance> d = I.dev;
        const bool slots = d && d->slots_resident;
        if (generation) *generation = I.value_gen;
        if (slots_resident) *slots_resident = slots ? 1 : 0;
        if (slot_bytes) { *slot_bytes = 0; if (slots) for (int k = 0; k < 3; k++) *slot_bytes += (uint64_t)d->ent[k].n * 8; }
        if (ms) for (int k = 0; k < 3; k++) ms[k] = I.values_ms[k];
        return OTTI_OK;
    });
}
int32_t otti_comp_comm_revalue(otti_comp_comm *comm, otti_instance *inst, otti_snark_gens *gens) {
    return guarded([&] {
        if (!comm || !inst || !gens) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        snark_revalue_gpu(*inst->I, *comm->c, *gens->g); return OTTI_OK;
    });
}
// ---- the inputs and witness files to a resident witness (zkif.h, k_wit_ingest.hip).  The ladder of otti_instance_from_zkif: the arguments, the
// files' readability, a missing device — said in every mode: a resident witness lives on one —, then the files; *out and *inputs_out are written last.
static double wit_min_mb() {
    if (const char *e = getenv("OTTI_INGEST_WIT_MIN_MB")) { char *end = nullptr; const double v = strtod(e, &end); if (end != e && v >= 0) return v; }
    return kIngestWitMinMB;
}
double otti_witness_ingest_min_mb(void) { return wit_min_mb(); }
int32_t otti_witness_from_zkif(otti_instance *inst, const char *inputs_path, const char *witness_path, int32_t mode, otti_witness **out, otti_r1cs **inputs_out) {
    return guarded([&] {
        if (!inst || !inputs_path || !witness_path || !out) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        if (mode != OTTI_INGEST_AUTO && mode != OTTI_INGEST_HOST && mode != OTTI_INGEST_DEVICE) throw Error(OTTI_ERR_BAD_ARG, "unknown ingest mode");
        uint64_t witness_bytes = 0;
        for (const char *path : {inputs_path, witness_path}) {
            struct stat st;
            if (access(path, R_OK) != 0 || stat(path, &st) != 0 || !S_ISREG(st.st_mode)) throw Error(OTTI_ERR_IO, std::string("cannot read ") + path);
            if (path == witness_path) witness_bytes = (uint64_t)st.st_size;
        }
        if (otti_device_count() < 1) throw Error(OTTI_ERR_NO_DEVICE, "no device: a resident witness lives on one");
        const Instance &I = *inst->I;
        const bool on_device = mode == OTTI_INGEST_DEVICE || (mode == OTTI_INGEST_AUTO && (double)witness_bytes >= wit_min_mb() * 1048576.0);
        const size_t dims[2] = {I.given_vars, I.num_inputs};
        std::unique_ptr<DeviceWitness> w; std::vector<uint8_t> inputs32;
        const auto t0 = std::chrono::steady_clock::now();
        if (on_device) {
            zkif_witness_with(inputs_path, witness_path, dims, [&](const ZkifWitness &zw) {
                const double walk_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                w = std::make_unique<DeviceWitness>(I, zw);
                w->file_ms[0] = walk_ms;
                inputs32 = zw.inputs32;
            });
        } else {
            otti_r1cs *r = zkif_load_assignment(inputs_path, witness_path, dims);
            struct Guard { otti_r1cs *r; ~Guard() { otti_r1cs_free(r); } } guard{r};
            std::vector<Fr> inputs = scalars_from_bytes(r->inputs32, r->ninputs);
            w = std::make_unique<DeviceWitness>(I, WIT_CANONICAL32, r->vars32, r->nvars, 0, false, nullptr, inputs);
            w->file_bytes = witness_bytes;
            inputs32.assign(r->inputs32, r->inputs32 + 32 * r->ninputs);
        }
        otti_r1cs *io = nullptr;
        if (inputs_out) {                                       // as otti_zkif_load_inputs gives them
            io = (otti_r1cs *)calloc(1, sizeof *io);
            if (!io) throw std::bad_alloc();
            io->num_inputs = io->ninputs = inputs32.size() / 32;
            io->vars32 = (uint8_t *)calloc(1, 1); io->inputs32 = (uint8_t *)calloc(std::max<size_t>(1, inputs32.size()), 1);
            if (!io->vars32 || !io->inputs32) { otti_r1cs_free(io); throw std::bad_alloc(); }
            if (!inputs32.empty()) memcpy(io->inputs32, inputs32.data(), inputs32.size());
        }
        *out = new otti_witness{std::move(w)};
        if (inputs_out) *inputs_out = io;
        return OTTI_OK;
    });
}
int32_t otti_witness_ingest_info(const otti_witness *wit, int32_t *on_device, uint64_t *witness_bytes, double ms[3]) {
    return guarded([&] {
        if (!wit) throw Error(OTTI_ERR_BAD_ARG, "null argument");
        const DeviceWitness &w = *wit->w;
        if (on_device) *on_device = w.from_file_on_device ? 1 : 0;
        if (witness_bytes) *witness_bytes = w.file_bytes;
        if (ms) for (int k = 0; k < 3; k++) ms[k] = w.file_ms[k];
        return OTTI_OK;
    });
}
static int32_t synth_entry(decltype(synth_r1cs) *synth, uint64_t n, uint64_t min_n, uint64_t ni, uint64_t seed, otti_r1cs **out) {
    return guarded([&] {
        if (!out || n < min_n) throw Error(OTTI_ERR_BAD_ARG, "bad argument");
        std::vector<otti_entry> A, B, C; std::vector<uint8_t> vars, inputs;
        synth(n, ni, seed, A, B, C, vars, inputs);
        *out = otti_r1cs_from(n, n, ni, A, B, C, vars, inputs); return OTTI_OK;
    });
}
int32_t otti_synth_r1cs(uint64_t n, uint64_t ni, uint64_t seed, otti_r1cs **out) { return synth_entry(synth_r1cs, n, 1, ni, seed, out); }
int32_t otti_synth_r1cs_compiler_like(uint64_t n, uint64_t ni, uint64_t seed, otti_r1cs **out) { return synth_entry(synth_r1cs_compiler_like, n, 8, ni, seed, out); }

}  // extern "C"
