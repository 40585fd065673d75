// New coefficients for a live instance (otti_instance_set_values): the structure — rows, columns, counts, both CSR copies' ptr / idx, the heavy
// rows and their segments — stays, and only what holds a coefficient is written: ent[k].val, by_row.val / by_col.val, and small[] of both copies
// when the variant reads codes.
//
// Two streaming passes, a thread per entry, no LDS:
//   convert  the caller's element (kernels_common.h wit_load: one 8-byte or two 16-byte loads) through wit_convert to the Montgomery value, stored
//            at the entry's own position of a STAGING list (two 16-byte stores) beside its fr_small_code (4 bytes); the small ones counted per wave
//            and added once per wave (k_coef_codes' reduction); a refused entry's key (coo_walk.h coo_key, kind scalar) offered to one atomicMin
//            word.  Nothing of the instance is touched: the word is read behind the launches, and a defect ends the call there.
//   place    staging[i] (32 bytes, coalesced) to by_row.val[slot_row[i]] and by_col.val[slot_col[i]] (two 32-byte stores each; the by-row slots
//            of a list given row by row are nearly consecutive, the by-column ones scatter), the code likewise when the variant reads codes.  No
//            atomics.  The staging list then BECOMES ent[k].val by a swap of the two buffers.
// The slot maps (device.h DeviceInstance) are what build_csr_set's scatter forgets: where the cursor put entry i.  They are made by the first call
// on an instance: that call runs the scatter again over the unchanged ptr (k_csr_fill plus one store), which rewrites idx / val / small of the copy in
// a new arrival order and records it; every later call places through the maps.  The yardstick of both passes is HBM bandwidth.
#include "kernels_common.h"
#include "coo_walk.h"

namespace otti {

template <int ValF>
__global__ __launch_bounds__(kBlock) void k_values_convert(const unsigned char *val, size_t stride, size_t n, int matrix, Fr *stage, int32_t *code,
                                                           unsigned long long *n_small, unsigned long long *err) {
    const bool wide = (((size_t)val | stride) & 15) == 0;
    unsigned mine = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        bool neg, refused, small;
        const Fr raw = wit_load<ValF>(val + i * stride, wide, neg);
        const Fr v = wit_convert<ValF>(raw, neg, refused, small);
        const int32_t cd = fr_small_code(v);
        stage[i] = v; code[i] = cd; mine += cd != kNotSmall;
        if (refused) atomicMin(err, (unsigned long long)coo_key(matrix, i, COO_KIND_SCALAR));
    }
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor((int)mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_small, (unsigned long long)mine);
}
// the codes of values that are in HBM already (a matrix the call leaves alone, when its count or its codes are wanted): code and n_small may be null
__global__ __launch_bounds__(kBlock) void k_values_codes(const Fr *val, size_t n, int32_t *code, unsigned long long *n_small) {
    unsigned mine = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int32_t cd = fr_small_code(val[i]);
        if (code) code[i] = cd;
        mine += cd != kNotSmall;
    }
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor((int)mine, off, 64);
    if (n_small && (threadIdx.x & 63) == 0 && mine) atomicAdd(n_small, (unsigned long long)mine);
}
__global__ __launch_bounds__(kBlock) void k_values_place(const Fr *stage, const int32_t *code, const uint32_t *slot_row, const uint32_t *slot_col, size_t n,
                                                         Fr *row_val, Fr *col_val, int32_t *row_small, int32_t *col_small) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const Fr v = stage[i];
        const uint32_t pr = slot_row[i], pc = slot_col[i];
        row_val[pr] = v; col_val[pc] = v;
        if (row_small) { const int32_t cd = code[i]; row_small[pr] = cd; col_small[pc] = cd; }
    }
}
// k_csr_fill (k_sparse.hip) plus one store: the position the cursor handed to entry i.  cursor starts as a copy of ptr, which was counted from
// this very list of majors: every position lies inside the copy.
__global__ __launch_bounds__(kBlock) void k_csr_fill_slots(const uint32_t *major, const uint32_t *minor, const Fr *val, const int32_t *code, size_t n, uint32_t *cursor,
                                                           uint32_t *idx, Fr *out, int32_t *out_code, uint32_t *slot) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t p = atomicAdd(&cursor[major[i]], 1u);
        idx[p] = minor[i]; out[p] = val[i]; slot[i] = p;
        if (out_code) out_code[p] = code[i];
    }
}

static void convert_launch(DevCtx &c, int format, const unsigned char *val, size_t stride, size_t n, int matrix, Fr *stage, int32_t *code, unsigned long long *n_small,
                           unsigned long long *err) {
    auto go = [&](auto F) {
        hipLaunchKernelGGL((k_values_convert<decltype(F)::value>), grid_for(n), kBlock, 0, c.stream, val, stride, n, matrix, stage, code, n_small, err);
    };
    switch (format) {
    case WIT_CANONICAL32: return go(std::integral_constant<int, WIT_CANONICAL32>{});
    case WIT_MONTGOMERY32: return go(std::integral_constant<int, WIT_MONTGOMERY32>{});
    case WIT_I64: return go(std::integral_constant<int, WIT_I64>{});
    case WIT_U64: return go(std::integral_constant<int, WIT_U64>{});
    default: throw Error(OTTI_ERR_BAD_ARG, "unknown coefficient format");
    }
}

bool instance_values_on_device(const Instance &I) {
    if (!I.ingested_on_device || !I.dev) return false;
    for (int k = 0; k < 3; k++) if (I.dev->ent[k].n != I.nnz[k]) return false;
    return true;
}

static void wait_for_producer(DevCtx &c, hipStream_t producer) {
    if (!producer || producer == c.stream) return;
    if (!c.ev_order) OTTI_HIP(hipEventCreateWithFlags(&c.ev_order, hipEventDisableTiming));
    OTTI_HIP(hipEventRecord(c.ev_order, producer)); OTTI_HIP(hipStreamWaitEvent(c.stream, c.ev_order, 0));
}

// the plain route with sources in HBM: downloaded as they are, then instance_set_values_host
static void set_values_host_from_device(Instance &I, const ValuesSource vals[3], hipStream_t producer) {
    DevCtx &c = DevCtx::get();
    wait_for_producer(c, producer);
    std::vector<uint8_t> copy[3]; ValuesSource host[3];
    for (int k = 0; k < 3; k++) {
        host[k] = vals[k];
        if (!vals[k].val || !vals[k].n) continue;
        copy[k].resize((vals[k].n - 1) * vals[k].val_stride + wit_elem_bytes(vals[k].val_format));
        OTTI_HIP(hipMemcpyAsync(copy[k].data(), vals[k].val, copy[k].size(), hipMemcpyDeviceToHost, c.stream));
        host[k].val = copy[k].data();
    }
    OTTI_HIP(hipStreamSynchronize(c.stream));
    instance_set_values_host(I, host);
}

void instance_set_values(Instance &I, const ValuesSource vals[3], bool src_on_device, hipStream_t producer) {
    if (!instance_values_on_device(I)) {
        double t0 = ingest_now();
        if (src_on_device) set_values_host_from_device(I, vals, producer); else instance_set_values_host(I, vals);
        I.values_ms[0] = 0; I.values_ms[1] = ingest_now() - t0; I.values_ms[2] = 0;
        return;
    }
    double t0 = ingest_now();
    DevCtx &c = DevCtx::get();
    const std::shared_ptr<DeviceInstance> d = I.dev;
    const bool first = !d->slots_resident;
    bool given[3]; size_t total = 0;
    for (int k = 0; k < 3; k++) { given[k] = vals[k].val != nullptr && vals[k].n != 0; total += d->ent[k].n; }

    // ---- the sources where the kernel reads them, staging and the four words (the error key, three small counts) allocated
    wait_for_producer(c, src_on_device ? producer : nullptr);
    const unsigned char *src[3] = {nullptr, nullptr, nullptr}; DevBuf<uint8_t> staged[3];
    // the staging value list is fresh every call (it becomes the list); the code lists and the four words are the instance's own, kept across calls
    DevBuf<Fr> stage[3]; DevBuf<int32_t> *code = d->values_code; DevBuf<unsigned long long> &words = d->values_words;
    if (!words.p) words.alloc(4);
    for (int k = 0; k < 3; k++) {
        const size_t n = d->ent[k].n;
        if ((given[k] || (first && n)) && code[k].n < n) code[k].alloc(n);
        if (given[k]) stage[k].alloc(n);
        if (!given[k]) continue;
        src[k] = static_cast<const unsigned char *>(vals[k].val);
        if (src_on_device) continue;
        const size_t bytes = (n - 1) * vals[k].val_stride + wit_elem_bytes(vals[k].val_format);
        staged[k].alloc(bytes);
        OTTI_HIP(hipMemcpyAsync(staged[k].p, vals[k].val, bytes, hipMemcpyHostToDevice, c.stream));
        src[k] = staged[k].p;
    }
    OTTI_HIP(hipMemsetAsync(words.p, 0xff, sizeof(unsigned long long), c.stream));
    OTTI_HIP(hipMemsetAsync(words.p + 1, 0, 3 * sizeof(unsigned long long), c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));
    double t1 = ingest_now(); const double ms_staging = t1 - t0; t0 = t1;

    // ---- convert + validate: into staging alone; the words read once behind the launches
    unsigned long long h[4] = {kCooNoError, 0, 0, 0};
    OTTI_HIP(hipEventRecord(c.ev0, c.stream));
    for (int k = 0; k < 3; k++) {
        const size_t n = d->ent[k].n;
        if (given[k]) convert_launch(c, vals[k].val_format, src[k], vals[k].val_stride, n, k, stage[k].p, code[k].p, words.p + 1 + k, words.p);
        else if (first && n) hipLaunchKernelGGL(k_values_codes, grid_for(n), kBlock, 0, c.stream, (const Fr *)d->ent[k].val.p, n, code[k].p, words.p + 1 + k);
    }
    OTTI_HIP(hipEventRecord(c.ev1, c.stream));
    OTTI_HIP(hipMemcpyAsync(h, words.p, sizeof h, hipMemcpyDeviceToHost, c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));                 // the sources are free again
    float ev_convert = 0; OTTI_HIP(hipEventElapsedTime(&ev_convert, c.ev0, c.ev1));
    t1 = ingest_now(); const double ms_convert = t1 - t0; t0 = t1;
    if (h[0] != kCooNoError) throw Error(coo_key_code(h[0]), coo_key_what(h[0]));
    for (auto &b : staged) b.release();

    // ---- the codes rule (classify_coefficients') on the counts of the new lists
    unsigned long long n_small[3], sum_small = 0;
    for (int k = 0; k < 3; k++) { n_small[k] = (given[k] || first) ? h[1 + k] : d->n_small[k]; sum_small += n_small[k]; }
    const bool was_small = d->by_row.use_small, use_small = total >= 1024 && 2 * sum_small >= total;
    // everything the place pass needs is allocated before it writes anything
    DeviceCsrSet *copies[2] = {&d->by_row, &d->by_col};
    DevBuf<int32_t> fresh_small[2][3]; DevBuf<uint32_t> fresh_slot[2][3]; DevBuf<uint32_t> cursor;
    if (use_small && !was_small) for (int s = 0; s < 2; s++) for (int k = 0; k < 3; k++) fresh_small[s][k].alloc(std::max<size_t>(1, d->ent[k].n));
    if (first) {
        for (int s = 0; s < 2; s++) for (int k = 0; k < 3; k++) fresh_slot[s][k].alloc(std::max<size_t>(1, d->ent[k].n));
        cursor.alloc(std::max(d->by_row.rows, d->by_col.rows));
    }
    auto small_of = [&](int s, int k) -> int32_t * { return !use_small ? nullptr : was_small ? copies[s]->small[k].p : fresh_small[s][k].p; };

    // ---- place
    OTTI_HIP(hipEventRecord(c.ev0, c.stream));
    for (int k = 0; k < 3; k++) {
        const DeviceCoo &e = d->ent[k]; const size_t n = e.n;
        if (!n) continue;
        const Fr *val = given[k] ? stage[k].p : e.val.p;
        if (first) {
            for (int s = 0; s < 2; s++) {
                DeviceCsrSet &m = *copies[s];
                const uint32_t *major = s ? e.col.p : e.row.p, *minor = s ? e.row.p : e.col.p;
                OTTI_HIP(hipMemcpyAsync(cursor.p, m.ptr[k].p, m.rows * 4, hipMemcpyDeviceToDevice, c.stream));
                hipLaunchKernelGGL(k_csr_fill_slots, grid_for(n), kBlock, 0, c.stream, major, minor, val, (const int32_t *)code[k].p, n, cursor.p, m.idx[k].p, m.val[k].p,
                                   small_of(s, k), fresh_slot[s][k].p);
            }
        } else if (given[k]) {
            hipLaunchKernelGGL(k_values_place, grid_for(n), kBlock, 0, c.stream, (const Fr *)stage[k].p, (const int32_t *)code[k].p, (const uint32_t *)d->slot_row[k].p,
                               (const uint32_t *)d->slot_col[k].p, n, d->by_row.val[k].p, d->by_col.val[k].p, small_of(0, k), small_of(1, k));
        } else if (use_small && !was_small) {                  // a matrix the call leaves alone, under a variant that reads codes from now on: straight from the copies' values
            for (int s = 0; s < 2; s++)
                hipLaunchKernelGGL(k_values_codes, grid_for(n), kBlock, 0, c.stream, (const Fr *)copies[s]->val[k].p, n, fresh_small[s][k].p, (unsigned long long *)nullptr);
        }
    }
    OTTI_HIP(hipEventRecord(c.ev1, c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));
    float ev_place = 0; OTTI_HIP(hipEventElapsedTime(&ev_place, c.ev0, c.ev1));

    // ---- the instance takes what was made: nothing throws between here and the generation's move
    for (int k = 0; k < 3; k++) {
        if (given[k]) std::swap(d->ent[k].val, stage[k]);      // (the old list goes with this frame)
        d->n_small[k] = n_small[k];
        for (int s = 0; s < 2; s++) {
            if (use_small && !was_small) copies[s]->small[k] = std::move(fresh_small[s][k]);
            if (!use_small && was_small) copies[s]->small[k].release();
        }
        if (first) { d->slot_row[k] = std::move(fresh_slot[0][k]); d->slot_col[k] = std::move(fresh_slot[1][k]); }
    }
    d->by_row.use_small = d->by_col.use_small = use_small;
    d->slots_resident = true;
    d->values_kernel_ms[0] = ev_convert; d->values_kernel_ms[1] = ev_place;
    I.shard.reset();
    I.value_gen++;
    // host lists that a consumer has downloaded are brought along (values only); lists never asked for stay unmade
    if (I.host_lists_pending && I.host_lists_materialised())
        for (int k = 0; k < 3; k++)
            if (given[k]) OTTI_HIP(hipMemcpy(I.M[k].val.data(), d->ent[k].val.p, d->ent[k].n * sizeof(Fr), hipMemcpyDeviceToHost));
    I.values_ms[0] = ms_staging; I.values_ms[1] = ms_convert; I.values_ms[2] = ingest_now() - t0;
}

}  // namespace otti
