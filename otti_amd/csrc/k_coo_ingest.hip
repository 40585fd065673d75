// An instance from row / column / coefficient arrays (otti_instance_from_coo): one streaming pass per matrix turns the caller's arrays, in HBM already
// or staged there as they are, into the entry lists classify_coefficients and build_csr_set take (device.h DeviceCoo) — the lists instance_new
// would have left on the host for the same triples, in the same order.
//
// One thread per entry, no LDS, no cross-lane work: two index loads (4 or 8 bytes a lane, packed: coalesced), the coefficient as one 8-byte or two
// 16-byte loads (four 8-byte ones when base or stride is off the 16-byte grid: kernels_common.h wit_load), the rule of coo_walk.h and
// wit_convert, and 40 bytes written at the entry's own position (4 + 4 + two 16-byte stores).  The yardstick is HBM bandwidth.  A refused entry
// writes nothing and offers its key to ONE atomicMin word, which is read once behind the three launches: the smallest key names what
// instance_new's sequential walk would have reported.
#include "kernels_common.h"
#include "coo_walk.h"

namespace otti {

static_assert(kCooErrInvalidScalar == OTTI_ERR_INVALID_SCALAR && kCooErrInvalidIndex == OTTI_ERR_INVALID_INDEX, "coo_walk.h restates the C ABI's codes");
static_assert(COO_IDX_U32 == OTTI_IDX_U32 && COO_IDX_I32 == OTTI_IDX_I32 && COO_IDX_U64 == OTTI_IDX_U64 && COO_IDX_I64 == OTTI_IDX_I64, "coo_walk.h restates the C ABI's index formats");

template <int IdxF, int ValF>
__global__ __launch_bounds__(kBlock) void k_coo_ingest(const void *row, const void *col, const unsigned char *val, size_t stride, size_t n, int matrix, CooDims dims,
                                                       uint32_t *row_out, uint32_t *col_out, Fr *val_out, unsigned long long *err) {
    const bool wide = (((size_t)val | stride) & 15) == 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        bool row_neg, col_neg, neg, refused, small;
        const uint64_t r = coo_load_index<IdxF>(row, i, row_neg), c = coo_load_index<IdxF>(col, i, col_neg);
        const Fr raw = wit_load<ValF>(val + i * stride, wide, neg);
        const Fr v = wit_convert<ValF>(raw, neg, refused, small);
        uint32_t r32 = 0, c32 = 0;
        const int kind = coo_place(dims, r, row_neg, c, col_neg, refused, r32, c32);
        if (kind == COO_PLACED) { row_out[i] = r32; col_out[i] = c32; val_out[i] = v; }
        else atomicMin(err, (unsigned long long)coo_key(matrix, i, kind));
    }
}

// the two runtime formats -> the kernel's template arguments
template <int IdxF> static void coo_launch_val(DevCtx &c, const CooSource &s, int matrix, const CooDims &dims, DeviceCoo &out, unsigned long long *err) {
    const unsigned char *val = static_cast<const unsigned char *>(s.val);
    auto go = [&](auto F) {
        hipLaunchKernelGGL((k_coo_ingest<IdxF, decltype(F)::value>), grid_for(s.n), kBlock, 0, c.stream, s.row, s.col, val, s.val_stride, s.n, matrix, dims,
                           out.row.p, out.col.p, out.val.p, err);
    };
    switch (s.val_format) {
    case WIT_CANONICAL32: return go(std::integral_constant<int, WIT_CANONICAL32>{});
    case WIT_MONTGOMERY32: return go(std::integral_constant<int, WIT_MONTGOMERY32>{});
    case WIT_I64: return go(std::integral_constant<int, WIT_I64>{});
    case WIT_U64: return go(std::integral_constant<int, WIT_U64>{});
    default: throw Error(OTTI_ERR_BAD_ARG, "unknown coefficient format");
    }
}
static void coo_launch(DevCtx &c, const CooSource &s, int matrix, const CooDims &dims, DeviceCoo &out, unsigned long long *err) {
    switch (s.index_format) {
    case COO_IDX_U32: return coo_launch_val<COO_IDX_U32>(c, s, matrix, dims, out, err);
    case COO_IDX_I32: return coo_launch_val<COO_IDX_I32>(c, s, matrix, dims, out, err);
    case COO_IDX_U64: return coo_launch_val<COO_IDX_U64>(c, s, matrix, dims, out, err);
    case COO_IDX_I64: return coo_launch_val<COO_IDX_I64>(c, s, matrix, dims, out, err);
    default: throw Error(OTTI_ERR_BAD_ARG, "unknown index format");
    }
}

std::unique_ptr<Instance> instance_from_coo(size_t num_cons, size_t num_vars, size_t num_inputs, const CooSource mats[3], bool src_on_device, hipStream_t producer) {
    double t0 = ingest_now();
    const size_t nvp = next_pow2(std::max(num_vars, num_inputs + 1)), ncp = num_cons < 2 ? 2 : next_pow2(num_cons);
    if (ncp > ((size_t)1 << 30) || nvp > ((size_t)1 << 30)) throw Error(OTTI_ERR_BAD_ARG, "instance too large for 32-bit indices");
    for (int k = 0; k < 3; k++) if (mats[k].n >= kCooMaxEntries) throw Error(OTTI_ERR_BAD_ARG, "a matrix with 2^32 entries or more");
    DevCtx &c = DevCtx::get();
    auto I = std::make_unique<Instance>();

    // ---- the sources where the kernel reads them: device arrays as they are, behind the producer's queued work; host arrays staged as they are
    CooSource src[3]; DevBuf<uint8_t> staged[3][3]; uint64_t source_bytes = 0;
    if (src_on_device && producer && producer != c.stream) {
        if (!c.ev_order) OTTI_HIP(hipEventCreateWithFlags(&c.ev_order, hipEventDisableTiming));
        OTTI_HIP(hipEventRecord(c.ev_order, producer)); OTTI_HIP(hipStreamWaitEvent(c.stream, c.ev_order, 0));
    }
    for (int k = 0; k < 3; k++) {
        src[k] = mats[k];
        const size_t n = src[k].n, ib = coo_index_bytes(src[k].index_format), eb = wit_elem_bytes(src[k].val_format);
        source_bytes += (uint64_t)n * (2 * ib + eb);
        if (!n || src_on_device) continue;
        const size_t bytes[3] = {n * ib, n * ib, (n - 1) * src[k].val_stride + eb};
        const void *from[3] = {mats[k].row, mats[k].col, mats[k].val}; const void **to[3] = {&src[k].row, &src[k].col, &src[k].val};
        for (int a = 0; a < 3; a++) {
            staged[k][a].alloc(bytes[a]);
            OTTI_HIP(hipMemcpyAsync(staged[k][a].p, from[a], bytes[a], hipMemcpyHostToDevice, c.stream));
            *to[a] = staged[k][a].p;
        }
    }
    unsigned long long *d_err = c.d_counts.p, err = kCooNoError;   // the context's first tally word serves as the error word: no allocation per call
    OTTI_HIP(hipMemsetAsync(d_err, 0xff, sizeof(unsigned long long), c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));
    double t1 = ingest_now(); I->ingest_ms[1] = t1 - t0; t0 = t1;

    // ---- one launch per matrix, the error word read once behind them
    auto d = std::make_shared<DeviceInstance>();
    const CooDims dims = coo_dims(num_cons, num_vars, num_inputs, nvp);
    for (int k = 0; k < 3; k++) {
        DeviceCoo &out = d->ent[k];
        const size_t n = src[k].n;
        out.n = n; out.row.alloc(std::max<size_t>(1, n)); out.col.alloc(std::max<size_t>(1, n)); out.val.alloc(std::max<size_t>(1, n));
        if (n) coo_launch(c, src[k], k, dims, out, d_err);
    }
    OTTI_HIP(hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));                 // the sources are free again
    t1 = ingest_now(); I->ingest_ms[2] = t1 - t0; t0 = t1;
    if (err != kCooNoError) throw Error(coo_key_code(err), coo_key_what(err));
    for (auto &m : staged) for (auto &b : m) b.release();
    finish_device_ingest(c, *I, d, IngestDims{ncp, nvp, num_inputs, num_cons, num_vars}, source_bytes, t0);
    return I;
}

}  // namespace otti
