// Circuit ingest on the device: the ConstraintSystem messages of a .zkif file go to HBM as they are in the file, and kernels walk the FlatBuffers
// tables there (zkif_walk.h: the same bounds-checked reader the host check program runs under sanitizers), map variable ids to columns, validate
// and convert the coefficients and write the entry lists in file order.  classify_coefficients and build_csr_set (k_sparse.hip) take them from
// there, as they take the lists upload_instance copies from the host.
//
// Three passes.  COUNT: a thread per constraint walks its three combinations: three counts per row.  SCAN: scan_inplace per matrix.  FILL: a thread
// per ENTRY finds its row in the scanned counts (a binary search: no thread holds a row's entries, however many there are), walks to its
// combination again and writes row, col, val at its place.  Every defect met is a key (zkif_walk.h) handed to ONE atomicMin word: the smallest
// names what a sequential host run would have reported (a coefficient >= l is held back until the frame has checked the assignment, as
// instance_new runs behind zkif_load).  Counts and scan are 32-bit; offsets in a file may alias, so the count pass also sums each matrix in 64 bits
// and a matrix of 2^32 entries is refused.  After an error everything allocated here is released and the context stays usable.
#include "kernels_common.h"
#include "zkif.h"
#include <thread>
#include <system_error>
#include <exception>

namespace otti {

// the message that holds row r: the last one that starts at or before it (a message without constraints shares its first row with its successor)
__device__ __forceinline__ ZwMsg ingest_msg_of(const uint8_t *image, const IngestMsg *msgs, uint32_t n_msgs, uint64_t r) {
    uint32_t lo = 0, hi = n_msgs - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (msgs[mid].first_row <= r) lo = mid; else hi = mid - 1; }
    const IngestMsg m = msgs[lo];
    return ZwMsg{image + m.off, m.size, m.vec_start, m.count, m.first_row};
}
// tot[k]: matrix k's entries summed in 64 bits.  The per-row counts are 32-bit and so is the scan; offsets in untrusted bytes may ALIAS (a million
// constraint slots pointing at one table of thousands of ids: 2^33 entries from a few MB), so only this sum says whether the scan can have wrapped.
__global__ __launch_bounds__(kBlock) void k_ingest_count(const uint8_t *image, const IngestMsg *msgs, uint32_t n_msgs, uint64_t rows, uint32_t *cnt,
                                                         unsigned long long *err, unsigned long long *tot) {
    unsigned long long mine[3] = {0, 0, 0};
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * blockDim.x) {
        const ZwMsg m = ingest_msg_of(image, msgs, n_msgs, r);
        uint32_t c3[3] = {0, 0, 0};
        Zw z{m.base, m.size, kZwNoError};
        if (r - m.first_row < m.count) zw_count(z, m, r - m.first_row, c3);
        for (int k = 0; k < 3; k++) { cnt[(uint64_t)k * rows + r] = c3[k]; mine[k] += c3[k]; }
        if (z.err != kZwNoError) atomicMin(err, (unsigned long long)z.err);
    }
    for (int k = 0; k < 3; k++) {                               // (every lane of the wave is here: the loop above has no early exit)
        unsigned long long v = mine[k];
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tot[k], v);
    }
}
// incl: matrix k's counts after the inclusive scan; total = incl[rows - 1] entries, one thread each
__global__ __launch_bounds__(kBlock) void k_ingest_fill(const uint8_t *image, const IngestMsg *msgs, uint32_t n_msgs, uint64_t rows, const uint32_t *incl, int k,
                                                        uint64_t total, const uint32_t *col_of, uint64_t n_ids, uint64_t num_vars, uint64_t pad_shift,
                                                        uint32_t *row_out, uint32_t *col_out, Fr *val_out, unsigned long long *err) {
    for (uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = rows - 1;                         // the first row whose inclusive count exceeds p
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (incl[mid] > p) hi = mid; else lo = mid + 1; }
        const uint64_t r = lo, e = p - (r ? incl[r - 1] : 0u);
        const ZwMsg m = ingest_msg_of(image, msgs, n_msgs, r);
        Zw z{m.base, m.size, kZwNoError};
        uint64_t id = 0; Fr raw = fr_zero(), v = fr_zero(); uint32_t col = 0;
        if (r - m.first_row < m.count && zw_emit(z, m, r - m.first_row, k, e, id, raw.v)) {
            col = zw_col(z, col_of, n_ids, id, num_vars, pad_shift, zw_key_parse(r, k, 1, e, 0));
            if (!fr_raw_is_canonical(raw.v)) z.fail(zw_key_noncanonical(k, p));
            else v = fr_mul(raw, fr_R2());                      // canonical -> Montgomery, as dev_from_canonical
        }
        row_out[p] = (uint32_t)r; col_out[p] = col; val_out[p] = v;
        if (z.err != kZwNoError) atomicMin(err, (unsigned long long)z.err);
    }
}

// ------------------------------------------------------------------------------------------------ getting the bytes there
// Pinned slabs, kept for the life of the process (allocating pinned memory costs more than filling it): at most kIngestThreads host threads fill
// slabs from the mapping, each queueing the copy of a slab it has filled and going on to fill its other one while that copy runs.
constexpr size_t kIngestSlab = (size_t)2 << 20;
constexpr unsigned kIngestThreads = 16;
namespace {
struct SlabPool { std::mutex mu; std::vector<uint8_t *> slab; std::vector<hipEvent_t> ev; };
SlabPool &slab_pool() { static SlabPool *p = new SlabPool(); return *p; }
}  // namespace

// image bytes [a, b) gathered from the messages that overlap them (layout: message j's body at off[j], 16-byte aligned; the gaps are never read)
static void fill_slab(uint8_t *dst, size_t a, size_t b, const std::vector<ZwMsg> &msgs, const std::vector<IngestMsg> &lay) {
    size_t j = (size_t)(std::upper_bound(lay.begin(), lay.end(), a, [](size_t x, const IngestMsg &m) { return x < m.off; }) - lay.begin());
    if (j) j--;
    for (; j < lay.size() && lay[j].off < b; j++) {
        const size_t m0 = (size_t)lay[j].off, m1 = m0 + (size_t)lay[j].size, s = std::max(a, m0), t = std::min(b, m1);
        if (s < t) memcpy(dst + (s - a), msgs[j].base + (s - m0), t - s);
    }
}
void ingest_stage_image(DevCtx &c, uint8_t *d_image, size_t image_bytes, const std::vector<ZwMsg> &msgs, const std::vector<IngestMsg> &lay) {
    const size_t n_slabs = (image_bytes + kIngestSlab - 1) / kIngestSlab;
    if (!n_slabs) return;
    unsigned nt = image_bytes < ((size_t)8 << 20) ? 1u : std::max(1u, std::min(kIngestThreads, std::thread::hardware_concurrency()));
    nt = (unsigned)std::min<size_t>(nt, n_slabs);
    SlabPool &P = slab_pool();
    std::lock_guard<std::mutex> lk(P.mu);                     // one ingest stages at a time
    while (P.slab.size() < 2 * (size_t)nt) {
        uint8_t *p = nullptr; hipEvent_t e = nullptr;
        OTTI_HIP(hipHostMalloc((void **)&p, kIngestSlab, hipHostMallocDefault));
        P.slab.push_back(p);
        OTTI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        P.ev.push_back(e);
    }
    std::vector<std::exception_ptr> err(nt);
    auto work = [&](unsigned w) {
        try {
            OTTI_HIP(hipSetDevice(c.device));
            bool used[2] = {false, false};
            unsigned turn = 0;
            for (size_t t = w; t < n_slabs; t += nt, turn ^= 1u) {
                const size_t q = 2 * (size_t)w + turn, a = t * kIngestSlab, b = std::min(image_bytes, a + kIngestSlab);
                if (used[turn]) OTTI_HIP(hipEventSynchronize(P.ev[q]));          // the copy that last read this slab
                fill_slab(P.slab[q], a, b, msgs, lay);
                OTTI_HIP(hipMemcpyAsync(d_image + a, P.slab[q], b - a, hipMemcpyHostToDevice, c.stream));
                OTTI_HIP(hipEventRecord(P.ev[q], c.stream));
                used[turn] = true;
            }
        } catch (...) { err[w] = std::current_exception(); }
    };
    // (a thread that cannot be started must not unwind through joinable threads: its share runs here instead, as zkif.cpp's fan_out)
    std::vector<std::thread> th; th.reserve(nt);
    unsigned started = 1;
    for (; started < nt; started++) { try { th.emplace_back(work, started); } catch (const std::system_error &) { break; } }
    work(0u);
    for (unsigned w = started; w < nt; w++) work(w);
    for (auto &x : th) x.join();
    hipError_t se = hipStreamSynchronize(c.stream);             // the slabs are the pool's again only once every copy has read them
    for (auto &e : err) if (e) std::rethrow_exception(e);
    OTTI_HIP(se);
}

double ingest_now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Instance::mat() of an instance made here: the entry lists the device copy keeps, as instance_new would have left them on the host
// (the caller hands over local lists and takes them only when all of this has succeeded)
static void host_lists_from_device(const Instance &I, SparseMat out[3]) {
    DevCtx::get();
    const std::shared_ptr<DeviceInstance> d = I.dev;
    if (!d) throw Error(OTTI_ERR_INTERNAL, "instance without host lists and without a device copy");
    for (int k = 0; k < 3; k++) {
        const size_t n = d->ent[k].n;
        out[k].row.resize(n); out[k].col.resize(n); out[k].val.resize(n);
        if (!n) continue;
        OTTI_HIP(hipMemcpy(out[k].row.data(), d->ent[k].row.p, n * 4, hipMemcpyDeviceToHost));
        OTTI_HIP(hipMemcpy(out[k].col.data(), d->ent[k].col.p, n * 4, hipMemcpyDeviceToHost));
        OTTI_HIP(hipMemcpy(out[k].val.data(), d->ent[k].val.p, n * sizeof(Fr), hipMemcpyDeviceToHost));
    }
}

// the device loader's constraint pass (zkif.h): fills I — dimensions, counts, the device copy — from the circuit's messages.  ms[1 .. 3]: staging +
// copies, kernels, CSR build.  A parse error is thrown from here.  A coefficient >= l is RETURNED (true, nothing built): instance_new finds those
// only once zkif_load has finished, so the frame's checks of the assignment, which follow this pass, come first.
static bool ingest_constraints(const ZkifCircuit &zc, Instance &I, double ms[4]) {
    double t0 = ingest_now();
    const size_t nvp = next_pow2(std::max(zc.num_vars, zc.num_inputs + 1)), ncp = zc.rows < 2 ? 2 : next_pow2((size_t)zc.rows);
    // (more rows than an error key can name, or a file beyond the budget of one image: said at once — the host path would say the first after parsing)
    if (ncp > ((size_t)1 << 30)) throw Error(OTTI_ERR_BAD_ARG, "instance too large for 32-bit indices");
    if (zc.file_bytes >= ((size_t)1 << 34)) throw Error(OTTI_ERR_BAD_ARG, "circuit file too large for the device ingest (16 GiB)");
    DevCtx &c = DevCtx::get();
    std::vector<IngestMsg> lay(zc.msgs.size()); size_t image_bytes = 0;
    for (size_t j = 0; j < zc.msgs.size(); j++) {
        const ZwMsg &m = zc.msgs[j];
        lay[j] = IngestMsg{image_bytes, m.size, m.vec_start, m.count, m.first_row};
        image_bytes = (image_bytes + (size_t)m.size + 15) & ~(size_t)15;
    }
    const size_t rows = (size_t)zc.rows;
    DevBuf<uint8_t> d_image(image_bytes + 16);
    DevBuf<IngestMsg> d_msgs(std::max<size_t>(1, lay.size()));
    DevBuf<uint32_t> d_col_of(std::max<size_t>(1, zc.n_ids)), d_cnt(std::max<size_t>(1, 3 * rows));
    DevBuf<unsigned long long> d_err(4);                        // the error key, then the three 64-bit totals
    ingest_stage_image(c, d_image.p, image_bytes, zc.msgs, lay);
    if (!lay.empty()) OTTI_HIP(hipMemcpyAsync(d_msgs.p, lay.data(), lay.size() * sizeof(IngestMsg), hipMemcpyHostToDevice, c.stream));
    if (zc.n_ids) OTTI_HIP(hipMemcpyAsync(d_col_of.p, zc.col_of, zc.n_ids * 4, hipMemcpyHostToDevice, c.stream));
    OTTI_HIP(hipMemsetAsync(d_err.p, 0xff, sizeof(unsigned long long), c.stream));
    OTTI_HIP(hipMemsetAsync(d_err.p + 1, 0, 3 * sizeof(unsigned long long), c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));
    double t1 = ingest_now(); ms[1] = t1 - t0; t0 = t1;

    auto d = std::make_shared<DeviceInstance>();
    DeviceCoo *coo = d->ent;
    unsigned long long err = kZwNoError, head[4] = {kZwNoError, 0, 0, 0}; uint32_t totals[3] = {0, 0, 0};
    auto refuse = [](unsigned long long key) {
        const int code = zw_key_code(key);
        throw Error(code, code == OTTI_ERR_IO ? "zkif: malformed constraint (device ingest)"
                        : code == OTTI_ERR_INVALID_INDEX ? "zkif: constraint references an undeclared variable id" : "zkif: coefficient wider than 32 bytes");
    };
    if (rows) {
        hipLaunchKernelGGL(k_ingest_count, grid_for(rows), kBlock, 0, c.stream, (const uint8_t *)d_image.p, (const IngestMsg *)d_msgs.p, (uint32_t)lay.size(), (uint64_t)rows,
                           d_cnt.p, d_err.p, d_err.p + 1);
        std::vector<DevBuf<uint32_t>> scan_levels; scan_levels.reserve(4);
        for (int k = 0; k < 3; k++) scan_inplace(c, d_cnt.p + (size_t)k * rows, rows, scan_levels);
        for (int k = 0; k < 3; k++) OTTI_HIP(hipMemcpyAsync(&totals[k], d_cnt.p + (size_t)k * rows + rows - 1, 4, hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipMemcpyAsync(head, d_err.p, sizeof head, hipMemcpyDeviceToHost, c.stream));
        OTTI_HIP(hipStreamSynchronize(c.stream));             // (also: the scan's scratch goes out of scope)
        // a matrix of 2^32 entries and more: the scan has wrapped and nothing behind it means anything.  Refused here — behind a malformed table, which the
        // count pass has found whole, and before any entry is looked at (the host path would have to hold the lists first; it has no such limit to name)
        for (int k = 0; k < 3; k++)
            if (head[1 + k] >= ((unsigned long long)1 << 32) || head[1 + k] != totals[k]) {
                if (head[0] != kZwNoError) refuse(head[0]);
                throw Error(OTTI_ERR_BAD_ARG, "a matrix with 2^32 entries or more: too many for the device ingest");
            }
    }
    for (int k = 0; k < 3; k++) {
        const size_t n = totals[k];
        coo[k].n = n; coo[k].row.alloc(std::max<size_t>(1, n)); coo[k].col.alloc(std::max<size_t>(1, n)); coo[k].val.alloc(std::max<size_t>(1, n));
        if (n) hipLaunchKernelGGL(k_ingest_fill, grid_for(n), kBlock, 0, c.stream, (const uint8_t *)d_image.p, (const IngestMsg *)d_msgs.p, (uint32_t)lay.size(), (uint64_t)rows,
                                  (const uint32_t *)(d_cnt.p + (size_t)k * rows), k, (uint64_t)n, (const uint32_t *)d_col_of.p, (uint64_t)zc.n_ids, (uint64_t)zc.num_vars,
                                  (uint64_t)(nvp - zc.num_vars), coo[k].row.p, coo[k].col.p, coo[k].val.p, d_err.p);
    }
    OTTI_HIP(hipMemcpyAsync(&err, d_err.p, sizeof err, hipMemcpyDeviceToHost, c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));
    t1 = ingest_now(); ms[2] = t1 - t0; t0 = t1;
    if (err != kZwNoError && !(err >> 63)) refuse(err);
    if (err != kZwNoError) return true;                       // a coefficient >= l and no parse error: the caller's, behind the frame
    d_image.release(); d_cnt.release(); d_col_of.release(); d_msgs.release();
    finish_device_ingest(c, I, d, IngestDims{ncp, nvp, zc.num_inputs, rows, zc.num_vars}, zc.file_bytes, t0);
    return false;
}
// the tail of every device ingest (device.h): the lists of d->ent, validated and in caller order, to a ready instance
void finish_device_ingest(DevCtx &c, Instance &I, const std::shared_ptr<DeviceInstance> &d, const IngestDims &dims, uint64_t source_bytes, double t0) {
    if (dims.nvp > ((size_t)1 << 30)) throw Error(OTTI_ERR_BAD_ARG, "instance too large for 32-bit indices");
    DeviceCoo *coo = d->ent;
    const bool use_small = classify_coefficients(c, coo);
    build_csr_set(c, d->by_row, coo, false, dims.ncp, use_small);
    build_csr_set(c, d->by_col, coo, true, 2 * dims.nvp, use_small);
    for (int k = 0; k < 3; k++) coo[k].code.release();        // the codes have gone into the CSR copies; row, col, val stay (device.h DeviceInstance::ent)
    d->nnz = coo[0].n + coo[1].n + coo[2].n;
    I.ingest_ms[3] = ingest_now() - t0;
    I.num_cons = dims.ncp; I.num_vars = dims.nvp; I.num_inputs = dims.num_inputs; I.given_cons = dims.given_cons; I.given_vars = dims.given_vars;
    for (int k = 0; k < 3; k++) I.nnz[k] = coo[k].n;
    I.host_lists_pending = true; I.ingested_on_device = true; I.circuit_bytes = source_bytes;
    I.dev = d;
}
static const bool g_host_lists_hook_set = (g_instance_host_lists_hook = host_lists_from_device, true);   // (the pointer itself is constant-initialised: no order to mind)

otti_r1cs *instance_from_zkif_device(const char *circuit_path, const char *inputs_path, const char *witness_path, std::unique_ptr<Instance> &inst) {
    const double t_begin = ingest_now();
    auto I = std::make_unique<Instance>();
    bool non_canonical = false;
    otti_r1cs *r = zkif_load_with(circuit_path, inputs_path, witness_path, [&](const ZkifCircuit &zc, otti_r1cs *out, const ZkifLap &lap) {
        I->ingest_ms[0] = ingest_now() - t_begin;
        non_canonical = ingest_constraints(zc, *I, I->ingest_ms);
        out->nA = I->nnz[0]; out->nB = I->nnz[1]; out->nC = I->nnz[2];
        lap("constraints (device)");
    });
    if (non_canonical) { otti_r1cs_free(r); throw Error(OTTI_ERR_INVALID_SCALAR, "non-canonical scalar in matrix"); }
    inst = std::move(I);
    return r;
}

}  // namespace otti
