// Witness ingest on the device: the Witness messages of a .wit.zkif go to HBM as they are in the file — through the pinned slabs of the circuit
// ingest (k_ingest.hip ingest_stage_image) — and ONE launch, a thread per assigned variable over all messages, reads id and value through the
// bounds-checked reader (zkif_wit_walk.h: the functions tests/zkif_wit_walk_check.cpp runs on the host under sanitizers), maps the id to its
// column, marks the column in a bitmap (a bit found set: assigned twice), judges and converts the value by THE conversion rule (kernels_common.h
// wit_convert, as k_witness_ingest_from applies it to format-32 sources; the small ones are tallied the same way) and writes z[col].  Every defect is
// a key handed to one atomicMin word that starts at the host walk's own (zkif.h ZkifWitness::seed): the smallest names what the host pair reports.
// The kernel moves the file once and z once; like the circuit kernels it is far from being the bottleneck of an ingest and is left plain.
#include "kernels_common.h"
#include "zkif.h"

namespace otti {

// IngestMsg's five words for a Witness message: vec_start = the ids, count, first_row = its first element's place in the concatenated list; the
// values' start, width and stride ride in a second array
struct WitMsgVals { unsigned long long vals_start, width, stride; };

__global__ __launch_bounds__(kBlock) void k_wit_ingest(const uint8_t *image, const IngestMsg *msgs, const WitMsgVals *vals, uint32_t n_msgs, uint64_t total,
                                                       const uint64_t *inst_sorted, uint64_t ni, uint64_t num_vars, Fr *z, unsigned int *seen,
                                                       unsigned long long *err, unsigned long long *counts) {
    unsigned nsmall = 0;
    for (uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_msgs - 1;                       // the message that holds element p: the last one that starts at or before it
        while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (msgs[mid].first_row <= p) lo = mid; else hi = mid - 1; }
        const IngestMsg m = msgs[lo];
        const WitMsgVals mv = vals[lo];
        const WwMsg w{image + m.off, m.size, m.vec_start, mv.vals_start, m.count, mv.width, mv.stride, m.first_row};
        Zw zz{w.base, w.size, kZwNoError};
        uint64_t id = 0; Fr raw = fr_zero();
        if (p - w.first < w.count) {                            // (always: the messages' counts add up to total)
            ww_elem(zz, w, lo, p - w.first, id, raw.v);
            const uint32_t col = ww_col(zz, inst_sorted, ni, id, num_vars, ww_key(WW_INDEX, p));
            bool refused, small; const Fr v = wit_convert<WIT_CANONICAL32>(raw, false, refused, small);
            if (refused) zz.fail(ww_key(WW_SCALAR, 1 + p));
            if (col != 0xffffffffu) {                           // col < num_vars: within z's first half and within the bitmap
                const unsigned int bit = 1u << (col & 31);
                if (atomicOr(&seen[col >> 5], bit) & bit) zz.fail(ww_key(WW_TWICE, 0));
                else { z[col] = v; nsmall += small; }
            }
        }
        if (zz.err != kZwNoError) atomicMin(err, (unsigned long long)zz.err);
    }
    wit_tally(0u, nsmall, counts);                              // (every lane of the wave is here: the loop above has no early exit)
}

static double wit_now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

uint64_t dev_witness_from_zkif(DevCtx &c, const ZkifWitness &zw, Fr *z, size_t *n_small, double ms[3]) {
    double t0 = wit_now();
    *n_small = 0;
    if (!zw.total) { OTTI_HIP(hipStreamSynchronize(c.stream)); return zw.seed; }     // (the caller's queued copies are done, as behind a launch)
    std::vector<ZwMsg> bodies(zw.msgs.size()); std::vector<IngestMsg> lay(zw.msgs.size()); std::vector<WitMsgVals> vals(zw.msgs.size());
    size_t image_bytes = 0;
    for (size_t j = 0; j < zw.msgs.size(); j++) {
        const WwMsg &m = zw.msgs[j];
        bodies[j] = ZwMsg{m.base, m.size, m.ids_start, m.count, m.first};
        lay[j] = IngestMsg{image_bytes, m.size, m.ids_start, m.count, m.first};
        vals[j] = WitMsgVals{m.vals_start, m.width, m.stride};
        image_bytes = (image_bytes + (size_t)m.size + 15) & ~(size_t)15;
    }
    const size_t ni = zw.inst_sorted.size(), words = (zw.num_vars + 31) / 32;
    DevBuf<uint8_t> d_image(image_bytes + 16);
    DevBuf<IngestMsg> d_msgs(lay.size());
    DevBuf<WitMsgVals> d_vals(vals.size());
    DevBuf<uint64_t> d_inst(std::max<size_t>(1, ni));
    DevBuf<unsigned int> d_seen(std::max<size_t>(1, words));
    DevBuf<unsigned long long> d_err(1);
    ingest_stage_image(c, d_image.p, image_bytes, bodies, lay);
    OTTI_HIP(hipMemcpyAsync(d_msgs.p, lay.data(), lay.size() * sizeof(IngestMsg), hipMemcpyHostToDevice, c.stream));
    OTTI_HIP(hipMemcpyAsync(d_vals.p, vals.data(), vals.size() * sizeof(WitMsgVals), hipMemcpyHostToDevice, c.stream));
    if (ni) OTTI_HIP(hipMemcpyAsync(d_inst.p, zw.inst_sorted.data(), ni * sizeof(uint64_t), hipMemcpyHostToDevice, c.stream));
    OTTI_HIP(hipMemsetAsync(d_seen.p, 0, std::max<size_t>(1, words) * sizeof(unsigned int), c.stream));
    const unsigned long long seed = zw.seed;
    OTTI_HIP(hipMemcpyAsync(d_err.p, &seed, sizeof seed, hipMemcpyHostToDevice, c.stream));
    OTTI_HIP(hipStreamSynchronize(c.stream));
    double t1 = wit_now(); ms[1] = t1 - t0; t0 = t1;
    unsigned long long err = kZwNoError;
    const Tallies t = counted_launch(c, [&](unsigned long long *counts) {
        KScope ks(c, KC_OTHER);
        hipLaunchKernelGGL(k_wit_ingest, grid_for((size_t)zw.total), kBlock, 0, c.stream, (const uint8_t *)d_image.p, (const IngestMsg *)d_msgs.p, (const WitMsgVals *)d_vals.p,
                           (uint32_t)lay.size(), (uint64_t)zw.total, (const uint64_t *)d_inst.p, (uint64_t)ni, (uint64_t)zw.num_vars, z, d_seen.p, d_err.p, counts);
        OTTI_HIP(hipMemcpyAsync(&err, d_err.p, sizeof err, hipMemcpyDeviceToHost, c.stream));
    });
    ms[2] = wit_now() - t0;
    *n_small = (size_t)t.second;
    return err;
}

}  // namespace otti
