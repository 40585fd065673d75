// Launch plan of the fixed-base MSM (k_msm.hip): which kernel a request runs, how its terms are cut into chunks, and where its row sums
// come back.  Pure arithmetic over the request's sizes — standard library only, so a host compiler can run it without HIP
// (tests/msm_plan_check.cpp pins the launches a proof makes and the edges between kernels and routes).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace otti {

enum { MSM_COMPRESSED = 0, MSM_RAW = 1, MSM_KEEP = 2 };     // what a launch's row sums become (device.h dev_msm_rows)
constexpr int kMsmThreads = 256;                             // threads per workgroup of every MSM kernel
constexpr int kSmallChunk = 64;                              // terms per workgroup at most (LDS: 36 B each)
constexpr int kSmallQuads = kMsmThreads / 4;
constexpr size_t kMsmBulkTerms = 4096;                       // bulk launches: terms per workgroup at most, and
constexpr size_t kMsmBulkWorkgroups = 1024;                  // the workgroups they aim for (4 per CU)
constexpr size_t kMsmMailCap = 512;                          // mails per launch (rows * chunks of a fused launch)
constexpr size_t kHostEncodeRows = 8;                        // up to this many row sums are compressed on the host
constexpr size_t kHostPtsCap = 512;                          // extended points the pinned buffer h_pts holds

enum class MsmKernel { bulk, bulk_sparse, small };
// Where the row sums of a launch come back (DevCtx::wait_points acts on it):
enum class MsmRoute {
    mail,            // every workgroup mailed its chunk's sum: the host adds them up into h_pts and compresses
    flag,            // the last workgroup left the row sums in h_pts and raised the host flag: the host compresses
    keep,            // they stay on the device (msm_keep or the caller's keep_dst)
    raw,             // h_pts, extended, behind a stream synchronise
    device_encode,   // compressed on the device: d_points, and h_points behind a stream synchronise
    host_encode,     // h_pts behind a stream synchronise, compressed by the host after it
};
// the recoding constant K = sum_w 2^(c - 1 + c w) over the W windows (288 bits): s' = raw(s) + K carries every window's signed digit
inline void msm_recoding_constant(uint32_t (&K)[9], int c, int W) {
    for (int i = 0; i < 9; i++) K[i] = 0;
    for (int w = 0; w < W; w++) { int bit = c - 1 + c * w; K[bit >> 5] |= 1u << (bit & 31); }
}

struct MsmShape {
    int c, W;                                                // window width and count of the table
    size_t rows, n_dense, n_extra;
    bool bullet;                                             // a bullet-reduction round (scalars derived in the kernel)
    int mode; bool addend, sparse, force_bulk;
    bool host_sum;                                           // this process's small launches are summed on the host (MsmMailbox::host_sum)
    // The workgroups a bulk launch aims for.  Every prover call site leaves the default.  ONLY the kernel-level test entry otti_k_msm_job sets
    // another value (the MSM's counterpart of sc_caps_override): with 1, one workgroup takes min(n_dense, kMsmBulkTerms) terms, so one row of
    // 2048 terms walks the sub-chunks of k_msm_rows that otherwise need an instance of 2^22 constraints.
    size_t bulk_workgroups = kMsmBulkWorkgroups;
};
struct MsmPlan { MsmKernel kernel; size_t chunk, nchunks; int fuse; MsmRoute route; uint32_t K[9]; };

inline MsmPlan msm_plan(const MsmShape &q) {
    const size_t rows = q.rows, n_dense = q.n_dense, lanes = (size_t)(kMsmThreads / q.W);
    const bool bulk = (rows * n_dense >= ((size_t)1 << 16) || (q.force_bulk && n_dense)) && !q.bullet;
    const bool sparse = bulk && q.sparse && q.W <= 32;
    size_t nchunks;
    if (bulk) {
        // aim for >= bulk_workgroups workgroups (1024, 4 per CU, unless a test says otherwise) but keep at least one term per term lane and at most kMsmMaxChunk per workgroup;
        // the sparse variant keeps a (term, window) work list in LDS: (chunk + extras) * W <= kMsmListCap;  W <= 32 there (5-bit window field)
        nchunks = std::max<size_t>(1, (std::max<size_t>(1, q.bulk_workgroups) + rows - 1) / rows);
        nchunks = std::min(nchunks, std::max<size_t>(1, n_dense / lanes));
        const size_t max_chunk = kMsmBulkTerms;               // both bulk kernels walk their chunk in sub-chunks that fit the LDS
        nchunks = std::max(nchunks, (n_dense + max_chunk - 1) / max_chunk);
    } else {
        // latency-bound launches: about two (term, window) pairs per quad (one or two rows) or four (many rows), at most 2048 workgroups
        // and, when the last workgroup sums the chunk results itself (rows <= 2), at most 256 of them per row
        // (whole steps: a workgroup's pairs, extras included, should fill its 64 quads k times — the bullet rounds carry one extra
        // term per workgroup, the slice of c_L / c_R, and two in chunk 0)
        const size_t steps = rows <= 2 ? 3 : 4, per_wg = steps * (size_t)kSmallQuads / (size_t)q.W, ex_wg = q.bullet ? 2 : q.n_extra;
        const size_t terms_wg = per_wg > ex_wg ? per_wg - ex_wg : 1;
        nchunks = std::max<size_t>(1, (n_dense + terms_wg - 1) / terms_wg);
        nchunks = std::min(nchunks, rows <= 2 ? (size_t)256 : std::max<size_t>(1, 2048 / rows));
        nchunks = std::min(nchunks, std::max<size_t>(1, n_dense));
        nchunks = std::max(nchunks, (n_dense + kSmallChunk - 1) / (size_t)kSmallChunk);
    }
    if (!n_dense) nchunks = 1;
    size_t chunk = n_dense ? (n_dense + nchunks - 1) / nchunks : 1;
    nchunks = n_dense ? (n_dense + chunk - 1) / chunk : 1;
    MsmPlan p;
    p.kernel = sparse ? MsmKernel::bulk_sparse : bulk ? MsmKernel::bulk : MsmKernel::small;
    p.chunk = chunk; p.nchunks = nchunks;
    p.fuse = (!bulk && q.mode == MSM_COMPRESSED && !q.addend && rows <= 2 && rows * nchunks <= kMsmMailCap) ? 1 : 0;
    if (p.fuse && q.host_sum) p.fuse = 2;
    if (p.fuse) p.route = p.fuse == 2 ? MsmRoute::mail : MsmRoute::flag;
    else if (q.mode == MSM_KEEP) p.route = MsmRoute::keep;     // (a launch that is not MSM_COMPRESSED never fuses or mails)
    else if (q.mode == MSM_RAW) p.route = MsmRoute::raw;
    else if (rows > kHostEncodeRows || q.addend) p.route = MsmRoute::device_encode;
    // a handful of points: the dependent inverse-square-root chain runs ~30x faster on a host core than on one GPU lane
    else p.route = MsmRoute::host_encode;
    msm_recoding_constant(p.K, q.c, q.W);
    return p;
}

// What dev_msm_rows / dev_bullet_round hand back: DevCtx::wait_points(ticket) returns once the launch's row sums are where the route says
// (the compressed ones in h_points).  seq: the number the mails or the flag will carry; 0 when the results come behind the stream.
struct MsmTicket {
    unsigned long long seq = 0; uint32_t rows = 0; MsmRoute route = MsmRoute::keep;
    bool delivers_without_sync() const { return route == MsmRoute::mail || route == MsmRoute::flag; }   // nothing behind it on the stream has to drain first
    bool points_on_device() const { return route == MsmRoute::device_encode; }                            // the compressed points are in d_points (else: h_points after the wait)
};

}  // namespace otti
