// The fixed-base MSM's launch plan (otti_amd/csrc/msm_plan.h) on the host: the launches a proof makes and the edges between kernels and
// result routes, as values of the launcher's arithmetic.  The plan sets the grid of the dominant kernel; nothing here needs a GPU.
// Built and run by tests/test_msm_plan_host.py (plain g++, standard library only).
#include "msm_plan.h"
#include <cstdio>

using namespace otti;

struct Case {
    int c; size_t rows, n_dense, n_extra; int mode; bool addend, sparse, force_bulk, bullet, host_sum;     // the request
    MsmKernel kernel; size_t chunk, nchunks; int fuse; MsmRoute route;                                     // what the plan must say
};
static const char *kKernel[] = {"bulk", "bulk-sparse", "small"};
static const char *kRoute[] = {"mail", "flag", "keep", "raw", "device-encode", "host-encode"};
constexpr MsmKernel BULK = MsmKernel::bulk, SPARSE = MsmKernel::bulk_sparse, SMALL = MsmKernel::small;
constexpr int CMP = MSM_COMPRESSED, RAW = MSM_RAW, KEEP = MSM_KEEP;
constexpr bool T = true, F = false;

static const Case kCases[] = {
    //c  rows  n_dense n_ex mode  add spa fb  bul hs    kernel  chunk nchunks fuse route
    {17, 1024, 1024,  0, KEEP, F, F, F, F, F,  BULK,   1024,   1, 0, MsmRoute::keep},             // the witness commitment at 2^20
    {17, 1024, 1024,  0, KEEP, F, T, F, F, F,  SPARSE, 1024,   1, 0, MsmRoute::keep},             // ... of mostly small scalars
    { 7, 1024, 1024,  0, KEEP, F, T, F, F, F,  BULK,   1024,   1, 0, MsmRoute::keep},             // W = 37 > 32: no work list
    {17, 4096, 4096,  0, KEEP, F, F, F, F, F,  BULK,   4096,   1, 0, MsmRoute::keep},             // a whole row of 4096 terms per workgroup
    {16,  512, 8192,  0, CMP,  F, F, F, F, F,  BULK,   4096,   2, 0, MsmRoute::device_encode},    // ... and no more than that
    { 8,  256,  256,  0, KEEP, F, F, F, F, F,  BULK,     64,   4, 0, MsmRoute::keep},             // 2^16 terms: the first bulk launch
    { 8,   64,   64,  0, KEEP, F, F, F, F, F,  SMALL,     8,   8, 0, MsmRoute::keep},
    { 8,    3,   64,  0, KEEP, F, F, T, F, F,  BULK,      8,   8, 0, MsmRoute::keep},             // a run of re-summed rows
    { 8,    2,   64,  0, KEEP, F, F, F, F, F,  SMALL,     6,  11, 0, MsmRoute::keep},
    {17, 1024,    0,  1, CMP,  T, F, F, F, F,  SMALL,     1,   1, 0, MsmRoute::device_encode},    // the blinds onto the kept row sums
    {17,  164,    0,  6, RAW,  F, F, F, F, F,  SMALL,     1,   1, 0, MsmRoute::raw},              // the sum-checks' round points
    {17,    1, 1024,  0, RAW,  F, F, F, F, F,  SMALL,    12,  86, 0, MsmRoute::raw},              // a verifier's row: RAW never fuses
    {17,    1, 1024,  1, CMP,  F, F, F, F, T,  SMALL,    11,  94, 2, MsmRoute::mail},             // Cx, delta
    {17,    1, 1024,  1, CMP,  F, F, F, F, F,  SMALL,    11,  94, 1, MsmRoute::flag},
    {17,    2,  512,  2, CMP,  F, F, F, T, T,  SMALL,    10,  52, 2, MsmRoute::mail},             // a bullet round at R = 1024
    { 8,    2,    2,  2, CMP,  F, F, F, T, T,  SMALL,     2,   1, 2, MsmRoute::mail},
    { 8,    1,    4,  1, CMP,  F, F, F, F, T,  SMALL,     4,   1, 2, MsmRoute::mail},
    { 8,    1,   16,  1, CMP,  F, F, F, F, T,  SMALL,     4,   4, 2, MsmRoute::mail},
    { 8,    2,   16,  1, CMP,  F, F, F, F, T,  SMALL,     4,   4, 2, MsmRoute::mail},
    { 8,    3,   16,  1, CMP,  F, F, F, F, T,  SMALL,     6,   3, 0, MsmRoute::host_encode},      // three rows: no longer fused
    { 8,    8,   16,  1, CMP,  F, F, F, F, T,  SMALL,     6,   3, 0, MsmRoute::host_encode},
    { 8,    9,   16,  1, CMP,  F, F, F, F, T,  SMALL,     6,   3, 0, MsmRoute::device_encode},    // past kHostEncodeRows
    { 4,    2, 32767, 1, CMP,  F, F, F, F, T,  SMALL,    64, 512, 0, MsmRoute::host_encode},      // 1024 mails > kMsmMailCap: not fused
};

// The tests' seam (MsmShape::bulk_workgroups, set only by otti_k_msm_job): aiming for ONE workgroup, a row of 2048 terms is one chunk, which the
// bulk kernels walk in sub-chunks — the walk a default plan reaches only from 2^22 constraints up (the {17, 4096, 4096} case above).
struct SeamCase { int c; size_t rows, n_dense, n_extra; bool sparse; size_t aim; MsmKernel kernel; size_t chunk, nchunks; };
static const SeamCase kSeamCases[] = {
    { 8, 1, 2048, 0, F, 1,    BULK,   2048, 1},
    { 8, 3, 2048, 8, F, 1,    BULK,   2048, 1},
    { 8, 1, 2048, 0, T, 1,    SPARSE, 2048, 1},
    {13, 3, 2048, 1, T, 1,    SPARSE, 2048, 1},
    { 4, 3, 2048, 0, T, 1,    BULK,   2048, 1},                                                   // W = 64: no work list
    { 8, 1, 4097, 0, F, 1,    BULK,   2049, 2},                                                   // never more than kMsmBulkTerms per workgroup
    { 8, 3, 2048, 0, F, 1024, BULK,      8, 256},                                                // the default aim, spelled out: as without the member
};

int main() {
    int failures = 0;
    for (const SeamCase &k : kSeamCases) {
        const int W = 253 / k.c + 1;
        const MsmPlan p = msm_plan({k.c, W, k.rows, k.n_dense, k.n_extra, false, MSM_COMPRESSED, false, k.sparse, true, true, k.aim});
        const MsmPlan d = msm_plan({k.c, W, k.rows, k.n_dense, k.n_extra, false, MSM_COMPRESSED, false, k.sparse, true, true});
        if (p.kernel != k.kernel || p.chunk != k.chunk || p.nchunks != k.nchunks || p.fuse != 0) {
            failures++;
            printf("FAIL seam c=%d rows=%zu n_dense=%zu aim=%zu: plan %s chunk %zu x %zu fuse %d, expected %s chunk %zu x %zu\n", k.c, k.rows, k.n_dense, k.aim,
                   kKernel[(int)p.kernel], p.chunk, p.nchunks, p.fuse, kKernel[(int)k.kernel], k.chunk, k.nchunks);
        }
        if (k.aim == kMsmBulkWorkgroups && (d.chunk != p.chunk || d.nchunks != p.nchunks || d.kernel != p.kernel)) { failures++; printf("FAIL the default aim is not kMsmBulkWorkgroups\n"); }
    }
    for (const Case &k : kCases) {
        const int W = 253 / k.c + 1;
        const MsmPlan p = msm_plan({k.c, W, k.rows, k.n_dense, k.n_extra, k.bullet, k.mode, k.addend, k.sparse, k.force_bulk, k.host_sum});
        const bool ok = p.kernel == k.kernel && p.chunk == k.chunk && p.nchunks == k.nchunks && p.fuse == k.fuse && p.route == k.route;
        if (!ok) {
            failures++;
            printf("FAIL c=%d rows=%zu n_dense=%zu n_extra=%zu mode=%d: plan %s chunk %zu x %zu fuse %d %s, expected %s chunk %zu x %zu fuse %d %s\n", k.c, k.rows,
                   k.n_dense, k.n_extra, k.mode, kKernel[(int)p.kernel], p.chunk, p.nchunks, p.fuse, kRoute[(int)p.route], kKernel[(int)k.kernel], k.chunk,
                   k.nchunks, k.fuse, kRoute[(int)k.route]);
        }
        // whatever the plan: the chunks cover the row, none is empty, and the ticket's query agrees with the route
        if (k.n_dense && (p.chunk * p.nchunks < k.n_dense || p.chunk * (p.nchunks - 1) >= k.n_dense)) { failures++; printf("FAIL chunks do not tile n_dense=%zu\n", k.n_dense); }
        const MsmTicket t{p.fuse ? 1ull : 0ull, (uint32_t)k.rows, p.route};
        if (t.delivers_without_sync() != (p.fuse != 0)) { failures++; printf("FAIL ticket query disagrees with fuse=%d\n", p.fuse); }
    }
    // the recoding constant: exactly W bits, at c - 1 + c w
    for (int c : {4, 8, 16, 17}) {
        const int W = 253 / c + 1;
        uint32_t K[9]; msm_recoding_constant(K, c, W);
        uint32_t want[9] = {0};
        for (int w = 0; w < W; w++) want[(c - 1 + c * w) / 32] |= 1u << ((c - 1 + c * w) % 32);
        int bits = 0;
        for (int i = 0; i < 9; i++) { bits += __builtin_popcount(K[i]); if (K[i] != want[i]) { failures++; printf("FAIL K word %d for c=%d\n", i, c); } }
        if (bits != W) { failures++; printf("FAIL K has %d bits for c=%d, W=%d\n", bits, c, W); }
        const MsmPlan p = msm_plan({c, W, 1, 16, 0, false, MSM_COMPRESSED, false, false, false, true});
        for (int i = 0; i < 9; i++) if (p.K[i] != K[i]) { failures++; printf("FAIL the plan's K differs for c=%d\n", c); break; }
    }
    printf("%zu plans checked, %d failures\n", sizeof kCases / sizeof kCases[0], failures);
    return failures ? 1 : 0;
}
