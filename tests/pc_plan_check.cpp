// The layer plan of the batched product-circuit sum-check (otti_amd/csrc/pc_plan.h) on the host: which rounds of a layer are launches, which
// the persistent tail's, which the host's, which launches are armed and where the host-only layers are exported to — for the layers of the
// proofs the GPU tests run, under the switches those tests set, and over a sweep of shapes for what k_pc_tail and the prover rely on.
// Nothing here needs a GPU.  Built and run by tests/test_pc_plan_host.py (plain g++, standard library only).
#include "pc_plan.h"
#include <cstdio>
#include <vector>

using namespace otti;

enum Variant { dflt, cap16, no_tail, cu64, cu16, lgt45 };
static const char *const kVariantName[] = {"default", "tail_cap 16", "tail_ok off", "64 CUs", "16 CUs", "lgt 4/5"};
static PcKnobs knobs_of(Variant v) {
    PcKnobs k;                                              // 256 CUs, IFMA host tail (6 / 7), capacity 1024, 128 per workgroup, 160 groups
    if (v == cap16) k.tail_cap = 16;
    if (v == no_tail) k.tail_ok = false;
    if (v == cu64) k.tail_groups_max = 64;
    if (v == cu16) k.tail_groups_max = 16;
    if (v == lgt45) { k.lgt_many = 4; k.lgt_few = 5; }
    return k;
}
constexpr bool Y = true, N = false;
struct Case { int ni; size_t nr; Variant v; size_t lgT, ndev, k0; int tailW; bool tail; size_t armed_lo, armed_hi; };   // armed launches: lo .. hi (0, 0: none)

static const Case kCases[] = {
    // ni  nr  knobs   lgT ndev k0 tailW tail armed
    { 4,  7, dflt,    7,  0,  0,  1, N, 0, 0},      // the longest layer a 4-instance batch leaves to the host
    { 4,  8, dflt,    7,  1,  0,  2, Y, 0, 0},      // one device round: the tail from round 0 on
    { 4, 12, dflt,    7,  5,  0, 32, Y, 0, 0},
    { 4, 20, dflt,    7, 13,  5, 32, Y, 1, 4},      // the memory circuits' input layer at 2^20
    {12,  7, dflt,    6,  1,  0,  1, Y, 0, 0},
    {12, 14, dflt,    6,  8,  1,  8, Y, 0, 0},      // one launch round, then the tail: its own launch is never armed
    {12, 20, dflt,    6, 14,  7,  8, Y, 3, 6},      // launches 1, 2 are over more than 2^22 elements
    {18, 20, dflt,    6, 14,  7,  8, Y, 4, 6},      // the operations circuits' input layer (with the dot-product triples) at 2^20
    {18, 18, dflt,    6, 12,  5,  8, Y, 2, 4},
    { 4,  8, cap16,   7,  1,  0, 16, Y, 0, 0},      // OTTI_PC_TAIL_CAP=16 (tests/test_gpu_snark.py)
    {12,  8, cap16,   6,  2,  1,  8, Y, 0, 0},
    {12, 12, cap16,   6,  6,  5,  8, Y, 1, 4},      // the tail picks up tables that launches folded in HBM
    {12, 12, no_tail, 6,  6,  6,  1, N, 1, 6},      // OTTI_PC_TAIL=0: a launch per round, the export (launch ndev) armed too
    {12, 22, no_tail, 6, 16, 16,  1, N, 5, 16},
    {12, 12, cu64,    6,  6,  0,  4, Y, 0, 0},      // a smaller device: fewer workgroups per instance
    {18, 12, cu64,    6,  6,  1,  2, Y, 0, 0},
    {18, 12, cu16,    6,  6,  6,  1, N, 1, 6},      // more instances than the grid may have workgroups: no tail
    {12,  6, lgt45,   4,  2,  0,  1, Y, 0, 0},      // the scalar host tail: 4 / 5 rounds
    { 4,  6, lgt45,   5,  1,  0,  1, Y, 0, 0},
};

// Pre-export at the defaults: layer li has li variables; slots of the leading host-only layers and where they end.  The input layer (the last,
// nl - 1 variables) carries the six dot-product triples of the operations circuits; it is host-only — and then pre-exported with 18 instances —
// only for circuits of at most 2^7 elements (nl - 1 <= lgt_many), which SNARK::prove accepts: the third case.
struct PreCase { int ni; size_t nl; int ni_last; size_t n; int slot[8]; size_t end; };
static const PreCase kPreCases[] = {
    { 4, 20,  4, 8, {128, 140, 164, 212, 308, 500, 884, 1652}, 3188},
    {12, 20, 18, 7, {128, 164, 236, 380, 668, 1244, 2396}, 4700},
    {12,  7, 18, 7, {128, 164, 236, 380, 668, 1244, 2396}, 5852},
};

// The grid of a launch over a batch (pc_round_grid): workgroups per instance and the most items a thread walks, on both sides of the cap
struct GridCase { size_t items; int ninst; size_t max_blocks; unsigned workgroups; size_t walk; };
static const GridCase kGridCases[] = {
    // items                   ninst  cap   workgroups walk
    {1,                           1, 2048,     1,    1},
    {256,                         1, 2048,     1,    1},
    {257,                         1, 2048,     2,    1},
    {(size_t)2048 * 256,          1, 2048,  2048,    1},      // the last length with a thread per item
    {(size_t)2048 * 256 + 1,      1, 2048,  2048,    2},
    {(size_t)1 << 25,             1, 2048,  2048,   64},
    {(size_t)113 * 256,          18, 2048,   113,    1},      // 2048 / 18 = 113 workgroups per instance
    {(size_t)113 * 256 + 1,      18, 2048,   113,    2},
    {(size_t)1 << 15,            18, 2048,   113,    2},      // tests/test_gpu_snark_kernels.py test_pc_round_at_the_grid_cap
    {(size_t)1 << 19,            18, 2048,   113,   19},      // the operations circuits' input layer of a 2^20 proof: 18.1 items per thread
    {(size_t)1 << 25,            18, 2048,   113, 1160},      // the longest tables the library accepts: far beyond kPcWalkMax
    {(size_t)102 * 256,          20, 2048,   102,    1},      // 2048 / 20 = 102
    {(size_t)102 * 256 + 1,      20, 2048,   102,    2},
    {(size_t)1 << 19,            20, 2048,   102,   21},
    {(size_t)256 * 64,           18,   18,     1,   64},      // the tests' seam: one workgroup per instance ...
    {(size_t)1 << 18,             3,    3,     1, 1024},
    {2048,                        2,    6,     3,    3},      // ... three, ragged: walks of 3 / 2 and 6 / 5
    {4096,                        2,    6,     3,    6},
    {(size_t)1 << 19,             1,    3,     3,  683},
    {(size_t)1 << 12,            18,    1,     1,   16},      // a cap below the instances still gives each its workgroup
    {5,                          64, 2048,     1,    1},
};

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; printf("FAIL " __VA_ARGS__); printf("\n"); } } while (0)

static std::vector<PcLayerShape> layers_of(int ni, size_t nl, int ni_last) {
    std::vector<PcLayerShape> v;
    for (size_t li = 0; li < nl; li++) v.push_back({li, li + 1 == nl ? ni_last : ni, true});
    return v;
}
// the slots PcPreExport hands out for the leading layers of v, up to the first it refuses; *end: the first slot after them
static std::vector<int> pc_preexport_slots(const std::vector<PcLayerShape> &v, const PcKnobs &kn, size_t *end = nullptr) {
    PcPreExport pre; std::vector<int> slots;
    for (const PcLayerShape &s : v) { const int slot = pre.take(s, kn); if (slot < 0) break; slots.push_back(slot); }
    if (end) *end = pre.at;
    return slots;
}
static bool pow2(size_t x) { return x && !(x & (x - 1)); }

int main() {
    for (const Case &k : kCases) {
        const PcKnobs kn = knobs_of(k.v);
        const PcLayerPlan p = pc_layer_plan({k.nr, k.ni, true}, kn);
        EXPECT(p.lgT == k.lgT && p.ndev == k.ndev && p.k0 == k.k0 && p.tailW == k.tailW && p.tail == k.tail && p.nr == k.nr && p.h == (size_t)1 << k.nr && p.T == (size_t)1 << k.lgT,
               "ni %d nr %zu %s: lgT %zu ndev %zu k0 %zu tailW %d tail %d; expected %zu %zu %zu %d %d", k.ni, k.nr, kVariantName[k.v], p.lgT, p.ndev, p.k0, p.tailW, (int)p.tail, k.lgT, k.ndev, k.k0, k.tailW, (int)k.tail);
        for (size_t a = 0; a <= k.nr + 2; a++)
            EXPECT(p.armed(a, k.ni, kn) == (a >= 1 && a >= k.armed_lo && a <= k.armed_hi), "ni %d nr %zu %s: launch %zu armed %d; expected armed %zu .. %zu", k.ni, k.nr, kVariantName[k.v], a, (int)p.armed(a, k.ni, kn), k.armed_lo, k.armed_hi);
    }
    for (const PreCase &k : kPreCases) {
        size_t end = 0;
        const std::vector<int> slots = pc_preexport_slots(layers_of(k.ni, k.nl, k.ni_last), PcKnobs{}, &end);
        EXPECT(slots.size() == k.n && end == k.end, "pre-export ni %d nl %zu: %zu layers ending at %zu; expected %zu, %zu", k.ni, k.nl, slots.size(), end, k.n, k.end);
        for (size_t li = 0; li < slots.size() && li < k.n; li++) EXPECT(slots[li] == k.slot[li], "pre-export ni %d nl %zu: layer %zu at %d; expected %d", k.ni, k.nl, li, slots[li], k.slot[li]);
    }
    {   // the run ends at the first layer that is not on the device
        std::vector<PcLayerShape> v = layers_of(12, 20, 18); v[3].on_device = false;
        EXPECT(pc_preexport_slots(v, PcKnobs{}).size() == 3, "pre-export does not stop at the first layer that is not on the device");
    }

    // whatever the shape and the knobs: what k_pc_tail (dev_pc_tail's own rejection conditions) and the prover's round loop rely on
    size_t swept = 0;
    for (int ni : {1, 4, 12, 18, 20})
        for (size_t nr = 0; nr <= 26; nr++)
            for (int cus : {16, 64, 256, 304})
                for (size_t cap : {(size_t)2, (size_t)16, (size_t)1024})
                    for (int tail_ok = 0; tail_ok < 2; tail_ok++) {
                        PcKnobs kn; kn.tail_groups_max = std::min(kTailMaxGroups, cus); kn.tail_cap = cap; kn.tail_ok = tail_ok != 0;
                        const PcLayerPlan p = pc_layer_plan({nr, ni, true}, kn);
                        swept++;
#define AT "ni %d nr %zu CUs %d cap %zu tail_ok %d: "
#define ATV ni, nr, cus, cap, tail_ok
                        EXPECT(p.lgT + p.ndev == nr && p.T == (size_t)1 << p.lgT && p.h == (size_t)1 << nr, AT "rounds do not add up", ATV);
                        EXPECT(pow2((size_t)p.tailW), AT "tailW %d", ATV, p.tailW);
                        EXPECT(p.k0 <= p.ndev && p.tail == (p.k0 < p.ndev), AT "k0 %zu ndev %zu tail %d", ATV, p.k0, p.ndev, (int)p.tail);
                        EXPECT(tail_ok || !p.tail, AT "a tail that is switched off", ATV);
                        if (p.tail) {
                            EXPECT(ni * p.tailW <= kn.tail_groups_max, AT "%d workgroups", ATV, ni * p.tailW);
                            EXPECT((p.h >> p.k0) / (size_t)p.tailW <= kn.tail_cap && (size_t)p.tailW <= p.T, AT "tailW %d for %zu elements, T %zu", ATV, p.tailW, p.h >> p.k0, p.T);
                        }
                        for (size_t j = 0; j < nr + 2; j++) {
                            const PcRound r = p.round(j);
                            EXPECT((r == PcRound::host) == (j >= p.ndev) && (r == PcRound::tail) == (p.tail && j >= p.k0 && j < p.ndev), AT "round %zu is of kind %d", ATV, j, (int)r);
                            if (p.armed(j, ni, kn)) EXPECT(j >= 1 && j <= p.ndev && !(p.tail && j >= p.k0), AT "launch %zu armed", ATV, j);
                        }
                        kn.arm_ok = false;
                        for (size_t j = 0; j < nr + 2; j++) EXPECT(!p.armed(j, ni, kn), AT "launch %zu armed against arm_ok", ATV, j);
                    }
    // the pre-exported layers' places: disjoint, in order, from kPcTailSlot to at most kPcPreExportEnd, host-only layers all
    for (int ni : {1, 4, 12, 18, 20})
        for (size_t nl = 1; nl <= 27; nl++)
            for (int dotp = 0; dotp <= 6 && ni + dotp <= 20; dotp += 6)
                for (size_t lgt : {(size_t)4, (size_t)6, (size_t)8}) {
                    PcKnobs kn; kn.lgt_many = lgt; kn.lgt_few = lgt + 1;
                    const std::vector<PcLayerShape> v = layers_of(ni, nl, ni + dotp);
                    size_t end = 0, at = kPcTailSlot;
                    const std::vector<int> slots = pc_preexport_slots(v, kn, &end);
                    swept++;
                    EXPECT(slots.size() <= nl, "pre-export ni %d nl %zu: more slots than layers", ni, nl);
                    for (size_t li = 0; li < slots.size() && li < nl; li++) {
                        EXPECT((size_t)slots[li] == at && pc_layer_plan(v[li], kn).ndev == 0, "pre-export ni %d nl %zu lgt %zu: layer %zu at %d, free from %zu", ni, nl, lgt, li, slots[li], at);
                        at += (size_t)3 * v[li].ni << li;
                    }
                    EXPECT(end == at && end <= (size_t)kPcPreExportEnd, "pre-export ni %d nl %zu lgt %zu: ends at %zu", ni, nl, lgt, end);
                }
    for (const GridCase &k : kGridCases) {
        const PcGrid g = pc_round_grid(k.items, k.ninst, k.max_blocks);
        EXPECT(g.workgroups == k.workgroups && g.items_per_thread == k.walk, "grid of %zu items x %d under %zu blocks: %u workgroups, walk %zu; expected %u, %zu", k.items, k.ninst, k.max_blocks, g.workgroups, g.items_per_thread, k.workgroups, k.walk);
    }
    // whatever the shape: every item has a thread's pass, no pass is wholly idle, and the grid stays within the cap (the partial sums' buffers)
    for (int ninst : {1, 4, 12, 18, 20, 64})
        for (size_t cap : {(size_t)1, (size_t)18, (size_t)54, (size_t)2048})
            for (size_t items : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)28928, (size_t)28929, (size_t)1 << 19, ((size_t)1 << 19) + 1, (size_t)1 << 25}) {
                const PcGrid g = pc_round_grid(items, ninst, cap);
                const size_t threads = (size_t)g.workgroups * kPcThreads;
                swept++;
                EXPECT(g.workgroups >= 1 && ((size_t)g.workgroups * ninst <= cap || g.workgroups == 1), "grid of %zu x %d under %zu: %u workgroups", items, ninst, cap, g.workgroups);
                EXPECT(g.items_per_thread * threads >= items && (g.items_per_thread - 1) * threads < items, "grid of %zu x %d under %zu: walk %zu on %zu threads", items, ninst, cap, g.items_per_thread, threads);
                EXPECT((size_t)(g.workgroups - 1) * kPcThreads < items, "grid of %zu x %d under %zu: an idle workgroup among %u", items, ninst, cap, g.workgroups);
            }
    printf("%zu plans checked, %zu pre-exports, %zu grids, %zu swept, %d failures\n", sizeof kCases / sizeof kCases[0], sizeof kPreCases / sizeof kPreCases[0], sizeof kGridCases / sizeof kGridCases[0], swept, failures);
    return failures ? 1 : 0;
}
