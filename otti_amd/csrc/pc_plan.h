// Layer plan of the batched product-circuit sum-check (snark_pc.cpp pcbatch_prove): which of a layer's rounds are a launch each, which the
// persistent tail (k_snark.hip k_pc_tail) plays, which the host; which launches are armed ahead of their challenge; where the layers the host
// plays alone are exported to.  Pure arithmetic over the layer's shape and the process's knobs — standard library only, so a host compiler
// can run it without HIP (tests/pc_plan_check.cpp pins the plans of the proofs' layers and the edges of the rule).
#pragma once
#include <algorithm>
#include <cstddef>

namespace otti {

constexpr int kTailCap = 1024;                               // elements per table and workgroup of the persistent tail (its LDS: three tables of them)
constexpr int kTailMaxGroups = 160;                          // its widest grid (rows of the tail's mail buffer)
// Places in the pinned result buffer (c.h_results)
constexpr int kPcTailSlot = 128;                             // where a layer's exported / handed-over tables start
constexpr int kPcPreExportEnd = 7400;                        // pre-exported host-only layers end below the hash layer's ahead-of-time results
constexpr int kHashEvalSlot = kPcPreExportEnd;               // result slots of the hash layer's 21 evaluations (clear of the round sums and the exported tails)
static_assert(kPcTailSlot < kPcPreExportEnd && kPcPreExportEnd <= kHashEvalSlot, "pre-exported layers would reach into the hash layer's ahead-of-time results");

// Grid of a launch over a batch of instances (k_snark.hip: the round kernel k_pc_round — items = pairs of a table's elements, quads with a fold —
// and the evaluations' k_dot_many, k_sum3 — items = elements): a thread per item up to max_blocks workgroups over ALL instances, the same number
// for each.  Beyond that the grid does not grow with the tables, the walk does: 18 instances of 2^19 items run on 113 workgroups each, 19 items
// per thread, and the 2^25 items per instance the library accepts are 1160.  k_pc_round takes any walk (pc_accum9.h kPcWalkMax: it folds its
// sums back every 256 items); the other two add canonical values.
constexpr int kPcThreads = 256;                              // threads per workgroup (device.h kBlock)
constexpr int kPcMaxBlocks = 2048;                           // the device's own max_blocks (device.h kMaxBlocks): 8 workgroups per CU of 256
struct PcGrid { unsigned workgroups; size_t items_per_thread; };   // per instance; the most items any thread walks
inline PcGrid pc_round_grid(size_t items, int ninst, size_t max_blocks) {
    const size_t per_inst = std::max<size_t>(1, max_blocks / (size_t)std::max(1, ninst));
    const size_t g = std::max<size_t>(1, std::min<size_t>((items + kPcThreads - 1) / kPcThreads, per_inst));
    return {(unsigned)g, (items + g * kPcThreads - 1) / (g * kPcThreads)};
}

// What the rule reads besides a layer's shape: the OTTI_PC_* switches (read once per process) and what the device and the process's state allow
// (per call).  The defaults are a 256-CU device's, with the AVX-512 IFMA host tail.
struct PcKnobs {
    size_t tail_cap = kTailCap;                              // OTTI_PC_TAIL_CAP: the tail's per-workgroup capacity, shrunk (tests)
    // elements of a table a workgroup of the tail starts with (it spreads wider only for what does not fit): fewer, busier workgroups mean fewer
    // mail lines per round for the host to collect — the larger cost (tools/hosttail_variants.sh)
    size_t tail_per_wg = 128;                                // OTTI_PC_TAIL_PER_WG
    // How many of a layer's last rounds the host plays (hosttail.h).  With the AVX-512 IFMA form a host round over tables of 32 / 64 elements costs
    // less than the 16 us of a round of the persistent launch: the last 6 rounds of the 12- and 18-instance batches (tables of 64), the last 7 of
    // the 4-instance batches (128); measured 4/5, 5/6, 5/7, 5/8, 6/7: product circuits 9.5, 9.1, 9.15, 9.3, 9.0 ms (tools/hosttail_variants.sh,
    // profiles/r4_hosttail_variants.txt).  With the scalar form (no such instructions): 4 and 5 as before (5/7 cost 10.9-11.4 ms against 10.7).
    size_t lgt_many = 6, lgt_few = 7;                        // OTTI_PC_LGT_MANY (8 instances and more), OTTI_PC_LGT_FEW
    size_t arm_max = (size_t)1 << 22;                        // OTTI_PC_ARM_MAX: elements of all instances' tables up to which a launch is armed (the sum-check kernels of the R1CS proof arm up to kArmMaxLen; here a round more or less ahead costs nothing else)
    // the tail's grid (W workgroups per instance, one per CU: 96 KB of LDS each) must be resident as a whole: never more workgroups than the device has CUs
    int tail_groups_max = kTailMaxGroups;                    // min(kTailMaxGroups, CUs)
    bool tail_ok = true;                                     // armed launches allowed, OTTI_PC_TAIL not 0, no tail timed out before, not a sharded proof
    bool arm_ok = true;                                      // DevCtx::armed_ok()
};

struct PcLayerShape { size_t nr; int ni; bool on_device; };  // variables (one round each; 2^nr elements per side), instances, tables in device memory

enum class PcRound { launch, tail, host };                   // a launch of its own; a round of the persistent launch; the host's

// what a layer's rounds are made of, decided from its shape alone (so that the NEXT layer's first launches can be issued ahead of time)
struct PcLayerPlan {
    size_t nr = 0, h = 1;                                    // elements per side in this layer, one round per variable
    size_t lgT = 0, T = 1, ndev = 0;                         // the device plays rounds 0 .. ndev - 1, the host the last lgT on tables of T elements
    size_t k0 = 0; int tailW = 1; bool tail = false;         // the persistent tail: first round it plays (== ndev: none), workgroups per instance
    PcRound round(size_t j) const { return j >= ndev ? PcRound::host : (tail && j >= k0) ? PcRound::tail : PcRound::launch; }
    // launch k >= 1 folds by r_{k-1} and yields the sums of round k (k < ndev) or the exported tail (k == ndev).  Armed (device.h), it is
    // queued one round ahead and starts the moment the host publishes r_{k-1}: small grids only; never the tail's own launch
    bool armed(size_t k, int ni, const PcKnobs &kn) const { return kn.arm_ok && k >= 1 && k < k0 + (tail ? 0 : 1) && k <= ndev && (h >> (k - 1)) * (size_t)ni <= kn.arm_max; }
};

inline PcLayerPlan pc_layer_plan(const PcLayerShape &s, const PcKnobs &kn) {
    PcLayerPlan p; p.nr = s.nr; p.h = (size_t)1 << s.nr;
    p.lgT = std::min<size_t>(s.nr, s.ni >= 8 ? kn.lgt_many : kn.lgt_few); p.T = (size_t)1 << p.lgT; p.ndev = s.nr - p.lgT;
    // The persistent tail (k_pc_tail, snark_dev.h): from round k0 on — the first round whose tables fit the LDS of W workgroups per
    // instance — ONE launch plays every remaining device round.  Only while this is the process's single proof in flight (its grid
    // must be resident as a whole: the workgroups wait for the host, the host for all of them) and no kernel class it belongs to is
    // being timed; otherwise, and for the rounds before k0, a launch per round as before.
    p.k0 = p.ndev; p.tailW = 1;
    if (p.ndev && kn.tail_ok && s.ni <= kn.tail_groups_max) {
        int Wmax = 1; while (2 * Wmax * s.ni <= kn.tail_groups_max && (size_t)(2 * Wmax) <= p.T) Wmax *= 2;
        const size_t cap_all = kn.tail_cap * (size_t)Wmax;
        p.k0 = 0; while ((p.h >> p.k0) > cap_all) p.k0++;
        if (p.k0 >= p.ndev) p.k0 = p.ndev;                   // (cannot happen for cap_all >= 2 T; kept for a shrunken test capacity)
        else { const size_t len0 = p.h >> p.k0; p.tailW = 1; while (p.tailW < Wmax && len0 / (size_t)p.tailW > kn.tail_per_wg) p.tailW *= 2; while (len0 / (size_t)p.tailW > kn.tail_cap) p.tailW *= 2; }
    }
    p.tail = p.k0 < p.ndev;
    return p;
}

// The layers the host plays alone are exported ahead of time, each to a place of its own.  Offered the layers' shapes in order (layer li has li
// variables), take() hands out the result slot of each leading layer that is — and -1 from the first with device rounds, the first not on the
// device, or the first whose three tables per instance would pass kPcPreExportEnd (the caller stops there).  at: the first slot not handed out.
struct PcPreExport {
    size_t at = kPcTailSlot;
    int take(const PcLayerShape &s, const PcKnobs &kn) {
        const PcLayerPlan p = pc_layer_plan(s, kn);
        const size_t need = (size_t)3 * s.ni * p.h;
        if (p.ndev || !s.on_device || at + need > (size_t)kPcPreExportEnd) return -1;
        const int slot = (int)at; at += need;
        return slot;
    }
};

}  // namespace otti
