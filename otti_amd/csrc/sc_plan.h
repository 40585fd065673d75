// Launch plan of the sum-check round kernels (k_sumcheck.hip): how wide a launch's grid is and how many items a thread walks.  Pure
// arithmetic over the table length and the device's capacities — standard library only, so a host compiler can run it without HIP
// (tests/sc_plan_check.cpp pins the launches of a 2^20 proof and the edges of the rule).
#pragma once
#include <algorithm>
#include <cstddef>

namespace otti {

constexpr int kScThreads = 256;                              // threads per workgroup of every round kernel
constexpr unsigned kScArmedWorkgroups = 64;                  // an armed launch waits for its challenge: no wider than this (device.h kArmMaxLen)
constexpr unsigned kScMaxWorkgroups = 2048;                  // rows of the partial-sum buffer (device.h kMaxBlocks)

enum class ScKind { cubic3_eval = 0, cubic3_fold = 1, quad_eval = 2, quad_fold = 3, cubic4_eval = 4, cubic4_fold = 5 };   // cubic4: the four-table round of the kernel ABI
constexpr int kScKinds = 6;

// The widest grid: two workgroups per CU, and never more than are resident at once.  Measured at 2^20 (profiles/sumcheck_split.md), kernels as
// they compile today (4, 2, 7 and 4 waves per SIMD): cubic3 evaluate 50.4 / 53.1 / 63.9 us and quad evaluate 29.0 / 31.8 / 44.4 us on 512 / 1024 /
// 2048 workgroups, the two folds 57.4 / 60.6 and 38.4 / 38.4 us on 512 / 1024 — more waves per SIMD bought nothing, more partial sums for the
// last workgroup cost; at 2^18 and below every item has a thread of its own on fewer workgroups than that.  Beyond 2^21 items the grid is as wide
// as the partial sums allow, as it has been since the kernels were measured at 2^24.
constexpr unsigned kScWorkgroupsPerCu = 2;
constexpr size_t kScWideItems = (size_t)1 << 21;
// The longest walk the tests pin is 64 items per thread (tests/test_gpu_sumcheck_walks.py): on 256 CUs the plan stays within it for every length up to 2^26.

// what the device says, once per process: its CUs and how many workgroups of each kernel are resident at once (occupancy per CU x CUs)
struct ScCaps {
    unsigned num_cu = 256;
    unsigned resident[kScKinds] = {512, 512, 512, 512, 512, 512};   // by ScKind
};
struct ScPlan { unsigned workgroups; size_t items, items_per_thread; };   // items: pairs (evaluate) or quadruples (fold) of table entries; per thread: the most any walks

inline size_t sc_ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

inline ScPlan sc_plan(ScKind kind, size_t len, bool armed, const ScCaps &caps) {
    const bool fold = ((int)kind & 1) != 0;
    ScPlan p;
    p.items = std::max<size_t>(1, fold ? len / 4 : len / 2);
    unsigned cap = p.items > kScWideItems ? kScMaxWorkgroups : std::min(caps.resident[(int)kind], kScWorkgroupsPerCu * caps.num_cu);
    cap = std::max(1u, std::min(cap, armed ? kScArmedWorkgroups : kScMaxWorkgroups));
    // the narrowest grid that gives every thread the fewest items `cap` workgroups allow: no workgroup walks an item more than another for
    // nothing, and the last one has fewer partial sums to add
    const size_t need = sc_ceil_div(p.items, kScThreads);
    p.workgroups = need <= cap ? (unsigned)need : (unsigned)sc_ceil_div(need, sc_ceil_div(need, cap));
    p.items_per_thread = sc_ceil_div(p.items, (size_t)p.workgroups * kScThreads);
    return p;
}

}  // namespace otti
