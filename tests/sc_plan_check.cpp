// The sum-check round kernels' launch plan (otti_amd/csrc/sc_plan.h) on the host: the grids of a 2^20 proof's two phases, the armed width and
// the edges of the rule, as values of the launchers' arithmetic.  Nothing here needs a GPU.
// Built and run by tests/test_sc_plan_host.py (plain g++, standard library only).
#include "sc_plan.h"
#include <cstdio>

using namespace otti;

constexpr ScKind C3E = ScKind::cubic3_eval, C3F = ScKind::cubic3_fold, QE = ScKind::quad_eval, QF = ScKind::quad_fold, C4E = ScKind::cubic4_eval, C4F = ScKind::cubic4_fold;
constexpr bool T = true, F = false;
struct Case { ScKind kind; int lg; bool armed; unsigned num_cu, resident; unsigned workgroups; size_t per; };

static const Case kCases[] = {
    // kind lg armed CUs resident  wgs  items per thread
    {C3E, 20, F, 256, 1024,  512, 4},      // phase one's first round: 2^19 items on two workgroups per CU
    {C3F, 20, F, 256,  512,  512, 2},      // its first fold
    {C3F, 19, F, 256,  512,  512, 1},
    {C3F, 17, F, 256,  512,  128, 1},
    {C3F, 16, T, 256,  512,   64, 1},      // the first armed round
    {C3F, 11, T, 256,  512,    2, 1},
    {C3F, 10, T, 256,  512,    1, 1},
    {C3F,  6, T, 256,  512,    1, 1},      // the shortest table a proof launches
    {C3F,  2, F, 256,  512,    1, 1},      // one item
    {QE,  20, F, 256, 1792,  512, 4},
    {QE,  18, F, 256, 1792,  512, 1},
    {QF,  20, F, 256, 1024,  512, 2},
    {QF,  16, T, 256, 1024,   64, 1},
    {QF,  18, T, 256, 1024,   64, 4},      // never an armed launch wider than 64, whatever its length
    {C4E, 20, F, 256, 1024,  512, 4},      // the four-table rounds of the kernel ABI
    {C4F, 12, F, 256,  512,    4, 1},
    {C4F, 22, F, 256,  512,  512, 8},
    {C3E, 22, F, 256, 1024,  512, 16},     // 2^21 items: still two per CU
    {C3E, 23, F, 256, 1024, 2048, 8},      // beyond: as wide as the partial sums allow
    {C3E, 20, F, 256,  256,  256, 8},      // a kernel of which only one workgroup per CU is resident
    {C3E, 20, F, 304, 1216,  512, 4},      // 608 allowed, 2048 wanted: four even walks of 512, not 608 walking 3.4
    {C3E, 20, F, 128,  512,  256, 8},      // half the CUs
    {QE,  20, F, 192,  768,  342, 6},      // 384 allowed: six walks, on the narrowest grid that still makes it six
};

int main() {
    int failures = 0;
    for (const Case &k : kCases) {
        ScCaps caps; caps.num_cu = k.num_cu;
        for (int i = 0; i < kScKinds; i++) caps.resident[i] = k.resident;
        const ScPlan p = sc_plan(k.kind, (size_t)1 << k.lg, k.armed, caps);
        if (p.workgroups != k.workgroups || p.items_per_thread != k.per) {
            failures++;
            printf("FAIL kind %d len 2^%d armed %d: %u workgroups, %zu items each; expected %u, %zu\n", (int)k.kind, k.lg, (int)k.armed, p.workgroups, p.items_per_thread, k.workgroups, k.per);
        }
    }
    // whatever the plan: the walks cover the table, no walk is empty, the partial-sum buffer holds the grid, an armed grid is at most 64 wide
    size_t swept = 0;
    for (int kind = 0; kind < kScKinds; kind++)
        for (int lg = 1; lg <= 26; lg++)
            for (int armed = 0; armed < 2; armed++)
                for (unsigned cus : {64u, 256u, 304u}) {
                    ScCaps caps; caps.num_cu = cus;
                    for (int i = 0; i < kScKinds; i++) caps.resident[i] = cus * (unsigned)(1 + i);
                    const size_t len = (size_t)1 << lg;
                    if ((kind & 1) && len < 4) continue;
                    const ScPlan p = sc_plan((ScKind)kind, len, armed != 0, caps);
                    const size_t threads = (size_t)p.workgroups * kScThreads;
                    swept++;
                    if (threads * p.items_per_thread < p.items || (p.items_per_thread > 1 && threads * (p.items_per_thread - 1) >= p.items)) { failures++; printf("FAIL kind %d 2^%d: walks do not tile the items\n", kind, lg); }
                    if (p.workgroups < 1 || p.workgroups > kScMaxWorkgroups || (armed && p.workgroups > kScArmedWorkgroups)) { failures++; printf("FAIL kind %d 2^%d: %u workgroups\n", kind, lg, p.workgroups); }
                    if (p.items != (size_t)((kind & 1) ? len / 4 : len / 2)) { failures++; printf("FAIL kind %d 2^%d: items\n", kind, lg); }
                }
    printf("%zu plans checked, %zu swept, %d failures\n", sizeof kCases / sizeof kCases[0], swept, failures);
    return failures ? 1 : 0;
}
