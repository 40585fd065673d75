// A thread's running sums in nine limbs (fr9.h) as the round kernels keep them, and what one item of the batched product-circuit sum-check
// (k_snark.hip k_pc_round) adds to them.  Host and device read the same text: tests/pc_accum_check.cpp walks it beside exact integers.
#pragma once
#include "fr9.h"

namespace otti {

// a thread's running sums (limbs grow by < 2^29 per item: carried down every fourth item) -> canonical words
HD void acc9_carry(Fr9 (&acc)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) acc[k] = fr9_norm(acc[k]);
}
template <int K> HD void acc9_canon(Fr (&out)[K], const Fr9 (&acc)[K]) {
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = fr9_canon(fr9_norm(acc[k]));
}

// ---- Product-circuit instance (third table = the shared eq table, never stored): per item
//   Q(0) += (E a_lo) b_lo,  Q(1) += (E a_hi) b_hi,  Q_inf += (E a_hi - E a_lo)(b_hi - b_lo)
// — the quadratic's values at 0, 1 and its leading coefficient, in FIVE products (E a_lo and E a_hi serve two sums each; six when E multiplied
// the three products a b); finish_many turns the totals into the values at 0, 2, 3.  E goes in times 2^10: E a_* then carries the factor 32
// the second product needs.  a_*, b_* normalised below 2.2 l; e10 normalised below 2^10 l.
HD void abe_accum9(Fr9 (&acc)[3], const Fr9 &a_lo, const Fr9 &a_hi, const Fr9 &b_lo, const Fr9 &b_hi, const Fr9 &e10) {
    const Fr9 u = fr9_mul(e10, a_lo), v = fr9_mul(e10, a_hi);                               // 2^10 l * 2.2 l / 2^261 + l < 5.4 l
    const Fr9 dv = fr9_norm(fr9_sub_kl<8>(v, u)), db = fr9_sub_kl<4>(b_hi, b_lo);           // < 13.4 l; < 6.2 l (loose)
    acc[0] = fr9_add(acc[0], fr9_mul(u, b_lo));                                             // 5.4 * 2.2 / 2^9 + 1 < 1.1 l
    acc[1] = fr9_add(acc[1], fr9_mul(v, b_hi));
    acc[2] = fr9_add(acc[2], fr9_mul(dv, db));                                              // 13.4 * 6.2 / 2^9 + 1 < 1.2 l
}
// Dot-product triple (three real tables): the cubic's values at 0, 2, 3 as they stand.  a_* plain, b_*5 and c_*5 times 32.
HD void abc_accum9(Fr9 (&acc)[3], const Fr9 &a_lo, const Fr9 &a_hi, const Fr9 &b_lo5, const Fr9 &b_hi5, const Fr9 &c_lo5, const Fr9 &c_hi5) {
    acc[0] = fr9_add(acc[0], fr9_mul(fr9_mul(a_lo, b_lo5), c_lo5));
    // point 2: x = 2 a_hi - a_lo + 4l (carried down), y5, z5 = 2 X_hi5 - X_lo5 + 128 l (limbs < 2^31): values 8.4 l, 270 l: products < 5.5 l, < 3.9 l
    const Fr9 x2 = fr9_norm(fr9_sub_kl<4>(fr9_add(a_hi, a_hi), a_lo));
    const Fr9 y2 = fr9_sub_kl<128>(fr9_add(b_hi5, b_hi5), b_lo5), z2 = fr9_sub_kl<128>(fr9_add(c_hi5, c_hi5), c_lo5);
    acc[1] = fr9_add(acc[1], fr9_mul(fr9_mul(x2, y2), z2));
    // point 3: X_3 = X_2 + (X_hi - X_lo): carried down on every side (their limbs would reach 3.5 * 2^30)
    const Fr9 x3 = fr9_norm(fr9_add(x2, fr9_sub_kl<4>(a_hi, a_lo)));
    const Fr9 y3 = fr9_norm(fr9_add(y2, fr9_sub_kl<128>(b_hi5, b_lo5))), z3 = fr9_norm(fr9_add(z2, fr9_sub_kl<128>(c_hi5, c_lo5)));
    acc[2] = fr9_add(acc[2], fr9_mul(fr9_mul(x3, y3), z3));          // values 14.6 l, 469 l: 14.6 * 469 / 512 + 1 = 14.4 l, then 14.4 * 469 / 512 + 1 = 14.2 l
}
// The walk bound.  The sweep only moves carries INTO limb 8; nothing takes them out again before fr9_canon, which is exact for values below
// 2^264 (limb 8 within its 32 bits) — a little under 4096 l.  A triple's term is below 14.2 l (above), so a sum that starts below 2 l holds
// kPcWalkMax = 256 items: 256 * 14.2 l + 2 l = 3637.2 l < 2^264 (288 items would still fit; 256 is the multiple of the sweep's four that
// costs one mask to test, and it divides 2^32, so the count may wrap).  A grid that does not grow with the tables (pc_plan.h pc_round_grid)
// walks further than that — 1160 items at the 2^25 items per instance the library accepts, with 18 instances — and limb 8 of an accumulator
// that is only swept wraps after 596 items of a triple's worst words, 3736 of a product circuit's (tests/pc_accum_check.cpp finds and prints
// them).  So every kPcWalkMax items the step folds limb 8 back (fr9_fold_top: the same value mod l, below 2 l) and the walk may be as long as
// it likes: k_pc_round has no bound on its walk left, the sweep's cost is unchanged and the fold's is 3 / 256 of a canonicalisation per item.
constexpr unsigned kPcWalkMax = 256;
static_assert(kPcWalkMax % 4 == 0 && (kPcWalkMax & (kPcWalkMax - 1)) == 0 && kPcWalkMax <= 288, "the fold sits on a sweep, its test is a mask, and 288 items are what the term bound proves");
// after every item of a walk: the carry sweep every fourth item (the limbs 0 .. 7 of an item's terms are below 2^29), the fold every kPcWalkMax
HD void pc_acc_step(Fr9 (&acc)[3], unsigned &n) {
    if ((++n & 3u) == 0) {
        acc9_carry(acc);
        if ((n & (kPcWalkMax - 1)) == 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) acc[k] = fr9_fold_top(acc[k]);
        }
    }
}

}  // namespace otti
