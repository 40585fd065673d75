// The per-item accumulation of the batched sum-check round kernel (otti_amd/csrc/pc_accum9.h: abe_accum9, abc_accum9 and the sweep / fold step
// pc_acc_step that k_snark.hip k_pc_round runs after every item) on the host, with an exact multi-word integer beside every accumulator.
//
// Every table of an instance holds one stored word in its lower half and one in its upper half, so every item of a walk adds the same three terms.
// The words come from {0, 1, l - 1, 2^252 - 1, 2^232, 2^29 - 1}, chosen independently per table and half: 6^6 triples, and 6^4 product circuits
// times the six eq factors 2^10 x word.  Checked:
//   (a) every term stays within the bound its comment states: 14.2 l for a triple's, 1.2 l for a product circuit's;
//   (b) kPcWalkMax terms of 14.2 l on top of what a fold leaves (below 2 l) stay below 2^264, the range of fr9_canon / fr9_fold_top;
//   (c) after kPcWalkMax items of the worst assignment of either kind fr9_canon(fr9_norm(acc)) is the exact sum mod l — and after 4096 items
//       walked with pc_acc_step, which folds limb 8 back every kPcWalkMax items, it still is.
// Printed: the smallest item count at which limb 8 of an accumulator that is only carry-swept (never folded) passes its 32 bits, and the assignment
// that does it — the corner tests/test_gpu_pc_round_walks.py walks on the device.
// Built and run by tests/test_pc_accum_host.py (g++, no GPU).
#include "../otti_amd/csrc/pc_accum9.h"
#include <stdio.h>
#include <stdint.h>
#include <string>
using namespace otti;

// ---- exact non-negative integers of 384 bits
struct Big { uint64_t w[6]; };
static Big big_zero() { Big r; for (int i = 0; i < 6; i++) r.w[i] = 0; return r; }
static Big big_add(const Big &a, const Big &b) { Big r; unsigned __int128 c = 0; for (int i = 0; i < 6; i++) { c += (unsigned __int128)a.w[i] + b.w[i]; r.w[i] = (uint64_t)c; c >>= 64; } return r; }
static Big big_sub(const Big &a, const Big &b) { Big r; __int128 c = 0; for (int i = 0; i < 6; i++) { c += (__int128)a.w[i] - b.w[i]; r.w[i] = (uint64_t)c; c >>= 64; } return r; }
static Big big_mul_small(const Big &a, uint64_t k) { Big r; unsigned __int128 c = 0; for (int i = 0; i < 6; i++) { c += (unsigned __int128)a.w[i] * k; r.w[i] = (uint64_t)c; c >>= 64; } return r; }
static int big_cmp(const Big &a, const Big &b) { for (int i = 5; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1; return 0; }
static Big big_shl(const Big &a, int s) {
    Big r = big_zero(); const int ws = s / 64, bs = s % 64;
    for (int i = 5; i >= ws; i--) { r.w[i] = a.w[i - ws] << bs; if (bs && i - ws - 1 >= 0) r.w[i] |= a.w[i - ws - 1] >> (64 - bs); }
    return r;
}
static Big big_shr(const Big &a, int s) {
    Big r = big_zero(); const int ws = s / 64, bs = s % 64;
    for (int i = 0; i + ws < 6; i++) { r.w[i] = a.w[i + ws] >> bs; if (bs && i + ws + 1 < 6) r.w[i] |= a.w[i + ws + 1] << (64 - bs); }
    return r;
}
static Big big_pow2(int s) { Big r = big_zero(); r.w[s / 64] = 1ull << (s % 64); return r; }
static Big big_from_words(const uint32_t w[8]) { Big r = big_zero(); for (int i = 0; i < 8; i++) r.w[i / 2] |= (uint64_t)w[i] << (32 * (i % 2)); return r; }
static Big big_l() { uint32_t w[8]; for (int i = 0; i < 8; i++) w[i] = fr_L(i); return big_from_words(w); }
static Big big_of(const Fr9 &a) { Big r = big_zero(); for (int i = 0; i < 9; i++) { Big t = big_zero(); t.w[0] = a.v[i]; r = big_add(r, big_shl(t, 29 * i)); } return r; }
static Big big_mod_l(Big a) {                                      // a < 2^383
    const Big l = big_l();
    for (int k = 130; k >= 0; k--) { const Big t = big_shl(l, k); if (big_cmp(a, t) >= 0) a = big_sub(a, t); }
    return a;
}
static Fr fr_of(const Big &a) { Fr r; for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)(a.w[i / 2] >> (32 * (i % 2))); return r; }

// ---- the stored words
static const char *const kWordName[6] = {"0", "1", "l - 1", "2^252 - 1", "2^232", "2^29 - 1"};
static Fr stored_word(int k) {
    Big b = big_zero();
    if (k == 1) b.w[0] = 1;
    if (k == 2) { Big one = big_zero(); one.w[0] = 1; b = big_sub(big_l(), one); }
    if (k == 3) { Big one = big_zero(); one.w[0] = 1; b = big_sub(big_pow2(252), one); }
    if (k == 4) b = big_pow2(232);
    if (k == 5) b.w[0] = (1u << 29) - 1;
    return fr_of(b);
}

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (failures < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } failures++; } } while (0)

// the three terms one item adds, as the kernel's evaluation path forms its operands from the stored words (k_pc_round, kFold == false)
struct Assign { bool triple; int a[2], b[2], c[2], e; };           // indices into the stored words: lower half, upper half; e: the eq factor's word
static void terms_of(const Assign &s, Fr9 (&t)[3]) {
    for (int k = 0; k < 3; k++) t[k] = fr9_zero();
    const Fr9 a_lo = fr9_unpack(stored_word(s.a[0])), a_hi = fr9_unpack(stored_word(s.a[1])), b_lo = fr9_unpack(stored_word(s.b[0])), b_hi = fr9_unpack(stored_word(s.b[1]));
    if (s.triple) abc_accum9(t, a_lo, a_hi, fr9_shl5(b_lo), fr9_shl5(b_hi), fr9_unpack5(stored_word(s.c[0])), fr9_unpack5(stored_word(s.c[1])));
    else abe_accum9(t, a_lo, a_hi, b_lo, b_hi, fr9_unpack_s<10>(stored_word(s.e)));
}
static std::string describe(const Assign &s) {
    char buf[256];
    if (s.triple) snprintf(buf, sizeof buf, "triple, (lower, upper) stored words A (%s, %s) B (%s, %s) C (%s, %s)", kWordName[s.a[0]], kWordName[s.a[1]], kWordName[s.b[0]], kWordName[s.b[1]], kWordName[s.c[0]], kWordName[s.c[1]]);
    else snprintf(buf, sizeof buf, "product circuit, (lower, upper) stored words A (%s, %s) B (%s, %s), eq factor 2^10 x %s", kWordName[s.a[0]], kWordName[s.a[1]], kWordName[s.b[0]], kWordName[s.b[1]], kWordName[s.e]);
    return buf;
}
// limb 8 of a sum of n equal terms T that is carry-swept after every fourth item and never folded: floor(n4 T / 2^232) + (n - n4) t8, n4 = n & ~3
// (after a sweep limbs 0 .. 7 are below 2^29, so limb 8 is the value's part from bit 232 up; the items since add their own limb 8)
static bool wraps_at(const Big &T, uint32_t t8, uint64_t n) {
    const uint64_t n4 = n & ~(uint64_t)3;
    Big top = big_shr(big_mul_small(T, n4), 232); Big add = big_zero(); add.w[0] = (n - n4) * (uint64_t)t8;
    return big_cmp(big_add(top, add), big_pow2(32)) >= 0;
}
static uint64_t first_wrap(const Big &T, uint32_t t8) {            // the smallest n at which limb 8 no longer fits (0: a zero term never does)
    if (!wraps_at(T, t8, (uint64_t)1 << 40)) return 0;
    uint64_t lo = 0, hi = (uint64_t)1 << 40;                      // wraps_at is monotone in n: 4 T / 2^232 >= 4 t8
    while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; (wraps_at(T, t8, mid) ? hi : lo) = mid; }
    return hi;
}

struct Worst { uint64_t wrap = 0; int sum = 0; Assign at{}; Big largest = big_zero(); Assign largest_at{}; };
static void visit(const Assign &s, Worst &w, const Big &bound_times_10) {
    Fr9 t[3]; terms_of(s, t);
    for (int k = 0; k < 3; k++) {
        const Big T = big_of(t[k]);
        for (int i = 0; i < 8; i++) EXPECT(t[k].v[i] <= FR9_M, "a term's limb %d is not normalised: %s", i, describe(s).c_str());
        EXPECT(big_cmp(big_mul_small(T, 10), bound_times_10) < 0, "term %d passes its stated bound: %s", k, describe(s).c_str());       // (a)
        if (big_cmp(T, w.largest) > 0) { w.largest = T; w.largest_at = s; }
        const uint64_t n = first_wrap(T, t[k].v[8]);
        if (n && (!w.wrap || n < w.wrap)) { w.wrap = n; w.sum = k; w.at = s; }
    }
}
// walk `items` items of s; fold: with pc_acc_step (the kernel's step), else with the bare sweep every fourth item.  Returns whether the canonical
// result is the exact sum mod l; *wrapped_at: the first item count at which a 64-bit shadow of limb 8 passed 32 bits (0: never)
static bool walk(const Assign &s, uint64_t items, bool fold, uint64_t *wrapped_at = nullptr) {
    Fr9 t[3]; terms_of(s, t);
    Fr9 acc[3] = {fr9_zero(), fr9_zero(), fr9_zero()}; Big exact[3] = {big_zero(), big_zero(), big_zero()};
    uint64_t shadow[3][9] = {}; unsigned n = 0;
    if (wrapped_at) *wrapped_at = 0;
    for (uint64_t it = 0; it < items; it++) {
        Fr9 one[3] = {acc[0], acc[1], acc[2]};
        const Fr9 a_lo = fr9_unpack(stored_word(s.a[0])), a_hi = fr9_unpack(stored_word(s.a[1])), b_lo = fr9_unpack(stored_word(s.b[0])), b_hi = fr9_unpack(stored_word(s.b[1]));
        if (s.triple) abc_accum9(one, a_lo, a_hi, fr9_shl5(b_lo), fr9_shl5(b_hi), fr9_unpack5(stored_word(s.c[0])), fr9_unpack5(stored_word(s.c[1])));
        else abe_accum9(one, a_lo, a_hi, b_lo, b_hi, fr9_unpack_s<10>(stored_word(s.e)));
        for (int k = 0; k < 3; k++) { acc[k] = one[k]; exact[k] = big_add(exact[k], big_of(t[k])); for (int i = 0; i < 9; i++) shadow[k][i] += t[k].v[i]; }
        if (fold) pc_acc_step(acc, n);
        else if ((++n & 3u) == 0) acc9_carry(acc);
        if (((it + 1) & 3) == 0) for (int k = 0; k < 3; k++) for (int i = 0; i < 8; i++) { shadow[k][i + 1] += shadow[k][i] >> 29; shadow[k][i] &= FR9_M; }
        if (wrapped_at && !*wrapped_at) for (int k = 0; k < 3; k++) if (shadow[k][8] >> 32) *wrapped_at = it + 1;
    }
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && fr_eq(fr9_canon(fr9_norm(acc[k])), fr_of(big_mod_l(exact[k])));
    return ok;
}

int main() {
    const Big l = big_l();
    static_assert(kPcWalkMax % 4 == 0 && kPcWalkMax <= 288, "the walk bound: a multiple of the sweep's four items, within the 288 items the term bound proves");
    // (b) kPcWalkMax terms below 14.2 l on top of a folded value below 2 l stay below 2^264 (times 10: 142 l kPcWalkMax + 20 l < 10 * 2^264)
    EXPECT(big_cmp(big_add(big_mul_small(big_mul_small(l, 142), kPcWalkMax), big_mul_small(l, 20)), big_mul_small(big_pow2(264), 10)) < 0, "kPcWalkMax x 14.2 l + 2 l reaches 2^264");

    Worst triple, circuit; size_t visited = 0;
    const Big l142 = big_mul_small(l, 142), l12 = big_mul_small(l, 12);
    Assign s{}; s.triple = true;
    for (s.a[0] = 0; s.a[0] < 6; s.a[0]++) for (s.a[1] = 0; s.a[1] < 6; s.a[1]++) for (s.b[0] = 0; s.b[0] < 6; s.b[0]++) for (s.b[1] = 0; s.b[1] < 6; s.b[1]++)
        for (s.c[0] = 0; s.c[0] < 6; s.c[0]++) for (s.c[1] = 0; s.c[1] < 6; s.c[1]++) { visit(s, triple, l142); visited++; }
    s = Assign{}; s.triple = false;
    for (s.a[0] = 0; s.a[0] < 6; s.a[0]++) for (s.a[1] = 0; s.a[1] < 6; s.a[1]++) for (s.b[0] = 0; s.b[0] < 6; s.b[0]++) for (s.b[1] = 0; s.b[1] < 6; s.b[1]++)
        for (s.e = 0; s.e < 6; s.e++) { visit(s, circuit, l12); visited++; }
    // (b) again, with the largest term met in the place of the stated bound
    EXPECT(big_cmp(big_add(big_mul_small(triple.largest, kPcWalkMax), big_mul_small(l, 2)), big_pow2(264)) < 0, "kPcWalkMax x the largest term met + 2 l reaches 2^264");

    for (const Worst *w : {&triple, &circuit}) {
        EXPECT(w->wrap != 0, "no assignment ever wraps");
        if (!w->wrap) continue;
        // the closed form of first_wrap against the walk itself: exact up to the item before, limb 8 past its 32 bits at the count it names
        uint64_t seen = 0;
        EXPECT(w->wrap > kPcWalkMax, "an unfolded accumulator wraps within kPcWalkMax items: %s", describe(w->at).c_str());
        if (w->wrap <= 8192) {
            EXPECT(walk(w->at, w->wrap - 1, false, &seen) && seen == 0, "wrong sums before the predicted wrap: %s", describe(w->at).c_str());
            walk(w->at, w->wrap, false, &seen);
            EXPECT(seen == w->wrap, "limb 8 wraps at %llu items, not at the predicted %llu: %s", (unsigned long long)seen, (unsigned long long)w->wrap, describe(w->at).c_str());
        }
        // (c)
        EXPECT(walk(w->at, kPcWalkMax, false), "after kPcWalkMax items the canonical sums are not the exact ones: %s", describe(w->at).c_str());
        EXPECT(walk(w->largest_at, kPcWalkMax, false), "after kPcWalkMax items of the largest term the canonical sums are not the exact ones: %s", describe(w->largest_at).c_str());
        for (uint64_t items : {(uint64_t)kPcWalkMax, (uint64_t)kPcWalkMax + 1, (uint64_t)683, (uint64_t)1024, (uint64_t)4096, (uint64_t)4099})
            EXPECT(walk(w->at, items, true) && walk(w->largest_at, items, true), "pc_acc_step: after %llu items the canonical sums are not the exact ones", (unsigned long long)items);
        printf("pc_accum: limb 8 first wraps after %llu items (sum %d of a %s)\n", (unsigned long long)w->wrap, w->sum, describe(w->at).c_str());
    }
    printf("pc_accum check: %zu assignments, kPcWalkMax %u, %d failures\n", visited, kPcWalkMax, failures);
    return failures != 0;
}
