// Host build of the nine-limb field arithmetic (otti_amd/csrc/fr9.h, fp9.h: the C bodies; the device uses generated asm blocks, which
// tests/test_gpu_scalar_arith.py (GF(l)) and tests/test_gpu_curve_arith.py (GF(2^255-19)) run on the same pools) checked against the 8 x u32
// arithmetic of field.h / point.h on random inputs and on the edge pool of tests/curve_cases.py, and, given a case file as second argument,
// against the plain-integer reference of tests/scalar_cases.py on its pool (limb for limb).
// Built and run by tests/test_limb9_host.py and tests/test_scalar_cases_host.py (g++, no GPU): limb9_check [iterations [case file]].
#include "fr9.h"
#include "fp9.h"
#include <stdio.h>
#include <string.h>
#include <random>
#include <vector>
using namespace otti;
static std::mt19937_64 rng(20261004);
static Fr rnd_fr() { Fr t; for (int i = 0; i < 8; i++) t.v[i] = (uint32_t)rng(); t.v[7] &= 0x0fffffffu; uint32_t w[8]; for (int i = 0; i < 8; i++) w[i] = t.v[i]; return fr_cond_sub_l(w, 0); }
static Fp rnd_fp() { Fp t; for (int i = 0; i < 8; i++) t.v[i] = (uint32_t)rng(); return t; }
static Fr l_minus(uint32_t k) { Fr a; for (int i = 0; i < 8; i++) a.v[i] = fr_L(i); a.v[0] -= k; return a; }
// ---- the edge pool of tests/curve_cases.py (limb-boundary and non-canonical 256-bit words) through the plain-C bodies of fp9.h: all pairs for the
// operations of two operands, the compound shapes whose operands sit at the bounds fp9.h states, and p9_madd (both signs, two in a chain, output bound)
static Fp raw_pow2(int s) { Fp r = fp_zero(); r.v[s >> 5] = 1u << (s & 31); return r; }
static Fp raw_sub1(Fp a) { for (int i = 0; i < 8; i++) { if (a.v[i]--) break; } return a; }                 // a - 1 on the raw words (a != 0)
static Fp raw_add(Fp a, uint32_t k) { uint64_t c = k; for (int i = 0; i < 8; i++) { c += a.v[i]; a.v[i] = (uint32_t)c; c >>= 32; } return a; }
static std::vector<Fp> edge_pool() {
    const Fp ones = fp_from_words(~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u);
    Fp p = ones; p.v[0] = 0xffffffedu; p.v[7] = 0x7fffffffu;                                                 // 2^255 - 19
    Fp two_p = ones; two_p.v[0] = 0xffffffdau;                                                               // 2^256 - 38
    Fp half = p; half.v[0] = 0xfffffff6u; half.v[7] = 0x3fffffffu;                                           // (p - 1) / 2 = 2^254 - 10
    std::vector<Fp> v = {fp_zero(), fp_one(), raw_add(fp_zero(), 2), raw_add(fp_zero(), 19), raw_sub1(p), p, raw_add(p, 1), raw_sub1(raw_pow2(255)), raw_pow2(255),
                         raw_add(raw_pow2(255), 18), two_p, ones, half, fp_D(), fp_2D(), fp_SQRT_M1()};
    for (int k = 1; k <= 8; k++) { v.push_back(raw_pow2(29 * k)); v.push_back(raw_sub1(raw_pow2(29 * k))); }
    const int ten[9] = {26, 51, 77, 102, 128, 153, 179, 204, 230};
    for (int s : ten) { v.push_back(raw_pow2(s)); v.push_back(raw_sub1(raw_pow2(s))); }
    return v;
}
static bool f9_reduced(const F9 &a) {
    for (int i = 0; i < 8; i++) if (a.v[i] >= (1u << 29) + (i < 2 ? (1u << 18) : 0u)) return false;
    return a.v[8] < (1u << 23) + 2;
}
static bool p9_reduced(const P9 &q) { return f9_reduced(q.X) && f9_reduced(q.Y) && f9_reduced(q.Z) && f9_reduced(q.T); }
static bool pt_same(const Pt &a, const Pt &b) { return fp_eq(a.X, b.X) && fp_eq(a.Y, b.Y) && fp_eq(a.Z, b.Z) && fp_eq(a.T, b.T); }
static int edge_pool_checks() {
    const std::vector<Fp> pool = edge_pool();
    const size_t n = pool.size();
    int bad = 0;
#define ECHECK(cond, what) do { if (!(cond)) { if (bad < 10) printf("FAIL edge pool: %s\n", what); bad++; } } while (0)
    for (size_t i = 0; i < n; i++) {
        const Fp a = pool[i]; const F9 a9 = f9_unpack(a);
        ECHECK(f9_reduced(a9) && fp_eq(f9_pack(a9), a), "unpack / pack");
        ECHECK(fp_eq(f9_pack(f9_neg(a9)), fp_neg(a)), "neg");
        for (size_t j = 0; j < n; j++) {
            const Fp b = pool[j]; const F9 b9 = f9_unpack(b);
            const F9 m = f9_mul(a9, b9);
            ECHECK(f9_reduced(m) && fp_eq(f9_pack(m), fp_mul(a, b)), "mul");
            ECHECK(fp_eq(f9_pack(f9_add(a9, b9)), fp_add(a, b)), "add");
            ECHECK(fp_eq(f9_pack(f9_sub(a9, b9)), fp_sub(a, b)), "sub");
            const F9 m32 = f9_mul(f9_add(f9_add(a9, a9), a9), f9_add(b9, b9));                             // fp9.h's 3 * 2^29 x 2^30
            ECHECK(f9_reduced(m32) && fp_eq(f9_pack(m32), fp_mul(fp_add(fp_add(a, a), a), fp_add(b, b))), "(a+a+a)(b+b)");
        }
    }
    // quadruples and point tuples: every all-equal tuple of the three largest words, then a seeded walk over the pool
    const size_t big[3] = {11, 7, 4};                                                                    // 2^256 - 1, 2^255 - 1, p - 1
    std::mt19937_64 pick(20261020);
    for (int it = 0; it < 4000; it++) {
        Fp t[7];
        for (int k = 0; k < 7; k++) t[k] = it < 3 ? pool[big[it]] : ((it & 1) && (pick() & 1) ? pool[big[pick() % 3]] : pool[pick() % n]);
        const F9 a9 = f9_unpack(t[0]), b9 = f9_unpack(t[1]), c9 = f9_unpack(t[2]), d9 = f9_unpack(t[3]);
        const F9 eh = f9_mul(f9_sub(a9, b9), f9_add(c9, d9));                                              // the E * H, G * H shapes
        ECHECK(f9_reduced(eh) && fp_eq(f9_pack(eh), fp_mul(fp_sub(t[0], t[1]), fp_add(t[2], t[3]))), "(a-b)(c+d)");
        const F9 fg = f9_mul(f9_carry(f9_sub(f9_add(a9, a9), b9)), f9_add(f9_add(c9, c9), d9));            // the normalised F times G
        ECHECK(f9_reduced(fg) && fp_eq(f9_pack(fg), fp_mul(fp_sub(fp_add(t[0], t[0]), t[1]), fp_add(fp_add(t[2], t[2]), t[3]))), "carry(2a-b)(2c+d)");
        const F9 cr = f9_carry(f9_add(f9_sub(a9, b9), f9_add(c9, d9)));
        ECHECK(f9_reduced(cr) && fp_eq(f9_pack(cr), fp_add(fp_sub(t[0], t[1]), fp_add(t[2], t[3]))), "carry((a-b)+(c+d))");
        Pt P; P.X = t[0]; P.Y = t[1]; P.Z = t[2]; P.T = t[3];
        Niels nl; nl.yplusx = t[4]; nl.yminusx = t[5]; nl.xy2d = t[6];
        for (int neg = 0; neg < 2; neg++) {
            N9 e = n9_unpack(nl); if (neg) e = n9_negate(e);
            const P9 q1 = p9_madd(p9_unpack(P), e), q2 = p9_madd(q1, e);
            const Pt w1 = neg ? pt_msub(P, nl) : pt_madd(P, nl), w2 = neg ? pt_msub(w1, nl) : pt_madd(w1, nl);
            ECHECK(p9_reduced(q1) && p9_reduced(q2), "p9_madd output bound");
            ECHECK(pt_same(p9_pack(q1), w1) && pt_same(p9_pack(q2), w2), "p9_madd");
        }
    }
#undef ECHECK
    return bad;
}
// ---- fr9_canon above 2^261.  A thread of a round kernel that walks 64 items ends with accumulators of several hundred l (limb 8 beyond 29 bits);
// fr9_canon takes q = limb 8 >> 20 and stays exact while that limb fits its 32 bits: any normalised value below 2^264.
// The reference: the limbs' value mod l by Horner over field.h's additions (29 doublings per limb; a limb is a canonical word as it stands).
static Fr fr9_value_ref(const Fr9 &a) {
    Fr acc = fr_zero();
    for (int i = 8; i >= 0; i--) {
        for (int s = 0; s < 29; s++) acc = fr_add(acc, acc);
        Fr limb = fr_zero(); limb.v[0] = a.v[i];
        acc = fr_add(acc, limb);
    }
    return acc;
}
static int wide_sum_checks() {
    int bad = 0;
#define WCHECK(cond, what) do { if (!(cond)) { if (bad < 10) printf("FAIL wide sums: %s\n", what); bad++; } } while (0)
    // running sums kept as the kernels keep them: normalised items (a product's output form) added without reduction, one carry sweep every fourth item,
    // fr9_canon(fr9_norm(.)) at the end.  An item is 32 (x + y) < 64 l, so at most 63 of them stay below 4032 l < 2^264; every sum must END in [2^261, 2^264).
    for (int it = 0; it < 600; it++) {
        const bool top = it % 4 == 0;                                    // every item at its largest: x = y = l - 1
        const int count = top ? 9 + it / 4 % 55 : 40 + it % 24;         // 9 .. 63 items of 64 (l - 1): 576 l .. 4032 l; 40 .. 63 random ones: about 32 l each
        Fr9 acc = fr9_zero(); Fr want = fr_zero();
        for (int k = 0; k < count; k++) {
            const Fr x = top ? l_minus(1) : rnd_fr(), y = top ? l_minus(1) : rnd_fr();
            const Fr9 item = fr9_norm(fr9_add(fr9_unpack5(x), fr9_unpack5(y)));
            acc = fr9_add(acc, item); want = fr_add(want, fr9_value_ref(item));
            if ((k & 3) == 3) acc = fr9_norm(acc);
        }
        const Fr9 end = fr9_norm(acc);
        const uint32_t q = end.v[8] >> 20;
        WCHECK(q >= 512, "a running sum ended below 2^261");            // (limb 8 is 32 bits: below 2^264 by the count above)
        WCHECK(fr_eq(fr9_value_ref(end), want), "the reference disagrees with itself");
        WCHECK(fr_eq(fr9_canon(end), want), "fr9_canon of a running sum between 2^261 and 2^264");
    }
    // the ends of the range, limb by limb: limb 8 around 2^29 (q = 511, 512), at every bit above it and at 2^32 - 1 (q = 4095), over low limbs of all ones,
    // all zeros and random bits
    const uint32_t tops[] = {0x1fffffffu, 0x20000000u, 0x200fffffu, 0x3fffffffu, 0x40000000u, 0x7fffffffu, 0x80000000u, 0xfff00000u, 0xffefffffu, 0xffffffffu};
    for (uint32_t t8 : tops)
        for (int low = 0; low < 6; low++) {
            Fr9 a;
            for (int i = 0; i < 8; i++) a.v[i] = low == 0 ? FR9_M : low == 1 ? 0u : ((uint32_t)rng() & FR9_M);
            a.v[8] = t8;
            WCHECK(fr_eq(fr9_canon(a), fr9_value_ref(a)), "fr9_canon at an end of its range");
        }
#undef WCHECK
    return bad;
}
// ---- the case file of tests/scalar_cases.py (write_case_file): per line an operation of otti_k_fr9_op, its operands and the word and / or limbs the
// plain-integer reference expects; the plain-C bodies of fr9.h must return exactly those.  The pool is stated once, in scalar_cases.py.
static bool read_u32s(FILE *f, uint32_t *p, int n) { for (int i = 0; i < n; i++) if (fscanf(f, "%x", &p[i]) != 1) return false; return true; }
static Fr9 fold9_host(const Fr &x0, const Fr &x2, const Fr9 &r5, Fr &word) {      // fold9 of kernels_common.h (a device-only header), as test "fold" above
    const Fr9 a = fr9_unpack(x0);
    const Fr9 s = fr9_norm(fr9_add(a, fr9_mul(r5, fr9_sub_kl<2>(fr9_unpack(x2), a))));
    word = fr9_pack_lt3l(s);
    return s;
}
static int scalar_case_file(const char *path) {
    static const char *names[] = {"unpack", "unpack5", "unpack10", "mul", "mul_self", "add", "norm", "sub_kl2", "sub_kl4", "sub_kl8", "sub_kl16", "sub_kl128",
                                  "fold_top", "shl5", "pack_lt2l", "pack_lt3l", "canon", "mul9", "fold9"};
    enum { UNPACK, UNPACK5, UNPACK10, MUL, MUL_SELF, ADD, NORM, SUB2, SUB4, SUB8, SUB16, SUB128, FOLD_TOP, SHL5, PACK2, PACK3, CANON, MUL9, FOLD9, NOPS };
    FILE *f = fopen(path, "r");
    if (!f) { printf("FAIL case file: cannot open %s\n", path); return 1; }
    int bad = 0; long line = 0, per_op[NOPS] = {0}; char name[32];
    while (fscanf(f, "%31s", name) == 1) {
        line++;
        int op = 0; while (op < NOPS && strcmp(name, names[op])) op++;
        if (op == NOPS) { printf("FAIL case file: unknown operation %s at line %ld\n", name, line); bad++; break; }
        const int nw = op <= UNPACK10 ? 1 : op == MUL9 ? 2 : op == FOLD9 ? 3 : 0;
        const int nl = nw ? 0 : (op == MUL || op == ADD || (op >= SUB2 && op <= SUB128)) ? 2 : 1;
        const bool has_word = op >= PACK2, has_limbs = op < PACK2 || op >= MUL9;
        Fr w[3], want_w = fr_zero(), got_w = fr_zero(); Fr9 x[2], want_l = fr9_zero(), got_l = fr9_zero();
        bool ok = true;
        for (int k = 0; k < nw; k++) ok = ok && read_u32s(f, w[k].v, 8);
        for (int k = 0; k < nl; k++) ok = ok && read_u32s(f, x[k].v, 9);
        if (has_word) ok = ok && read_u32s(f, want_w.v, 8);
        if (has_limbs) ok = ok && read_u32s(f, want_l.v, 9);
        if (!ok) { printf("FAIL case file: short line %ld (%s)\n", line, name); bad++; break; }
        switch (op) {
        case UNPACK: got_l = fr9_unpack(w[0]); break;
        case UNPACK5: got_l = fr9_unpack5(w[0]); break;
        case UNPACK10: got_l = fr9_unpack_s<10>(w[0]); break;
        case MUL: got_l = fr9_mul(x[0], x[1]); break;
        case MUL_SELF: got_l = fr9_mul(x[0], x[0]); break;
        case ADD: got_l = fr9_add(x[0], x[1]); break;
        case NORM: got_l = fr9_norm(x[0]); break;
        case SUB2: got_l = fr9_sub_kl<2>(x[0], x[1]); break;
        case SUB4: got_l = fr9_sub_kl<4>(x[0], x[1]); break;
        case SUB8: got_l = fr9_sub_kl<8>(x[0], x[1]); break;
        case SUB16: got_l = fr9_sub_kl<16>(x[0], x[1]); break;
        case SUB128: got_l = fr9_sub_kl<128>(x[0], x[1]); break;
        case FOLD_TOP: got_l = fr9_fold_top(x[0]); break;
        case SHL5: got_l = fr9_shl5(x[0]); break;
        case PACK2: got_w = fr9_pack_lt2l(x[0]); break;
        case PACK3: got_w = fr9_pack_lt3l(x[0]); break;
        case CANON: got_w = fr9_canon(x[0]); break;
        case MUL9: got_l = fr9_mul(fr9_unpack5(w[0]), fr9_unpack(w[1])); got_w = fr9_pack_lt2l(got_l); break;
        default: got_l = fold9_host(w[0], w[1], fr9_unpack5(w[2]), got_w); break;
        }
        bool same = fr_eq(got_w, want_w);
        for (int i = 0; i < 9; i++) same = same && got_l.v[i] == want_l.v[i];
        if (!same) { if (bad < 10) printf("FAIL case file: %s, case %ld of the operation (line %ld)\n", name, per_op[op], line); bad++; }
        per_op[op]++;
    }
    fclose(f);
    for (int op = 0; op < NOPS; op++) if (!per_op[op] && !bad) { printf("FAIL case file: no case of %s\n", names[op]); bad++; }
    printf("case file: %ld cases\n", line);
    return bad;
}
#define CHECK(cond, what) do { if (!(cond)) { if (bad < 10) printf("FAIL %s at iteration %d\n", what, it); bad++; } } while (0)
int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 20000;
    int bad = argc > 2 ? scalar_case_file(argv[2]) : 0;
    for (int it = 0; it < iters; it++) {
        Fr a = rnd_fr(), b = rnd_fr(), c = rnd_fr();
        if (it == 0) a = fr_zero();
        if (it == 1) { a = l_minus(1); b = a; c = a; }
        if (it == 2) { a = fr_one(); b = l_minus(1); }
        const Fr9 a9 = fr9_unpack(a), b9 = fr9_unpack(b), c5 = fr9_unpack5(c);
        // products, the radix correction on either operand, computed operands shifted afterwards
        const Fr9 p = fr9_mul(fr9_unpack5(a), b9);
        const Fr ab = fr_mul(a, b);
        CHECK(fr_eq(fr9_pack_lt2l(p), ab), "mul");
        CHECK(fr_eq(fr9_pack_lt2l(fr9_mul(fr9_shl5(p), fr9_unpack(c))), fr_mul(ab, c)), "shl5");
        CHECK(fr_eq(fr9_canon(fr9_mul(fr9_unpack_s<10>(a), fr9_mul(b9, fr9_unpack(c)))), fr_mul(a, fr_mul(b, c))), "unpack_s<10>");
        // differences with offsets, folds
        CHECK(fr_eq(fr9_canon(fr9_norm(fr9_sub_kl<2>(a9, b9))), fr_sub(a, b)), "sub 2l");
        CHECK(fr_eq(fr9_canon(fr9_norm(fr9_sub_kl<4>(a9, b9))), fr_sub(a, b)), "sub 4l");
        CHECK(fr_eq(fr9_canon(fr9_norm(fr9_sub_kl<16>(a9, b9))), fr_sub(a, b)), "sub 16l");
        CHECK(fr_eq(fr9_canon(fr9_norm(fr9_sub_kl<128>(fr9_unpack5(a), fr9_unpack5(b)))), fr_mul(fr_sub(a, b), fr_from_u64(32))), "sub 128l");
        const Fr9 f = fr9_norm(fr9_add(a9, fr9_mul(c5, fr9_sub_kl<2>(b9, a9))));
        CHECK(fr_eq(fr9_pack_lt3l(f), fr_add(a, fr_mul(c, fr_sub(b, a)))), "fold");
        // running sums carried down every fourth item, any normalised value back to the canonical word
        if (it % 16 == 0) {
            Fr9 acc = fr9_zero(); Fr want = fr_zero();
            for (int k = 0; k < 70; k++) { const Fr x = rnd_fr(); acc = fr9_add(acc, fr9_mul(c5, fr9_sub_kl<16>(fr9_unpack(x), a9))); want = fr_add(want, fr_mul(c, fr_sub(x, a))); if ((k & 3) == 3) acc = fr9_norm(acc); }
            CHECK(fr_eq(fr9_canon(fr9_norm(acc)), want), "accumulate");
        }
        // GF(2^255 - 19)
        const Fp x = it == 3 ? fp_from_words(~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u) : rnd_fp(), y = rnd_fp();
        CHECK(fp_eq(f9_pack(f9_mul(f9_unpack(x), f9_unpack(y))), fp_mul(x, y)), "f9_mul");
        CHECK(fp_eq(f9_pack(f9_sub(f9_unpack(x), f9_unpack(y))), fp_sub(x, y)), "f9_sub");
        CHECK(fp_eq(f9_pack(f9_add(f9_unpack(x), f9_unpack(y))), fp_add(x, y)), "f9_add");
    }
    // a walk of mixed additions / subtractions against pt_madd / pt_msub (the formulas are polynomial identities: any field elements serve as operands)
    Pt P; P.X = rnd_fp(); P.Y = rnd_fp(); P.Z = rnd_fp(); P.T = rnd_fp();
    P9 Q = p9_unpack(P);
    for (int it = 0; it < iters; it++) {
        Niels n; n.yplusx = rnd_fp(); n.yminusx = rnd_fp(); n.xy2d = rnd_fp();
        const bool neg = rng() & 1;
        N9 e = n9_unpack(n); if (neg) e = n9_negate(e);
        Q = p9_madd(Q, e); P = neg ? pt_msub(P, n) : pt_madd(P, n);
        for (int i = 0; i < 8; i++) CHECK(Q.X.v[i] < (1u << 29) + (1u << 18) && Q.Y.v[i] < (1u << 29) + (1u << 18) && Q.Z.v[i] < (1u << 29) + (1u << 18) && Q.T.v[i] < (1u << 29) + (1u << 18), "reduced bound");
        if (it % 61 == 0 || it < 40) { const Pt q = p9_pack(Q); CHECK(fp_eq(q.X, P.X) && fp_eq(q.Y, P.Y) && fp_eq(q.Z, P.Z) && fp_eq(q.T, P.T), "p9_madd"); }
    }
    bad += edge_pool_checks();
    bad += wide_sum_checks();
    printf("limb9 check: %d failures\n", bad);
    return bad != 0;
}
