// batch_terms.h (otti_amd/csrc) on the host alone: own main, the field type and the standard library, nothing linked beside it.  A point is modelled
// by its discrete logarithm — point number q stands for d(q) * B with d(q) a scalar this program knows — so "the sum is the identity" becomes
// "sum of s_j d_j is zero" and every claim about the merged form can be held against the long form, term by term.
// Built and run by tests/test_verify_batch_terms_host.py, plain and under the address + undefined-behaviour sanitizers.
#include "../otti_amd/csrc/batch_terms.h"
#include <cstdio>

using namespace otti;

static int g_failures = 0;
#define CHECK(x) do { if (!(x)) { g_failures++; fprintf(stderr, "verify_batch_check: line %d: %s\n", __LINE__, #x); } } while (0)

static uint64_t g_rng = 0x243f6a8885a308d3ULL;
static uint64_t rnd() { g_rng += 0x9e3779b97f4a7c15ULL; uint64_t z = g_rng; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); }
static Fr rnd_fr() { uint8_t w[64]; for (int i = 0; i < 8; i++) { const uint64_t x = rnd(); memcpy(w + 8 * i, &x, 8); } return fr_from_bytes_wide(w); }

constexpr size_t kPoints = 24, kGens = 12;
static Fr g_dlog_point[kPoints], g_dlog_gen[kGens];
static BtKey key_of(size_t q) { BtKey k; k.fill(0); k[0] = (uint8_t)(2 * q); k[9] = (uint8_t)(q * 37 + 1); k[31] = (uint8_t)q; return k; }
static size_t point_of(const BtKey &k) { return k[31]; }

// the long form: sum over the equations of w_k * sum of its terms, nothing merged
static Fr long_form(const BtEquations &E, const Fr *w) {
    Fr acc = fr_zero();
    for (size_t k = 0; k < E.count(); k++)
        for (uint32_t i = E.eq[k]; i < E.eq[k + 1]; i++) {
            const BtTerm &t = E.terms[i];
            const Fr d = t.gen >= 0 ? g_dlog_gen[t.gen] : g_dlog_point[point_of(t.key)];
            acc = fr_add(acc, fr_mul(w[k], fr_mul(t.s, d)));
        }
    return acc;
}
static Fr merged_points(const BtWeighted &W) { Fr acc = fr_zero(); for (size_t i = 0; i < W.keys.size(); i++) acc = fr_add(acc, fr_mul(W.point_s[i], g_dlog_point[point_of(W.keys[i])])); return acc; }
static Fr over_gens(const std::vector<Fr> &s) { Fr acc = fr_zero(); for (size_t i = 0; i < s.size(); i++) acc = fr_add(acc, fr_mul(s[i], g_dlog_gen[i])); return acc; }

// an equation that HOLDS over random points and generators: the last term, on point `fix`, makes up for the rest; err is added to its scalar's effect
static void add_equation(BtEquations &E, size_t npts, size_t ngens, size_t fix, const Fr &err_dlog) {
    Fr acc = fr_zero();
    for (size_t i = 0; i < npts; i++) { const size_t q = rnd() % kPoints; const Fr s = rnd_fr(); E.point(s, key_of(q).data()); acc = fr_add(acc, fr_mul(s, g_dlog_point[q])); }
    for (size_t i = 0; i < ngens; i++) { const uint32_t q = (uint32_t)(rnd() % kGens); const Fr s = rnd_fr(); E.gen(s, q); acc = fr_add(acc, fr_mul(s, g_dlog_gen[q])); }
    // -acc / d(fix) on point fix closes the equation; an error of err_dlog * B is one more term on the point whose logarithm is 1 (point 0)
    E.point(fr_mul(fr_neg(acc), fr_inv(g_dlog_point[fix])), key_of(fix).data());
    if (!fr_is_zero(err_dlog)) E.point(err_dlog, key_of(0).data());
    E.close();
}

int main() {
    g_dlog_point[0] = fr_one();
    for (size_t q = 1; q < kPoints; q++) g_dlog_point[q] = rnd_fr();
    for (size_t q = 0; q < kGens; q++) g_dlog_gen[q] = rnd_fr();
    int cases = 0;

    {   // the empty list
        BtEquations E; BtWeighted W;
        CHECK(E.count() == 0 && bt_weigh(E, nullptr, kGens, W));
        CHECK(W.keys.empty() && W.point_s.empty() && W.gen_s.size() == kGens);
        for (size_t i = 0; i < kGens; i++) CHECK(fr_is_zero(W.gen_s[i]) && !W.gen_used[i]);
        std::vector<Fr> total; std::vector<uint8_t> used;
        CHECK(bt_fold_gens(total, used, W) == 0 && total.size() == kGens);
        cases++;
    }
    {   // one equation, repeated points merged: 3 a P5 + 4 b P5 + c P7 under weight w -> two points, w (3 a + 4 b) and w c
        BtEquations E; const Fr a = rnd_fr(), b = rnd_fr(), c = rnd_fr(), w = rnd_fr();
        E.point(a, key_of(5).data()); E.point(b, key_of(5).data()); E.point(c, key_of(7).data()); E.gen(a, 3); E.gen(b, 3); E.close();
        BtWeighted W;
        CHECK(bt_weigh(E, &w, kGens, W));
        CHECK(W.keys.size() == 2 && W.keys[0] == key_of(5) && W.keys[1] == key_of(7));
        CHECK(fr_eq(W.point_s[0], fr_mul(w, fr_add(a, b))) && fr_eq(W.point_s[1], fr_mul(w, c)));
        CHECK(fr_eq(W.gen_s[3], fr_mul(w, fr_add(a, b))) && W.gen_used[3] && !W.gen_used[2]);
        CHECK(fr_eq(fr_add(merged_points(W), over_gens(W.gen_s)), long_form(E, &w)));
        CHECK(!bt_weigh(E, &w, 3, W));                                       // slot 3 of 3 generators: refused
        cases++;
    }
    {   // many equations over few points: merged form == long form, and valid equations sum to zero under any weights
        for (int round = 0; round < 20; round++) {
            BtEquations E;
            const size_t ne = 1 + rnd() % 40;
            for (size_t k = 0; k < ne; k++) add_equation(E, rnd() % 6, rnd() % 5, 1 + rnd() % (kPoints - 1), fr_zero());
            std::vector<Fr> w(ne); for (auto &x : w) x = rnd_fr();
            BtWeighted W;
            CHECK(bt_weigh(E, w.data(), kGens, W));
            CHECK(W.keys.size() <= kPoints);
            for (size_t i = 0; i < W.keys.size(); i++) for (size_t j = 0; j < i; j++) CHECK(!(W.keys[i] == W.keys[j]));
            const Fr merged = fr_add(merged_points(W), over_gens(W.gen_s));
            CHECK(fr_eq(merged, long_form(E, w.data())));
            CHECK(fr_is_zero(merged));
            cases++;
        }
    }
    {   // generator folding over several proofs against the long form
        std::vector<Fr> total; std::vector<uint8_t> used; Fr want = fr_zero(); size_t slots = 0;
        std::vector<uint8_t> want_used(kGens, 0);
        for (int proof = 0; proof < 7; proof++) {
            BtEquations E;
            const size_t ne = 1 + rnd() % 9;
            for (size_t k = 0; k < ne; k++) add_equation(E, 2, 1 + rnd() % 4, 1 + rnd() % (kPoints - 1), fr_zero());
            std::vector<Fr> w(ne); for (auto &x : w) x = rnd_fr();
            BtWeighted W;
            CHECK(bt_weigh(E, w.data(), kGens, W));
            for (size_t k = 0; k < ne; k++) for (uint32_t i = E.eq[k]; i < E.eq[k + 1]; i++) if (E.terms[i].gen >= 0) { want = fr_add(want, fr_mul(w[k], fr_mul(E.terms[i].s, g_dlog_gen[E.terms[i].gen]))); want_used[E.terms[i].gen] = 1; }
            slots = bt_fold_gens(total, used, W);
        }
        size_t n_used = 0; for (uint8_t u : want_used) n_used += u;
        CHECK(total.size() == kGens && slots == n_used && fr_eq(over_gens(total), want));
        cases++;
    }
    {   // two equations whose errors are +T and -T: independent weights see them, equal weights do not — which is why every equation has its own
        for (int round = 0; round < 10; round++) {
            BtEquations E; const Fr T = rnd_fr();
            add_equation(E, 3, 2, 1 + rnd() % (kPoints - 1), T);
            add_equation(E, 4, 1, 1 + rnd() % (kPoints - 1), fr_neg(T));
            BtWeighted W;
            Fr w[2] = {rnd_fr(), rnd_fr()};
            CHECK(bt_weigh(E, w, kGens, W));
            CHECK(!fr_is_zero(fr_add(merged_points(W), over_gens(W.gen_s))));
            w[1] = w[0];
            CHECK(bt_weigh(E, w, kGens, W));
            CHECK(fr_is_zero(fr_add(merged_points(W), over_gens(W.gen_s))));      // the test can tell the difference
            cases++;
        }
    }
    printf("verify_batch_check: %d cases, %d failures\n", cases, g_failures);
    return g_failures ? 1 : 0;
}
