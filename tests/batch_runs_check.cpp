// Product-form runs in the verifiers' term lists (otti_amd/csrc/batch_terms.h, spartan_host.cpp dotproductlog_verify) on the host alone: own main,
// the host sources linked beside it.  A generator is modelled by its discrete logarithm, as tests/verify_batch_check.cpp models points, so a list
// with runs can be held against the same list with every generator term written out.
// Built and run by tests/test_batch_runs_host.py, plain and under the address + undefined-behaviour sanitizers.
#include "../otti_amd/csrc/verify.h"
#include <cstdio>

using namespace otti;

extern "C" void otti_r1cs_free(otti_r1cs *r) { if (!r) return; free(r->A); free(r->B); free(r->C); free(r->vars32); free(r->inputs32); free(r); }   // zkif.cpp's, unused here

static int g_failures = 0;
#define CHECK(x) do { if (!(x)) { g_failures++; fprintf(stderr, "batch_runs_check: line %d: %s\n", __LINE__, #x); } } while (0)

static uint64_t g_rng = 0x13198a2e03707344ULL;
static uint64_t rnd() { g_rng += 0x9e3779b97f4a7c15ULL; uint64_t z = g_rng; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); }
static Fr rnd_fr() { uint8_t w[64]; for (int i = 0; i < 8; i++) { const uint64_t x = rnd(); memcpy(w + 8 * i, &x, 8); } return fr_from_bytes_wide(w); }
static CPoint rnd_bytes() { CPoint c; for (int i = 0; i < 4; i++) { const uint64_t x = rnd(); memcpy(c.b + 8 * i, &x, 8); } return c; }

// the definition: the doubling recurrence of dotproductlog_verify over the squared challenges ch2, s[0] = allinv
static std::vector<Fr> recurrence(const std::vector<Fr> &ch2, const Fr &allinv) {
    const size_t lg = ch2.size(), n = (size_t)1 << lg;
    std::vector<Fr> s(n); s[0] = allinv;
    for (size_t i = 1; i < n; i++) { size_t lg_i = ilog2(i + 1) - 1; size_t k = (size_t)1 << lg_i; s[i] = fr_mul(s[i - k], ch2[(lg - 1) - lg_i]); }
    return s;
}
static BtRun run_of(const std::vector<Fr> &ch2, const Fr &c) { BtRun r; r.c = c; const size_t lg = ch2.size(); r.f.resize(lg); for (size_t t = 0; t < lg; t++) r.f[t] = ch2[lg - 1 - t]; return r; }

constexpr size_t kGens = 80;
static Fr g_dlog_gen[kGens];
static Fr over_gens(const std::vector<Fr> &s) { Fr acc = fr_zero(); for (size_t i = 0; i < s.size(); i++) acc = fr_add(acc, fr_mul(s[i], g_dlog_gen[i])); return acc; }

int main() {
    for (size_t q = 0; q < kGens; q++) g_dlog_gen[q] = rnd_fr();
    int cases = 0;

    // ---- bt_run_expand equals the recurrence, lg = 0 .. 13; it ADDS to what is there
    for (size_t lg = 0; lg <= 13; lg++) {
        std::vector<Fr> ch2(lg); for (auto &x : ch2) x = rnd_fr();
        const Fr allinv = rnd_fr(), mz1 = rnd_fr(), c = fr_mul(mz1, allinv);
        const std::vector<Fr> s = recurrence(ch2, allinv);
        const BtRun r = run_of(ch2, c);
        CHECK(r.lg() == lg && r.slots() == s.size());
        std::vector<Fr> out(s.size() + 3), before;
        for (auto &x : out) x = rnd_fr();
        before = out;
        bt_run_expand(r, out.data());
        bool same = true;
        for (size_t i = 0; i < s.size(); i++) same &= fr_eq(out[i], fr_add(before[i], fr_mul(mz1, s[i])));
        for (size_t i = s.size(); i < out.size(); i++) same &= fr_eq(out[i], before[i]);          // nothing past 2^lg
        CHECK(same);
        cases++;
    }
    // ---- bt_weigh with runs equals bt_weigh over the written-out terms (generators by their discrete logarithms)
    for (int round = 0; round < 12; round++) {
        BtEquations with, without; with.accept_runs = true;
        const size_t ne = 1 + rnd() % 6;
        for (size_t k = 0; k < ne; k++) {
            for (size_t i = 0, m = rnd() % 4; i < m; i++) { const uint32_t q = (uint32_t)(rnd() % kGens); const Fr s = rnd_fr(); with.gen(s, q); without.gen(s, q); }
            for (size_t j = 0, m = rnd() % 3; j < m; j++) {                                      // up to two runs of different lg in one equation
                const size_t lg = rnd() % 7;
                std::vector<Fr> ch2(lg); for (auto &x : ch2) x = rnd_fr();
                const Fr c = (rnd() % 5 == 0) ? fr_zero() : rnd_fr();
                if (lg && rnd() % 4 == 0) ch2[rnd() % lg] = fr_zero();
                const BtRun r = run_of(ch2, c);
                with.run(r.c, r.f.data(), r.lg());
                const std::vector<Fr> s = recurrence(ch2, c);
                for (size_t i = 0; i < s.size(); i++) without.gen(s[i], (uint32_t)i);
            }
            with.close(); without.close();
        }
        CHECK(with.count() == ne && without.count() == ne);
        std::vector<Fr> w(ne); for (auto &x : w) x = rnd_fr();
        BtWeighted A, B;
        CHECK(bt_weigh(with, w.data(), kGens, A) && bt_weigh(without, w.data(), kGens, B));
        CHECK(A.runs.size() == with.runs.size() && B.runs.empty());
        std::vector<Fr> total = A.gen_s;
        for (const BtRun &r : A.runs) bt_run_expand(r, total.data());
        bool same = true;
        for (size_t i = 0; i < kGens; i++) same &= fr_eq(total[i], B.gen_s[i]);
        CHECK(same);
        CHECK(fr_eq(over_gens(total), over_gens(B.gen_s)));
        for (size_t i = 0; i < A.runs.size(); i++) { bool f = true; for (size_t t = 0; t < A.runs[i].lg(); t++) f &= fr_eq(A.runs[i].f[t], with.runs[i].f[t]); CHECK(f); }   // factors left alone
        cases++;
    }
    {   // a run that reaches past the generators is refused
        BtEquations E; std::vector<Fr> f(7, fr_one()); E.run(fr_one(), f.data(), 7); E.close();
        const Fr w = fr_one(); BtWeighted W;
        CHECK(!bt_weigh(E, &w, kGens, W) && bt_weigh(E, &w, 128, W));
        cases++;
    }
    // ---- the closed-form a_hat equals the direct sum: random points, and coordinates 0, 1 and l - 1
    for (size_t lg = 0; lg <= 11; lg++)
        for (int kind = 0; kind < 4; kind++) {
            std::vector<Fr> r(lg), ch2(lg);
            const Fr special[3] = {fr_zero(), fr_one(), fr_neg(fr_one())};
            for (size_t j = 0; j < lg; j++) { ch2[j] = rnd_fr(); r[j] = kind == 0 ? rnd_fr() : kind == 3 ? (rnd() % 2 ? rnd_fr() : special[rnd() % 3]) : special[(j + kind) % 3]; }
            const Fr allinv = rnd_fr();
            const std::vector<Fr> a = eq_evals_host(r.data(), lg), s = recurrence(ch2, allinv);
            Fr direct = fr_zero(); for (size_t i = 0; i < a.size(); i++) direct = fr_add(direct, fr_mul(a[i], s[i]));
            CHECK(fr_eq(direct, dotproductlog_a_hat(r.data(), ch2.data(), lg, allinv)));
            cases++;
        }
    // ---- dotproductlog_verify itself: a sink without accept_runs gets today's list; one with it gets the same equation with ONE run
    for (size_t lg = 0; lg <= 9; lg++) {
        const size_t n = (size_t)1 << lg;
        Gens g; g.P.assign(n + 2, pt_identity());
        const PcView v = {(uint32_t)(n + 1), (uint32_t)n, (uint32_t)(n + 1), n};
        DotProductProofLog pf; pf.L_vec.resize(lg); pf.R_vec.resize(lg);
        for (size_t i = 0; i < lg; i++) { pf.L_vec[i] = rnd_bytes(); pf.R_vec[i] = rnd_bytes(); }
        pf.delta = rnd_bytes(); pf.beta = rnd_bytes(); pf.z1 = rnd_fr(); pf.z2 = rnd_fr();
        const CPoint Cx = rnd_bytes(), Cy = rnd_bytes();
        std::vector<Fr> r(lg); for (auto &x : r) x = rnd_fr();
        const std::vector<Fr> a = eq_evals_host(r.data(), lg);
        BtEquations plain, plain_pt, runs, runs_nopt; runs.accept_runs = runs_nopt.accept_runs = true;
        BtEquations *sinks[4] = {&plain, &plain_pt, &runs, &runs_nopt};
        for (int k = 0; k < 4; k++) {
            Transcript tr("runs", 4); Deferred later(sinks[k]);
            dotproductlog_verify(pf, n, g, v, tr, a.data(), Cx, Cy, &later, (k == 1 || k == 2) ? r.data() : nullptr);
            later.finish();
        }
        CHECK(plain.count() == 1 && plain.terms.size() == 2 * lg + 6 + n && plain.runs.empty());        // today's term count exactly
        CHECK(plain_pt.terms.size() == plain.terms.size() && plain_pt.runs.empty());                     // the point alone changes nothing
        bool same = true;
        for (size_t i = 0; i < plain.terms.size(); i++) same &= fr_eq(plain.terms[i].s, plain_pt.terms[i].s) && plain.terms[i].gen == plain_pt.terms[i].gen && plain.terms[i].key == plain_pt.terms[i].key;
        CHECK(same);
        for (BtEquations *R : {&runs, &runs_nopt}) {
            CHECK(R->count() == 1 && R->terms.size() == 2 * lg + 6 && R->runs.size() == 1 && R->runs[0].eq == 0 && R->runs[0].lg() == lg);
            // the point terms and G_1, h_1 are the same terms (a_hat sits in most of their scalars); the run expands to the n generator terms
            same = true;
            for (size_t i = 0; i < 2 * lg + 4; i++) same &= fr_eq(R->terms[i].s, plain.terms[i].s) && R->terms[i].key == plain.terms[i].key && R->terms[i].gen < 0;
            for (size_t i = 0; i < 2; i++) { const BtTerm &x = R->terms[2 * lg + 4 + i], &y = plain.terms[2 * lg + 4 + n + i]; same &= fr_eq(x.s, y.s) && x.gen == y.gen && x.gen >= (int32_t)n; }
            std::vector<Fr> out(n, fr_zero()); bt_run_expand(R->runs[0], out.data());
            for (size_t i = 0; i < n; i++) { const BtTerm &y = plain.terms[2 * lg + 4 + i]; same &= y.gen == (int32_t)i && fr_eq(out[i], y.s); }
            CHECK(same);
        }
        cases++;
    }
    printf("batch_runs_check: %d cases, %d failures\n", cases, g_failures);
    return g_failures ? 1 : 0;
}
