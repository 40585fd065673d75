// term_sum (otti_amd/csrc/verify.h): the one evaluator every deferred group equation of the verifiers runs through, held to an independent
// computation — host_scalarmul of each decoded point, added with pt_add — and the five sites that state their equations as term lists
// (knowledge, equality, product, the dot-product pair of a sum-check round, the closing equation of the log dot-product proof), each with a
// proof it must accept and with every scalar and every point of that proof replaced once, which it must refuse.  Own main, host sources only;
// built by tests/test_term_sum_host.py plain and with -fsanitize=address,undefined and run directly.
#include "../otti_amd/csrc/spartan.h"
#include "../otti_amd/csrc/verify.h"
#include <stdio.h>
#include <functional>
#include <vector>

using namespace otti;
extern "C" void otti_r1cs_free(otti_r1cs *r) { if (!r) return; free(r->A); free(r->B); free(r->C); free(r->vars32); free(r->inputs32); free(r); }   // the C ABI's, for zkif.cpp

static int g_cases = 0, g_failures = 0;
static void check(bool ok, const char *what, size_t k = 0) { g_cases++; if (!ok) { g_failures++; fprintf(stderr, "FAIL: %s (%zu)\n", what, k); } }

static uint64_t g_rng = 0x243f6a8885a308d3ULL;
static uint64_t rnd() { g_rng += 0x9e3779b97f4a7c15ULL; uint64_t z = g_rng; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); }
static Fr rnd_fr() { uint8_t w[64]; for (int i = 0; i < 8; i++) { const uint64_t x = rnd(); memcpy(w + 8 * i, &x, 8); } return fr_from_bytes_wide(w); }
static CPoint enc(const Pt &p) { CPoint c; pt_encode(c.b, p); return c; }
static std::unique_ptr<Gens> G;
static Pt rnd_pt() { return host_scalarmul(G->P[0], rnd_fr()); }
static Fr dot(const Fr *a, const Fr *b, size_t n) { Fr s = fr_zero(); for (size_t i = 0; i < n; i++) s = fr_add(s, fr_mul(a[i], b[i])); return s; }

// ------------------------------------------------------------------------------------------------ the evaluator against term-by-term sums
static Pt naive(const std::vector<BtTerm> &t) {
    Pt acc = pt_identity();
    for (const BtTerm &x : t) {
        Pt p;
        if (x.gen >= 0) p = G->P[x.gen]; else if (!pt_decode_fast(p, x.key.data())) { fprintf(stderr, "the check's own point does not decode\n"); exit(2); }
        acc = pt_add(acc, host_scalarmul(p, x.s));
    }
    return acc;
}
static void agrees(const std::vector<BtTerm> &t, const char *what, size_t k = 0) { check(pt_eq(term_sum(t.data(), t.size(), *G), naive(t)), what, k); }
static int code_of(const std::vector<BtTerm> &t) { try { (void)term_sum(t.data(), t.size(), *G); return 0; } catch (const VerifyFail &f) { return f.code; } }
static std::vector<BtTerm> rnd_terms(size_t n) { std::vector<BtTerm> t; for (size_t i = 0; i < n; i++) t.push_back(term(rnd_fr(), enc(rnd_pt()))); return t; }

static void evaluator_cases() {
    for (size_t n : {1, 2, 7, 23, 24, 40}) agrees(rnd_terms(n), "random terms", n);      // 23 | 24: host_msm's Straus / bucket cut-over
    const Fr special[3] = {fr_zero(), fr_one(), fr_neg(fr_one())};                      // 0, 1, l - 1
    for (int k = 0; k < 3; k++) {
        std::vector<BtTerm> t = rnd_terms(3); t[1].s = special[k];
        const std::vector<BtTerm> alone = {term(special[k], enc(rnd_pt()))};
        check(pt_eq(term_sum(t.data(), 3, *G), naive(t)) && pt_eq(term_sum(alone.data(), 1, *G), naive(alone)), "scalar 0 / 1 / l - 1", k);
    }
    { std::vector<BtTerm> t = rnd_terms(4); t[3].key = t[0].key; agrees(t, "one encoding named twice"); }
    { std::vector<BtTerm> t = rnd_terms(3); t[1] = term(rnd_fr(), enc(pt_identity())); agrees(t, "the identity's encoding"); }
    {
        std::vector<BtTerm> t = rnd_terms(5);
        t[0] = term(rnd_fr(), (uint32_t)0); t[2] = term(rnd_fr(), (uint32_t)(G->P.size() - 1)); t[4] = term(rnd_fr(), (uint32_t)0);
        agrees(t, "generator slots mixed with points");
    }
    check(pt_eq(term_sum(nullptr, 0, *G), pt_identity()), "an empty list is the identity");
    CPoint junk; memset(junk.b, 0xff, 32);
    { std::vector<BtTerm> t = rnd_terms(4); t[0] = term(fr_one(), junk); check(code_of(t) == OTTI_ERR_VERIFY_DECOMPRESS, "an encoding that does not decode, first"); }
    { std::vector<BtTerm> t = rnd_terms(4); t[3] = term(fr_one(), junk); check(code_of(t) == OTTI_ERR_VERIFY_DECOMPRESS, "an encoding that does not decode, last"); }
    { std::vector<BtTerm> t = rnd_terms(2); t.push_back(term(fr_one(), (uint32_t)G->P.size())); check(code_of(t) == OTTI_ERR_VERIFY_INTERNAL, "a slot past the generators"); }
}

// ------------------------------------------------------------------------------------------------ the sites
typedef std::function<void(Transcript &, Deferred &)> Site;
// the site's verdict as the verifiers take it (Deferred with no threads: every equation runs in finish())
static int verdict(const Site &site) {
    Transcript tr("term_sum_check", 14); Deferred later(0);
    try { site(tr, later); later.finish(); return 0; } catch (const VerifyFail &f) { return f.code; }
}
// accepted, and the lists the same site states to a collecting Deferred are `equations` lists that each sum to the identity
static void accepted(const Site &site, size_t equations, const char *what) {
    bool ok = verdict(site) == 0;
    BtEquations E; Transcript tr("term_sum_check", 14); Deferred later(&E);
    try { site(tr, later); later.finish(); } catch (const VerifyFail &) { ok = false; }
    ok = ok && E.count() == equations;
    for (size_t k = 0; ok && k < E.count(); k++) ok = pt_eq(term_sum(E.terms.data() + E.eq[k], E.eq[k + 1] - E.eq[k], *G), pt_identity());
    check(ok, what);
}
static void refused_with_each_replaced(const Site &site, const std::vector<Fr *> &scalars, const std::vector<CPoint *> &points, const char *what) {
    for (size_t k = 0; k < scalars.size(); k++) { const Fr keep = *scalars[k]; *scalars[k] = rnd_fr(); check(verdict(site) != 0, what, k); *scalars[k] = keep; }
    for (size_t k = 0; k < points.size(); k++) { const CPoint keep = *points[k]; *points[k] = enc(rnd_pt()); check(verdict(site) != 0, what, 100 + k); *points[k] = keep; }
}

static void knowledge_site() {
    const uint8_t seed[32] = {1}; RandomTape tape(seed); Transcript ptr("term_sum_check", 14);
    CPoint C; KnowledgeProof pf = knowledge_prove(C, *G, ptr, tape, rnd_fr(), rnd_fr());
    const Site site = [&](Transcript &tr, Deferred &later) { knowledge_verify(pf, *G, tr, C, later); };
    accepted(site, 1, "knowledge proof accepted");
    refused_with_each_replaced(site, {&pf.z1, &pf.z2}, {&C, &pf.alpha}, "knowledge proof with a field replaced");
}
static void equality_site() {
    const uint8_t seed[32] = {2}; RandomTape tape(seed); Transcript ptr("term_sum_check", 14);
    const Fr v = rnd_fr(), s1 = rnd_fr(), s2 = rnd_fr();
    EqualityProof pf = equality_prove(*G, ptr, tape, v, s1, v, s2);
    const Term t1[2] = {{G->sc_1.G[0], v}, {G->sc_1.h, s1}}, t2[2] = {{G->sc_1.G[0], v}, {G->sc_1.h, s2}};
    CPoint C1, C2; G->commit_terms_c(C1.b, t1, 2); G->commit_terms_c(C2.b, t2, 2);
    const Site site = [&](Transcript &tr, Deferred &later) { equality_verify(pf, *G, tr, C1, C2, later); };
    accepted(site, 1, "equality proof accepted");
    refused_with_each_replaced(site, {&pf.z}, {&C1, &C2, &pf.alpha}, "equality proof with a field replaced");
}
static void product_site() {
    const uint8_t seed[32] = {3}; RandomTape tape(seed); Transcript ptr("term_sum_check", 14);
    const Fr x = rnd_fr(), y = rnd_fr();
    CPoint X, Y, Z; ProductProof pf = product_prove(X, Y, Z, *G, ptr, tape, x, rnd_fr(), y, rnd_fr(), fr_mul(x, y), rnd_fr());
    const Site site = [&](Transcript &tr, Deferred &later) { product_verify(pf, *G, tr, X, Y, Z, later); };
    accepted(site, 3, "product proof accepted");
    refused_with_each_replaced(site, {&pf.z[0], &pf.z[1], &pf.z[2], &pf.z[3], &pf.z[4]}, {&X, &Y, &Z, &pf.alpha, &pf.beta, &pf.delta}, "product proof with a field replaced");
}
// one cubic sum-check round by the prover's two halves; the verifier's side is the round of ZKSumcheckInstanceProof::verify around dotproduct_verify
static void dotproduct_site() {
    const uint8_t seed[32] = {4}; RandomTape tape(seed); Transcript ptr("term_sum_check", 14);
    const Gens &g = *G; const GensView &gn = g.sc_4; const size_t ne = 4;
    SumcheckState st; sumcheck_draw_tape(st, tape, 1, ne);
    RoundPre &pre = st.pre[0];
    {   // what the device prepares from the tape alone
        Term t[5]; for (size_t i = 0; i < ne; i++) t[i] = {gn.G[i], pre.d[i]}; t[ne] = {gn.h, pre.r_delta};
        pre.delta = g.commit_terms(t, ne + 1); pre.delta_c = enc(pre.delta);
        const Term bp = {gn.h, st.blinds_poly[0]}, be = {g.sc_1.h, st.blinds_evals[0]}, rb = {g.sc_1.h, pre.r_beta};
        pre.bp_h = g.commit_terms(&bp, 1); pre.be_h = g.commit_terms(&be, 1); pre.rb_h = g.commit_terms(&rb, 1); pre.to_fe();
    }
    st.claim = rnd_fr(); st.blind_claim = rnd_fr();
    { const Term t[2] = {{g.sc_1.G[0], st.claim}, {g.sc_1.h, st.blind_claim}}; g.commit_terms_c(st.comm_claim.b, t, 2); }
    CPoint comm_claim = st.comm_claim;
    Fr evals[4] = {rnd_fr(), fr_zero(), rnd_fr(), rnd_fr()}; evals[1] = fr_sub(st.claim, evals[0]);      // p(0) + p(1) = claim
    ZKSumcheckProof pf; pf.comm_polys.resize(1); pf.comm_evals.resize(1); pf.proofs.resize(1);
    const RoundPart1 p1 = sumcheck_round_begin(pf, 0, evals, ne, st, g, gn, ptr);
    sumcheck_round_finish(pf, 0, p1, st, g, gn, ptr);
    const Site site = [&](Transcript &tr, Deferred &later) {
        tr.append_point("comm_poly", pf.comm_polys[0].b);
        const Fr r = tr.challenge_scalar("challenge_nextround");
        tr.append_point("comm_claim_per_round", comm_claim.b); tr.append_point("comm_eval", pf.comm_evals[0].b);
        const std::vector<Fr> w = tr.challenge_vector("combine_two_claims_to_one", 2);
        const CPoint target = enc(pt_add(host_scalarmul(dec(comm_claim), w[0]), host_scalarmul(dec(pf.comm_evals[0]), w[1])));
        Fr a[4], pw = fr_one();
        for (size_t k = 0; k < ne; k++) { a[k] = fr_add(fr_mul(w[0], fr_from_u64(k == 0 ? 2 : 1)), fr_mul(w[1], pw)); pw = fr_mul(pw, r); }
        dotproduct_verify(pf.proofs[0], g, gn, tr, a, ne, pf.comm_polys[0], target, later);
    };
    accepted(site, 2, "sum-check round's dot-product proof accepted");
    DotProductProof &dp = pf.proofs[0];
    refused_with_each_replaced(site, {&dp.z[0], &dp.z[1], &dp.z[2], &dp.z[3], &dp.z_delta, &dp.z_beta}, {&pf.comm_polys[0], &comm_claim, &pf.comm_evals[0], &dp.delta, &dp.beta},
                               "sum-check round's dot-product proof with a field replaced");
}
// DotProductProofLog::prove over the first n generators, for the site's own check only (the library's prover of it runs on the device)
static void dotproductlog_site() {
    const Gens &g = *G; const PcView v = {g.pc_n.h, g.pc_1.G[0], g.pc_1.h, g.R};
    const Pt Q = g.P[v.g1], H = g.P[v.h_n], H1 = g.P[v.h1];
    size_t n = v.R;
    std::vector<Fr> x(n), b(n); for (size_t i = 0; i < n; i++) { x[i] = rnd_fr(); b[i] = rnd_fr(); }
    const std::vector<Fr> a = b;
    const Fr blind_x = rnd_fr(), blind_y = rnd_fr();
    std::vector<Pt> Gv(g.P.begin(), g.P.begin() + n);
    Transcript ptr("term_sum_check", 14);
    ptr.append_protocol_name("dot product proof (log)");
    CPoint Cx = enc(pt_add(host_msm(x.data(), Gv.data(), n), host_scalarmul(H, blind_x)));
    CPoint Cy = enc(pt_add(host_scalarmul(Q, dot(x.data(), b.data(), n)), host_scalarmul(H1, blind_y)));
    ptr.append_point("Cx", Cx.b); ptr.append_point("Cy", Cy.b);
    Fr blind = fr_add(blind_x, blind_y);
    DotProductProofLog pf;
    while (n > 1) {
        n /= 2;
        const Fr cL = dot(&x[0], &b[n], n), cR = dot(&x[n], &b[0], n), bl = rnd_fr(), br = rnd_fr();
        const Pt L = pt_add(pt_add(host_msm(&x[0], &Gv[n], n), host_scalarmul(Q, cL)), host_scalarmul(H, bl));
        const Pt R = pt_add(pt_add(host_msm(&x[n], &Gv[0], n), host_scalarmul(Q, cR)), host_scalarmul(H, br));
        pf.L_vec.push_back(enc(L)); pf.R_vec.push_back(enc(R));
        ptr.append_point("L", pf.L_vec.back().b); ptr.append_point("R", pf.R_vec.back().b);
        const Fr u = ptr.challenge_scalar("u"), ui = fr_inv(u);
        for (size_t i = 0; i < n; i++) {
            x[i] = fr_add(fr_mul(x[i], u), fr_mul(ui, x[n + i])); b[i] = fr_add(fr_mul(b[i], ui), fr_mul(u, b[n + i]));
            Gv[i] = pt_add(host_scalarmul(Gv[i], ui), host_scalarmul(Gv[n + i], u));
        }
        blind = fr_add(blind, fr_add(fr_mul(bl, fr_sqr(u)), fr_mul(br, fr_sqr(ui))));
    }
    const Fr d = rnd_fr(), r_delta = rnd_fr(), r_beta = rnd_fr();
    pf.delta = enc(pt_add(host_scalarmul(Gv[0], d), host_scalarmul(H1, r_delta)));
    pf.beta = enc(pt_add(host_scalarmul(Q, d), host_scalarmul(H1, r_beta)));
    ptr.append_point("delta", pf.delta.b); ptr.append_point("beta", pf.beta.b);
    const Fr c = ptr.challenge_scalar("c");
    pf.z1 = fr_add(d, fr_mul(c, fr_mul(x[0], b[0])));
    pf.z2 = fr_add(fr_mul(b[0], fr_add(fr_mul(c, blind), r_beta)), r_delta);
    const Site site = [&](Transcript &tr, Deferred &later) { dotproductlog_verify(pf, v.R, g, v, tr, a.data(), Cx, Cy, &later); };
    accepted(site, 1, "log dot-product proof accepted");
    std::vector<CPoint *> points = {&Cx, &Cy, &pf.delta, &pf.beta};
    for (CPoint &p : pf.L_vec) points.push_back(&p);
    for (CPoint &p : pf.R_vec) points.push_back(&p);
    refused_with_each_replaced(site, {&pf.z1, &pf.z2}, points, "log dot-product proof with a field replaced");
    // the same equation with no Deferred at all: its parts run inline
    Transcript tr("term_sum_check", 14);
    bool inline_ok = true; try { dotproductlog_verify(pf, v.R, g, v, tr, a.data(), Cx, Cy, nullptr); } catch (const VerifyFail &) { inline_ok = false; }
    check(inline_ok, "log dot-product proof accepted inline");
}

int main() {
    G = gens_new(16, 16, 0);                                    // R = 4: P[0 .. 4), G_1 = P[4], h = P[5]
    evaluator_cases();
    knowledge_site(); equality_site(); product_site(); dotproduct_site(); dotproductlog_site();
    G.reset();
    printf("term_sum_check: %d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
