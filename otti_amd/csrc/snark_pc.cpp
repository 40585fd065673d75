// SNARK mode's product circuits on the MI355X and their batched layered sum-check (ProductCircuitEvalProofBatched::prove).  Follows upstream
// libspartan src/product_tree.rs and src/sumcheck.rs (prove_cubic_batched) step for step; see snark.h and, for the layer plan, pc_plan.h.
#include "snark_prover.h"
#include "pool.h"
#include "hosttail.h"

namespace otti {

void Circuits::gather_small(DevCtx &c, ShardComm &sh) {
    small.assign(nl, {});
    for (size_t k = 0; k < nl; k++) {
        const size_t h = side(k);
        if (h > kSmallSide) continue;
        small[k].resize(count);
        for (auto &lr : small[k]) { lr.first.resize(h); lr.second.resize(h); }
        if (k < nl_dev) {                                 // on the devices: every rank's share, interleaved
            const size_t hl = side_dev(k);
            std::vector<Fr> mine(2 * hl * count), all(mine.size() * (size_t)G);
            for (int i = 0; i < count; i++) {
                OTTI_HIP(hipMemcpyAsync(&mine[(size_t)2 * i * hl], left(i, k), hl * sizeof(Fr), hipMemcpyDeviceToHost, c.stream));
                OTTI_HIP(hipMemcpyAsync(&mine[(size_t)(2 * i + 1) * hl], right(i, k), hl * sizeof(Fr), hipMemcpyDeviceToHost, c.stream));
            }
            OTTI_HIP(hipStreamSynchronize(c.stream));
            sh.allgather(mine.data(), mine.size() * sizeof(Fr), all.data());
            for (int i = 0; i < count; i++) {
                interleave_ranks(small[k][i].first.data(), all.data(), (size_t)G, mine.size(), (size_t)2 * i * hl, hl);
                interleave_ranks(small[k][i].second.data(), all.data(), (size_t)G, mine.size(), (size_t)(2 * i + 1) * hl, hl);
            }
        } else {                                          // above the devices' layers: compute_layer on the host from the layer below
            for (int i = 0; i < count; i++) {
                const auto &below = small[k - 1][i]; auto &lr = small[k][i];
                for (size_t e = 0; e < h; e++) { lr.first[e] = fr_mul(below.first[e], below.second[e]); lr.second[e] = fr_mul(below.first[h + e], below.second[h + e]); }
            }
        }
    }
}

namespace {
std::atomic<bool> g_tail_timed_out{false};
// The knobs of the layer plan (pc_plan.h).  The OTTI_PC_* switches are read once per process; what the device and the process's state allow, per call.
PcKnobs pc_knobs(DevCtx &c, bool tail_allowed) {
    // OTTI_PC_TAIL=0 switches the persistent tail off; OTTI_PC_TAIL_CAP shrinks its per-workgroup capacity (tests: small instances then
    // also take the route where the tail picks up tables that earlier launches folded in HBM)
    static const bool tail_env = [] { const char *e = getenv("OTTI_PC_TAIL"); return !(e && e[0] == '0'); }();
    static const size_t tail_cap = [] { const char *e = getenv("OTTI_PC_TAIL_CAP"); size_t v = e ? (size_t)atoi(e) : 0; return (v >= 2 && v <= (size_t)kTailCap && !(v & (v - 1))) ? v : (size_t)kTailCap; }();
    static const size_t tail_per_wg = [] { const char *e = getenv("OTTI_PC_TAIL_PER_WG"); size_t v = e ? (size_t)atoi(e) : 0; return (v >= 16 && v <= (size_t)kTailCap && !(v & (v - 1))) ? v : (size_t)128; }();
    static const size_t lgt_env_many = [] { const char *e = getenv("OTTI_PC_LGT_MANY"); return e ? (size_t)atoi(e) : (size_t)0; }();
    static const size_t lgt_env_few = [] { const char *e = getenv("OTTI_PC_LGT_FEW"); return e ? (size_t)atoi(e) : (size_t)0; }();
    static const size_t pc_arm_max = [] { const char *e = getenv("OTTI_PC_ARM_MAX"); return e ? (size_t)atoll(e) : (size_t)1 << 22; }();
    PcKnobs k;
    k.tail_cap = tail_cap; k.tail_per_wg = tail_per_wg; k.arm_max = pc_arm_max;
    const bool fr8 = host_fr8_available();                  // the AVX-512 IFMA host tail: 6 / 7 rounds per layer; the scalar form: 4 / 5 (pc_plan.h)
    k.lgt_many = lgt_env_many ? lgt_env_many : (fr8 ? 6 : 4); k.lgt_few = lgt_env_few ? lgt_env_few : (fr8 ? 7 : 5);
    k.arm_ok = c.armed_ok();
    k.tail_ok = k.arm_ok && tail_env && !pc_tail_timed_out() && tail_allowed;
    k.tail_groups_max = std::min(kTailMaxGroups, c.num_cu);
    return k;
}
// OTTI_PC_PREEXPORT=0: the layers the host plays alone are exported by a launch at the head of each, not ahead of time (PcBatch::pre_export)
bool pc_preexport_env() { static const bool on = [] { const char *e = getenv("OTTI_PC_PREEXPORT"); return !(e && e[0] == '0'); }(); return on; }
bool pc_trace_env() { static const bool on = getenv("OTTI_TRACE") != nullptr; return on; }

// OTTI_TRACE: where a batch's time went.  Kinds 0 .. 2 are the rounds by PcRound (counted); the others are parts of them and the layers' set-up
struct PcTrace {
    enum { tail_first = 3, tail_wait, tail_sum, layer0, kinds };
    double ms[kinds] = {}; size_t rounds[3] = {}, tail_layers = 0;
    void add(int kind, double dt) { ms[kind] += dt; if (kind < 3) rounds[kind]++; }
    void print(int np, size_t nl) const {
        const size_t nt = rounds[(int)PcRound::tail], nla = rounds[(int)PcRound::launch]; const double tail_ms = ms[(int)PcRound::tail], launch_ms = ms[(int)PcRound::launch];
        fprintf(stderr, "[otti] pcbatch ni=%d layers=%zu (tail in %zu): %zu tail rounds %.3f ms (%.1f us each: first mail in after %.1f, all after %.1f, summed and combined after %.1f), %zu launch rounds %.3f ms (%.1f us each), %zu host rounds %.3f ms, layer set-up %.3f ms\n",
                np, nl, tail_layers, nt, tail_ms, nt ? 1e3 * tail_ms / nt : 0.0, nt ? 1e3 * ms[tail_first] / nt : 0.0, nt ? 1e3 * ms[tail_wait] / nt : 0.0, nt ? 1e3 * ms[tail_sum] / nt : 0.0, nla, launch_ms,
                nla ? 1e3 * launch_ms / nla : 0.0, rounds[(int)PcRound::host], ms[(int)PcRound::host], ms[layer0]);
    }
};

// a layer's tables and, from its shape alone, what its rounds are made of (pc_plan.h)
struct Plan : PcLayerPlan { size_t layer_id; int ni; bool with_dotp, on_device; PcList P; };
enum class TailSrc { small, gathered, pinned };            // where the host tail's tables come from (PcBatch::build_host_tail)

// One batched proof in progress: what pcbatch_prove's steps share.  The steps are in the order the driver calls them.
struct PcBatch {
    DevCtx &c; Circuits &C; DotpTables *const D; const std::vector<Fr> &dotp_evals; Transcript &tr; ShardComm *const sh;
    const int np; const size_t nl, G, rk;
    const PcKnobs knobs; const int host_threads; const bool trace = pc_trace_env();
    // eq(rand[1..], .) of a layer with nr variables as the round kernels read it: pyramids over the last n_lo of rand[1..] and the n_hi before them
    Fr *const pyr_lo, *const pyr_hi;
    const Fr one = fr_one();
    ProductCircuitEvalProofBatched pf; std::vector<Fr> claims, rand, rprod;
    // launched at the end of the layer before (launch_ahead): the pyramids of the layer about to start, and its first round's kernel
    bool pyr_ahead = false, eval_ahead = false; unsigned long long eval_ahead_tick = 0;
    std::vector<unsigned long long> pre_tick; std::vector<int> pre_slot;      // pre_export: the ticket and the place of every layer exported ahead of time
    PcTrace t;
    // the layer being played
    size_t li = 0; Plan plan{}; unsigned long long tail_seq = 0; std::vector<unsigned long long> tick; int layer_slot = kPcTailSlot;     // layer_slot: where this layer's exported tables are
    std::vector<Fr> coeff; Fr e;                             // the batching coefficients and the running claim
    std::vector<std::vector<Fr>> tA, tB, tC; std::vector<Fr> tE; std::unique_ptr<HostTail> host_tail;   // host tail: T elements per table
    Fr cj, cj_tail;                                          // cj_tail: the eq factor accumulated before the tail took over (its eq table carries the rest)
    PcBatch(DevCtx &c_, Circuits &C_, const std::vector<Fr> &evals, DotpTables *D_, const std::vector<Fr> &dotp_evals_, Transcript &tr_, Fr *pyr, bool tail_allowed, ShardComm *sh_)
        : c(c_), C(C_), D(D_), dotp_evals(dotp_evals_), tr(tr_), sh(sh_), np(C_.count), nl(C_.nl), G(sh_ ? (size_t)sh_->world() : 1), rk(sh_ ? (size_t)sh_->rank() : 0),
          knobs(pc_knobs(c_, tail_allowed)), host_threads(std::min(8, SpinPool::get().workers() + 1)), pyr_lo(pyr), pyr_hi(pyr + 8192), claims(evals), pre_tick(nl, 0), pre_slot(nl, kPcTailSlot) { pf.layers.resize(nl); }
    PcLayerShape shape_of(size_t li_, size_t nr_) const {
        const size_t layer_id = nl - 1 - li_;
        const bool with_dotp = layer_id == 0 && D && D->n;
        return PcLayerShape{nr_, np + (with_dotp ? D->n : 0), layer_id < C.nl_dev};      // (sharded: the layers with sides shorter than the number of ranks exist on the host only)
    }
    Plan make_plan(size_t li_, size_t nr_) const {
        const PcLayerShape s = shape_of(li_, nr_);
        Plan p{pc_layer_plan(s, knobs), nl - 1 - li_, s.ni, s.ni > np, s.on_device, {}};
        p.P.n = 0;
        for (int i = 0; i < np; i++) { p.P.A[p.P.n] = p.on_device ? C.left(i, p.layer_id) : nullptr; p.P.B[p.P.n] = p.on_device ? C.right(i, p.layer_id) : nullptr; p.P.C[p.P.n] = nullptr; p.P.n++; }
        if (p.with_dotp) for (int i = 0; i < D->n; i++) { p.P.A[p.P.n] = D->l[i]; p.P.B[p.P.n] = D->r[i]; p.P.C[p.P.n] = D->w[i]; p.P.n++; }
        return p;
    }
    EqSrc eq_src_of(size_t nr_, size_t m, const Fr *first_var) const {
        const size_t nv = nr_ ? nr_ - 1 : 0, n_lo = std::min<size_t>(nv, 12);
        EqSrc s;
        const size_t mt = std::min(m, nv);                       // tabulated variables
        if (mt <= n_lo) { s.hi = nullptr; s.lo = pyr_lo + (((size_t)1 << mt) - 1); s.lo_bits = 0; }
        else { s.hi = pyr_hi + (((size_t)1 << (mt - n_lo)) - 1); s.lo = pyr_lo + (((size_t)1 << n_lo) - 1); s.lo_bits = (int)n_lo; }
        if (m > nv) { if (m != nv + 1 || !nr_ || !first_var) throw Error(OTTI_ERR_INTERNAL, "eq table over more variables than the layer has"); s.top_bit = (int)nv; s.top = *first_var; }
        s.stride = (uint32_t)G; s.offset = (uint32_t)rk;           // sharded: item i of a kernel is element i G + rk of the table
        return s;
    }
    void launch_pyramids(size_t nr_, const Fr *vars_from_1 /* nr_ - 1 of them */) {
        const size_t nv = nr_ ? nr_ - 1 : 0, n_lo = std::min<size_t>(nv, 12), n_hi = nv - n_lo;
        if (n_hi > 13) throw Error(OTTI_ERR_BAD_ARG, "product circuit over more than 2^26 elements");
        dev_eq_pyramid2(c, vars_from_1 + n_hi, n_lo, pyr_lo, vars_from_1, n_hi, n_hi ? pyr_hi : nullptr);
    }
    // The layers the host plays alone (sides of at most T elements: the first 7 / 8 layers) are exported to pinned memory by ONE run of tiny launches
    // queued here, each to a place of its own — not one launch and one wait at the head of each layer (layer li has li variables whatever the
    // challenges are).  on_start (the caller's work for a second stream) is queued after them, so that they are not held up behind it.
    // OTTI_PC_PREEXPORT=0: a launch per layer as before.
    void pre_export() {
        if (sh || !pc_preexport_env()) return;
        PcPreExport pre;
        for (size_t l = 0; l < nl; l++) {
            const int slot = pre.take(shape_of(l, l), knobs);
            if (slot < 0) break;
            const Plan p = make_plan(l, l);
            pre_slot[l] = slot; pre_tick[l] = dev_pc_export(c, p.P, p.h, false, nullptr, slot);
        }
    }
    // ---- a layer's launches
    EqSrc eq_src(size_t m) const { return eq_src_of(plan.nr, m, plan.nr ? rand.data() : nullptr); }
    bool armed(size_t k) const { return plan.armed(k, plan.ni, knobs); }      // launch k is queued a round ahead of its challenge (pc_plan.h)
    void launch_tail(const Fr *r) { tail_seq = dev_pc_tail(c, plan.P, plan.tailW, plan.h >> plan.k0, plan.T, r, eq_src(plan.nr - plan.k0), kPcTailSlot); }
    void launch_for(size_t k, const Fr *r) {
        const size_t len_in = (plan.h >> (k - 1)) / G;         // of this rank
        if (plan.tail && k == plan.k0) { launch_tail(r); return; }
        tick[k] = k < plan.ndev ? dev_pc_fold_eval(c, plan.P, len_in, r, eq_src(plan.nr - k - 1), kSumSlot) : dev_pc_export(c, plan.P, len_in, true, r, kPcTailSlot);
    }
    void start_layer(size_t li_) {
        const double t0 = trace ? now_ms() : 0;
        li = li_; plan = make_plan(li, rand.size());
        if (plan.with_dotp) { if (D->len != plan.h / G) throw Error(OTTI_ERR_INTERNAL, "dot-product circuits do not match the input layer"); claims.insert(claims.end(), dotp_evals.begin(), dotp_evals.end()); }
        if (sh && plan.ndev && (plan.T < G || !plan.on_device)) throw Error(OTTI_ERR_INTERNAL, "sharded product circuits: more ranks than a host tail has elements");
        tail_seq = 0;
        // The layer's FIRST variable is in no pyramid: no round's factor table contains it (round j uses eq over rand[j+1..]), only the persistent
        // tail's own eq table when it starts at round 0 (EqSrc.top) — and rand[0] is the last challenge to be drawn, so without it the pyramids of
        // layer li + 1 (and its first round's kernel, when that is a launch of its own) are issued as soon as layer li's last round challenge is
        // out (launch_ahead) and run while the host absorbs the layer's claims and draws the next coefficients.
        if (plan.ndev && !pyr_ahead) launch_pyramids(plan.nr, rand.data() + 1);
        pyr_ahead = false;
        tick.assign(plan.ndev + 2, 0);
        if (plan.round(0) == PcRound::tail) launch_tail(nullptr);
        else if (plan.ndev) { tick[0] = eval_ahead ? eval_ahead_tick : dev_pc_eval(c, plan.P, plan.h / G, eq_src(plan.nr - 1), kSumSlot); if (armed(1)) launch_for(1, nullptr); }
        else if (!sh) tick[0] = pre_tick[li] ? pre_tick[li] : dev_pc_export(c, plan.P, plan.h, false, nullptr, kPcTailSlot);     // (sharded: the host-only layers are in C.small already)
        layer_slot = (!plan.ndev && pre_tick[li]) ? pre_slot[li] : kPcTailSlot;
        eval_ahead = false;
        coeff = tr.challenge_vector("rand_coeffs_next_layer", claims.size());
        e = fr_zero(); for (size_t k = 0; k < claims.size(); k++) e = fr_add(e, fr_mul(claims[k], coeff[k]));
        rprod.clear();
        tA.assign(plan.ni, {}); tB.assign(plan.ni, {}); tC.assign(plan.ni, {}); host_tail.reset();
        cj = cj_tail = one;
        if (trace) { t.add(PcTrace::layer0, now_ms() - t0); if (plan.tail) t.tail_layers++; }
    }
    // ---- a round's sums (points 0, 2, 3), by kind
    // a round of the persistent launch: W partial sums per instance, in the workgroups' own mail lines; the eq table is a real
    // third table there, so the sums already carry the bound variable's factor — only the factor of the rounds before k0 is missing
    void sums_tail(size_t j, Fr s[3]) {
        const double t0 = trace ? now_ms() : 0;
        if (j == plan.k0) cj_tail = cj;
        Fr inst_sums[3 * kMaxInst];
        if (trace) { c.wait_tail(1, tail_seq + (j - plan.k0)); t.add(PcTrace::tail_first, now_ms() - t0); }     // (trace only: when the first line is in)
        c.wait_tail_sums(plan.ni, plan.tailW, tail_seq + (j - plan.k0), inst_sums);
        if (trace) t.add(PcTrace::tail_wait, now_ms() - t0);
        Fr ps[3], ds[3];                                      // the product instances' sums (they share the eq factor) and the triples', times the coefficients
        weighted_sums3(inst_sums, coeff.data(), np, plan.ni, ps, ds);
        for (int p = 0; p < 3; p++) s[p] = fr_add(ds[p], fr_mul(cj_tail, ps[p]));
        if (trace) t.add(PcTrace::tail_sum, now_ms() - t0);
    }
    void sums_launch(size_t j, Fr s[3]) {
        c.wait_ticket(tick[j]);
        if (sh) sh->allreduce_fr(&c.h_results[kSumSlot], (size_t)3 * plan.ni);      // this round's sums over the ranks' residue classes (pinned memory: the next launch writes them afresh)
        const Fr &tau = rand[j];
        const Fr w0 = fr_sub(one, tau), dw = fr_sub(fr_add(tau, tau), one), w2 = fr_add(w0, fr_add(dw, dw)), w3 = fr_add(w2, dw);
        const Fr f[3] = {fr_mul(cj, w0), fr_mul(cj, w2), fr_mul(cj, w3)};
        Fr ps[3], ds[3];                                      // the product circuits share the eq factor
        weighted_sums3(&c.h_results[kSumSlot], coeff.data(), np, plan.ni, ps, ds);
        for (int p = 0; p < 3; p++) s[p] = fr_add(ds[p], fr_mul(f[p], ps[p]));
    }
    void sums_host(Fr s[3]) { if (!host_tail) build_host_tail(); host_tail->sums(s); }
    // The host tail's tables, from one of three sources.  small: a layer the host plays alone in a sharded proof is in Circuits::small, in full on
    // every rank already (product circuits only).  gathered: every rank's share of the exported tables, interleaved.  pinned: one device — the
    // host tail packs the tables straight out of the pinned buffer the device exported them to.
    void build_host_tail() {
        const TailSrc src = !sh ? TailSrc::pinned : plan.ndev == 0 ? TailSrc::small : TailSrc::gathered;
        if (src == TailSrc::small) {
            if (C.small[plan.layer_id].size() != (size_t)plan.ni || C.small[plan.layer_id][0].first.size() != plan.T) throw Error(OTTI_ERR_INTERNAL, "sharded product circuits: a host-played layer was not gathered (host tail longer than kSmallSide)");
            for (int k = 0; k < plan.ni; k++) { tA[k] = C.small[plan.layer_id][k].first; tB[k] = C.small[plan.layer_id][k].second; }
        } else if (src == TailSrc::gathered) {
            c.wait_ticket(tick[plan.ndev]);
            const size_t Tl = plan.T / G, per = (size_t)3 * plan.ni * Tl;
            std::vector<Fr> all(per * G);
            sh->allgather(&c.h_results[kPcTailSlot], per * sizeof(Fr), all.data());
            for (int k = 0; k < plan.ni; k++) {
                std::vector<Fr> *const tab[3] = {&tA[k], &tB[k], k >= np ? &tC[k] : nullptr};
                for (int t3 = 0; t3 < 3; t3++) if (tab[t3]) { tab[t3]->resize(plan.T); interleave_ranks(tab[t3]->data(), all.data(), G, per, ((size_t)3 * k + t3) * Tl, Tl); }
            }
        } else if (plan.tail) c.wait_tail(plan.ni * plan.tailW, tail_seq + (plan.ndev - plan.k0));
        else c.wait_ticket(tick[plan.ndev]);
        tE = eq_evals_host(rand.data() + plan.ndev, plan.nr - plan.ndev);
        for (auto &x : tE) x = fr_mul(x, cj);
        std::vector<const Fr *> pa(plan.ni), pb(plan.ni), pc(plan.ni);
        for (int k = 0; k < plan.ni; k++) {
            const Fr *base = &c.h_results[layer_slot + (size_t)3 * k * plan.T]; const bool direct = src == TailSrc::pinned;
            pa[k] = direct ? base : tA[k].data(); pb[k] = direct ? base + plan.T : tB[k].data(); pc[k] = k < np ? nullptr : direct ? base + 2 * plan.T : tC[k].data();
        }
        host_tail = HostTail::make(np, plan.ni - np, plan.T, pa.data(), pb.data(), pc.data(), tE.data(), coeff.data(), host_threads);   // hosttail.h: AVX-512 IFMA where the CPU has it
    }
    // ---- after a round's challenge
    // The layer's last challenge: everything the NEXT layer's eq pyramids are made of (its variables 1 .. nr are this layer's challenges; its
    // variable 0 comes after the claims and is in no pyramid).  The device is idle — this layer's last rounds are the host's — so
    // the pyramids, and the next layer's first sums when they are a launch of their own (they read tables and pyramids only), run under
    // the host's closing work and the next layer's coefficient draws instead of in front of its first round.
    void launch_ahead() {
        const Plan nx = make_plan(li + 1, plan.nr + 1);
        if (!nx.ndev) return;
        launch_pyramids(nx.nr, rprod.data());
        pyr_ahead = true;
        if (nx.round(0) != PcRound::tail && !(sh && (nx.T < G || !nx.on_device))) {
            eval_ahead_tick = dev_pc_eval(c, nx.P, nx.h / G, eq_src_of(nx.nr, nx.nr - 1, nullptr), kSumSlot);
            eval_ahead = true;
        }
    }
    void advance(PcRound kind, size_t j, const Fr &r_j) {
        if (kind == PcRound::host) { host_tail->fold(r_j); return; }
        if (kind == PcRound::tail) c.go(&r_j, 1);              // the persistent launch folds and goes on (or exports, after its last round)
        else {
            if (armed(j + 1)) c.go(&r_j, 1); else launch_for(j + 1, &r_j);
            if (armed(j + 2)) launch_for(j + 2, nullptr);
        }
        cj = fr_mul(cj, fr_add(fr_mul(rand[j], r_j), fr_mul(fr_sub(one, rand[j]), fr_sub(one, r_j))));
    }
    // SumcheckInstanceProof::prove_cubic_batched, one round
    void round(size_t j) {
        const double t0 = trace ? now_ms() : 0;
        const PcRound kind = plan.round(j);
        Fr s[3];
        switch (kind) { case PcRound::tail: sums_tail(j, s); break; case PcRound::launch: sums_launch(j, s); break; case PcRound::host: sums_host(s); break; }
        Fr evals4[4] = {s[0], fr_sub(e, s[0]), s[1], s[2]}, poly[4];
        unipoly_from_evals(poly, evals4, 4);
        append_unipoly(tr, poly, 4);
        const Fr r_j = tr.challenge_scalar("challenge_nextround");
        rprod.push_back(r_j);
        if (kind == PcRound::host && j + 1 == plan.nr && li + 1 < nl) launch_ahead();      // (before the host folds: the device starts at once)
        advance(kind, j, r_j);
        e = unipoly_eval(poly, 4, r_j);
        LayerProofBatched &L = pf.layers[li];
        L.coeffs.push_back(poly[0]); L.coeffs.push_back(poly[2]); L.coeffs.push_back(poly[3]);      // UniPoly::compress
        if (trace) t.add((int)kind, now_ms() - t0);
    }
    // ---- the tables' last elements: claims_prod (left, right per circuit; the eq table's is not sent), then the dot-product triples; r_layer
    void close_layer() {
        if (host_tail) {                                    // out of the host tail's own representation
            if (host_tail->len() != 1) throw Error(OTTI_ERR_INTERNAL, "host sum-check tail ended early");
            for (int k = 0; k < plan.ni; k++) { Fr t3[3]; host_tail->last(k, t3); tA[k].assign(1, t3[0]); tB[k].assign(1, t3[1]); if (k >= np) tC[k].assign(1, t3[2]); }
        } else if (sh) {                                    // a layer without rounds, sharded: from the host copies
            for (int k = 0; k < plan.ni; k++) { tA[k].assign(1, C.small[plan.layer_id][k].first[0]); tB[k].assign(1, C.small[plan.layer_id][k].second[0]); }
        } else {                                            // a layer without rounds: the tables are single elements
            c.wait_ticket(tick[0]);
            for (int k = 0; k < plan.ni; k++) { const Fr *base = &c.h_results[layer_slot + (size_t)3 * k * plan.T]; tA[k].assign(base, base + 1); tB[k].assign(base + plan.T, base + plan.T + 1); if (k >= np) tC[k].assign(base + 2 * plan.T, base + 2 * plan.T + 1); }
        }
        LayerProofBatched &L = pf.layers[li];
        L.left.resize(np); L.right.resize(np);
        for (int i = 0; i < np; i++) { L.left[i] = tA[i][0]; L.right[i] = tB[i][0]; tr.append_scalar("claim_prod_left", L.left[i]); tr.append_scalar("claim_prod_right", L.right[i]); }
        if (plan.with_dotp) for (int i = 0; i < D->n; i++) {
            const Fr t3[3] = {tA[np + i][0], tB[np + i][0], tC[np + i][0]};
            pf.dotp_left.push_back(t3[0]); pf.dotp_right.push_back(t3[1]); pf.dotp_weight.push_back(t3[2]);
            tr.append_scalar("claim_dotp_left", t3[0]); tr.append_scalar("claim_dotp_right", t3[1]); tr.append_scalar("claim_dotp_weight", t3[2]);
        }
        const Fr r_layer = tr.challenge_scalar("challenge_r_layer");
        claims.resize(np);
        for (int i = 0; i < np; i++) claims[i] = fr_add(L.left[i], fr_mul(r_layer, fr_sub(L.right[i], L.left[i])));
        rand.assign(1, r_layer); rand.insert(rand.end(), rprod.begin(), rprod.end());
    }
};
}  // namespace
bool pc_set_tail_timed_out() { return g_tail_timed_out.exchange(true); }
bool pc_tail_timed_out() { return g_tail_timed_out.load(std::memory_order_relaxed); }

// ProductCircuitEvalProofBatched::prove.  evals: the circuits' outputs (already known to the caller).  The tables are folded in place.
//
// One layer = one SumcheckInstanceProof::prove_cubic_batched over (left, right, eq(rand)) of every circuit (+ the dot-product triples at
// the input layer).  Per round ONE launch (k_pc_round: fold by the previous challenge + this round's sums, mailed to the host by the
// last workgroup).  The eq table is never stored: eq(rand, .) is a tensor product, so after j rounds it is
//   c_j * (b ? rand_j : 1 - rand_j) * E_j[i],  E_j = eq(rand[j+1..), .),  c_j = prod_{k<j} eq(rand_k, r_k)
// (two L2-resident pyramids of small tables, as phase one of the R1CS proof); the kernel returns S_t = sum_i E_j[i] (A_t B_t)[i] and the
// host applies c_j * ((1 - rand_j) + t (2 rand_j - 1)).  Once the tables are down to T elements they are exported to pinned memory and
// the host plays the last rounds itself: a launch + hand-off costs more than the arithmetic of such a round on a host core.
// sh (sharded SNARK::prove): the tables are this rank's residue classes (Circuits; D: strided copies); a device round works on them
// with the eq factor taken at the global index, its sums are added across the ranks (allreduce_fr: 3 elements per instance), and where the
// host takes a layer over the ranks' shares of its tables are gathered and interleaved.  Host rounds run on every rank alike.
ProductCircuitEvalProofBatched pcbatch_prove(DevCtx &c, Circuits &C, const std::vector<Fr> &evals, DotpTables *D, const std::vector<Fr> &dotp_evals, Transcript &tr,
                                             Fr *pyr, std::vector<Fr> &rand_out, bool tail_allowed, ShardComm *sh, const std::function<void()> *on_start) {
    if (sh && (C.G != sh->world() || C.small.size() != C.nl)) throw Error(OTTI_ERR_INTERNAL, "sharded product circuits were not prepared for this exchange");
    struct Release { DevCtx &c; ~Release() { c.go_abort(); } } release{c};      // an exception below must not leave an armed kernel waiting
    PcBatch b(c, C, evals, D, dotp_evals, tr, pyr, tail_allowed, sh);
    b.pre_export();
    if (on_start) (*on_start)();
    for (size_t li = 0; li < b.nl; li++) {
        b.start_layer(li);
        for (size_t j = 0; j < b.plan.nr; j++) b.round(j);
        b.close_layer();
    }
    if (b.trace) b.t.print(b.np, b.nl);
    rand_out = b.rand;
    return std::move(b.pf);
}

}  // namespace otti
