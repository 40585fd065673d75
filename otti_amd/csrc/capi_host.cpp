// Host-only entries of libottispartan: the self-test of the host primitives and the host measurement aids.  None of them needs a GPU.
#include "capi_common.h"

extern "C" {

int32_t otti_host_selftest(uint32_t iterations) {
    return guarded([&] {
        auto g = gens_new(16, 16, 1);
        Shake256 xof; xof.absorb("otti-host-selftest", 18);
        for (uint32_t it = 0; it < iterations; it++) {
            uint8_t w[64]; xof.squeeze(w, 64);
            Fr s = fr_from_bytes_wide(w);
            if (it == 0) s = fr_zero(); if (it == 1) s = fr_one(); if (it == 2) s = fr_neg(fr_one());
            xof.squeeze(w, 64);
            const Pt rnd = pt_from_uniform_bytes(w);
            // five-limb round trip and compression against the generic code
            uint8_t a[32], b[32];
            pt_encode_fast(a, rnd); pt_encode_ref(b, rnd);
            if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "pt_encode_fast differs from pt_encode_ref");
            const Pt back = ptfe_to(ptfe_from(rnd));
            pt_encode_ref(a, back);
            if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "five-limb round trip changed a point");
            // fixed-base table (8-bit windows, five-limb mixed additions) against a variable-base multiplication
            const size_t slot = it % g->small_tables.size();
            size_t base = 0; for (size_t i = 0; i < g->small_slot.size(); i++) if (g->small_slot[i] == (int)slot) base = i;
            Pt acc = rnd; g->small_tables[slot].accumulate(acc, s);
            const Pt want = pt_add(rnd, host_scalarmul(g->P[base], s));
            pt_encode_ref(a, acc); pt_encode_ref(b, want);
            if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "fixed-base table result differs from the variable-base multiplication");
            if (host_ifma_available()) {   // the AVX-512 IFMA mixed addition (hostifma.h) against the scalar five-limb one, both signs, on a point with lazily reduced limbs
                const NielsFe &ne = g->small_tables[slot].t[(it * 37) % g->small_tables[slot].t.size()];
                const Niels4 n4 = niels4_from(ne);
                for (int neg = 0; neg < 2; neg++) {
                    PtFe x1 = ptfe_from(rnd), x2 = x1;
                    for (int k = 0; k < 3; k++) { ptfe_madd(x1, ne, neg != 0); ifma_madd(x2, n4, neg != 0); }
                    pt_encode_fe(a, x1); pt_encode_fe(b, x2);
                    if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "IFMA mixed addition differs from the scalar one");
                }
            }
            {   // host_scalarmul (windowed; AVX-512 IFMA doublings and additions where the CPU has them) against plain double-and-add in the generic
                // 4 x u64 code of point.h, and a small multi-scalar sum against the sum of the single products
                const Fr raw = fr_to_raw(s);
                Pt ref = pt_identity();
                for (int bit = 255; bit >= 0; bit--) { ref = pt_dbl(ref); if ((raw.v[bit / 32] >> (bit % 32)) & 1) ref = pt_add(ref, rnd); }
                pt_encode_ref(a, host_scalarmul(rnd, s)); pt_encode_ref(b, ref);
                if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "host_scalarmul differs from double-and-add");
                const Fr s3[3] = {s, fr_neg(s), fr_add(s, fr_one())}; const Pt p3[3] = {rnd, g->P[1], g->P[2]};
                Pt sum = pt_add(pt_add(host_scalarmul(p3[0], s3[0]), host_scalarmul(p3[1], s3[1])), host_scalarmul(p3[2], s3[2]));
                pt_encode_ref(a, host_msm(s3, p3, 3)); pt_encode_ref(b, sum);
                if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "host_msm differs from the sum of its terms");
            }
            // the host's last sum-check rounds (hosttail.h): the AVX-512 IFMA form against the scalar one on random tables of every size, both kinds of instance
            {   // the division-step inversion against the exponentiation (the fast one falls back to the other if its own check fails: also count that it did not)
                Fr inv_fast; const Fr inv_ref = fr_inv(s);
                if (!fr_inv_fast_try(s, inv_fast)) throw Error(OTTI_ERR_INTERNAL, "fr_inv_fast gave up on an input");
                if (!fr_eq(inv_ref, inv_fast)) throw Error(OTTI_ERR_INTERNAL, "fr_inv_fast differs from fr_inv");
            }
            if (it < 128) hosttail_selftest(it);
            {   // the four-way split multiplication (verifier rounds) against the plain one
                SplitTable st; split_table_build(st, rnd);
                pt_encode_ref(a, split_table_mul(st, s)); pt_encode_ref(b, host_scalarmul(rnd, s));
                if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "split_table_mul differs from host_scalarmul");
            }
            {   // five-limb extended addition against the generic one
                PtFe x = ptfe_from(rnd); ptfe_add(x, ptfe_from(want));
                pt_encode_fe(a, x); pt_encode_ref(b, pt_add(rnd, want));
                if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "five-limb point addition differs from pt_add");
                x = ptfe_identity(); ptfe_add(x, ptfe_from(rnd)); pt_encode_fe(a, x); pt_encode_ref(b, rnd);
                if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "five-limb addition to the identity changed a point");
            }
            {   // five-limb decompression against the generic one (valid encodings, and one that is not)
                Pt d1, d2; pt_encode_ref(a, rnd);
                if (!pt_decode_fast(d1, a) || !pt_decode(d2, a)) throw Error(OTTI_ERR_INTERNAL, "a valid encoding did not decode");
                pt_encode_ref(b, d1); if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "pt_decode_fast does not invert the encoding");
                if (memcmp(&d1, &d2, sizeof(Pt)) && !(fp_eq(d1.X, d2.X) && fp_eq(d1.Y, d2.Y) && fp_eq(d1.T, d2.T))) throw Error(OTTI_ERR_INTERNAL, "pt_decode_fast differs from pt_decode");
                a[0] ^= 1;                                        // negative s: both must refuse
                if (pt_decode_fast(d1, a) != pt_decode(d2, a)) throw Error(OTTI_ERR_INTERNAL, "pt_decode_fast and pt_decode disagree on a non-canonical encoding");
                for (int k = 0; k < 32; k++) a[k] = (uint8_t)(w[k] ^ (it * 37 + k));   // arbitrary bytes: mostly invalid, sometimes valid
                a[31] &= 0x7f;
                const bool ok1 = pt_decode_fast(d1, a), ok2 = pt_decode(d2, a);
                if (ok1 != ok2) throw Error(OTTI_ERR_INTERNAL, "pt_decode_fast and pt_decode disagree on arbitrary bytes");
                if (ok1) { pt_encode_ref(b, d1); uint8_t b2[32]; pt_encode_ref(b2, d2); if (memcmp(b, b2, 32)) throw Error(OTTI_ERR_INTERNAL, "pt_decode_fast and pt_decode decode to different points"); }
            }
            {   // multiplication by a small signed integer (the SpMV kernels' path for compiled circuits) against the Montgomery product
                const int32_t cs[6] = {0, 1, -1, 0x7ffffffe, -0x7ffffffe, (int32_t)(w[5] | (w[6] << 8) | (w[7] << 16) | ((w[8] & 0x3f) << 24)) * ((w[9] & 1) ? -1 : 1)};
                for (int32_t cc : cs) {
                    const Fr cm = cc < 0 ? fr_neg(fr_from_u64((uint64_t)(-(int64_t)cc))) : fr_from_u64((uint64_t)cc);
                    if (!fr_eq(fr_mul_small(s, cc), fr_mul(s, cm))) throw Error(OTTI_ERR_INTERNAL, "fr_mul_small differs from fr_mul");
                    if (fr_small_code(cm) != cc) throw Error(OTTI_ERR_INTERNAL, "fr_small_code does not recover a small integer");
                }
                Fr big = fr_from_u64(0x80000000ull); if (fr_small_code(big) != kNotSmall || fr_small_code(fr_neg(big)) != kNotSmall) throw Error(OTTI_ERR_INTERNAL, "fr_small_code accepts 2^31");
                if (it > 2 && fr_small_code(s) != kNotSmall) throw Error(OTTI_ERR_INTERNAL, "fr_small_code accepts a random field element");
            }
            pt_encode_fast(a, pt_identity()); pt_encode_ref(b, pt_identity());
            if (memcmp(a, b, 32)) throw Error(OTTI_ERR_INTERNAL, "identity encodes differently");
        }
        {   // the transcript's fused message operations (hash.h Strobe128::merlin_append / merlin_challenge) against the separate STROBE
            // operations they stand for: random labels and messages of 0 .. 100 bytes, so that every position of the rate block, the
            // block boundary and the long-message fallback are all crossed many times
            Strobe128 fused("Merlin v1.0"), plain("Merlin v1.0");
            for (uint32_t it = 0; it < 40 * iterations + 2000; it++) {
                uint8_t rnd[8]; xof.squeeze(rnd, 8);
                const size_t L = 1 + rnd[0] % 30, n = rnd[1] % 101; const bool chal = (rnd[2] & 3) == 0;
                char label[32]; uint8_t msg[128], o1[128], o2[128];
                xof.squeeze(label, L); xof.squeeze(msg, n ? n : 1);
                const uint8_t len[4] = {(uint8_t)n, 0, 0, 0};
                if (chal) {
                    fused.merlin_challenge(label, L, o1, n);
                    plain.meta_ad(label, L, false); plain.meta_ad(len, 4, true); plain.prf(o2, n, false);
                    if (memcmp(o1, o2, n)) throw Error(OTTI_ERR_INTERNAL, "fused transcript challenge differs from the separate STROBE operations");
                } else {
                    fused.merlin_append(label, L, msg, n);
                    plain.meta_ad(label, L, false); plain.meta_ad(len, 4, true); plain.ad(msg, n, false);
                }
            }
            uint8_t o1[64], o2[64];
            fused.prf(o1, 64, false); plain.prf(o2, 64, false);
            if (memcmp(o1, o2, 64)) throw Error(OTTI_ERR_INTERNAL, "fused transcript operations left a different state");
        }
        return OTTI_OK;
    });
}

// nanoseconds per operation of the host-side primitives on the sequential path (measurement aid: tools/hostbench.py)
int32_t otti_host_tail_bench(uint32_t np, uint32_t nd, uint64_t T, uint32_t threads, uint32_t reps, double out[2]) {
    return guarded([&] {
        if (!out) throw Error(OTTI_ERR_BAD_ARG, "null out pointer");
        if (np > 12 || nd > 12 || T < 2 || T > 4096 || (T & (T - 1))) throw Error(OTTI_ERR_BAD_ARG, "host tail bench: at most 12 + 12 instances, tables of 2 .. 4096 elements");
        hosttail_bench((int)np, (int)nd, (size_t)T, (int)threads, (int)reps, out);
        return OTTI_OK;
    });
}
// ---- the host's sum of a small MSM's chunk mails (device.h MsmMail, DevCtx::msm_host_sum), reachable without a GPU
int32_t otti_host_point_from_uniform(const uint8_t b64[64], uint8_t out128[128]) {
    return guarded([&] {
        if (!b64 || !out128) throw Error(OTTI_ERR_BAD_ARG, "null pointer");
        const Pt p = pt_from_uniform_bytes(b64);
        memcpy(out128, &p, 128);
        return OTTI_OK;
    });
}
// the mails the device would write for these extended points (cached form, any representatives < 2^256), number `seq` and its tags
static std::vector<MsmMail> mails_for(const uint8_t *pts128, size_t n, unsigned long long seq) {
    std::vector<MsmMail> m(n);
    for (size_t i = 0; i < n; i++) {
        Pt p; memcpy(&p, pts128 + 128 * i, 128);
        memset(&m[i], 0, sizeof(MsmMail));
        m[i].v[0] = fp_sub(p.Y, p.X); m[i].v[1] = fp_add(p.Y, p.X); m[i].v[2] = fp_mul(p.T, fp_2D()); m[i].v[3] = fp_add(p.Z, p.Z);
        m[i].seq = seq; m[i].tag = msm_mail_tag(seq, m[i].v);
    }
    return m;
}
int32_t otti_host_point_sum(const uint8_t *pts128, size_t n, int32_t path, uint32_t parts, uint8_t out32[32]) {
    return guarded([&] {
        if ((!pts128 && n) || !out32 || n > 4096 || parts < 1 || parts > 64) throw Error(OTTI_ERR_BAD_ARG, "host point sum: bad arguments");
        if (path == 0) {                                               // the generic 4 x u64 code of point.h
            Pt acc = pt_identity();
            for (size_t i = 0; i < n; i++) { Pt p; memcpy(&p, pts128 + 128 * i, 128); acc = pt_add(acc, p); }
            pt_encode_ref(out32, acc);
            return OTTI_OK;
        }
        if (path != 1 && path != 2 && path != 3) throw Error(OTTI_ERR_BAD_ARG, "host point sum: path is 0 (generic), 1 (mails, IFMA where available), 2 (mails, scalar), 3 (1 with a stale last mail)");
        const unsigned long long seq = 0x1234567ull;
        std::vector<MsmMail> m = mails_for(pts128, n, seq);
        if (path == 3 && n) m[n - 1].seq = seq - 2;                  // left over from the launch before last on this region
        // as the prover splits a row: `parts` consecutive ranges, each summed from the identity, then added up
        PtFe acc = ptfe_identity();
        for (uint32_t k = 0; k < parts; k++) {
            const int i0 = (int)(n * k / parts), i1 = (int)(n * (k + 1) / parts);
            PtFe part = ptfe_identity();
            if (!msm_mail_sum(m.data(), i0, i1, seq, part, 1000u, path != 2)) return OTTI_ERR_INTERNAL;
            host_point_add(acc, part, path != 2);
        }
        pt_encode_ref(out32, ptfe_to(acc));
        return OTTI_OK;
    });
}
// nanoseconds per mail of msm_mail_sum over n valid mails in one range: out[0] AVX-512 IFMA (0 without it), out[1] the scalar form
int32_t otti_host_point_sum_bench(uint32_t n, uint32_t reps, double out[2]) {
    return guarded([&] {
        if (!out || n < 1 || n > 4096 || reps < 1) throw Error(OTTI_ERR_BAD_ARG, "host point sum bench: bad arguments");
        std::vector<uint8_t> pts(128 * (size_t)n);
        for (uint32_t i = 0; i < n; i++) { uint8_t w[64]; for (int k = 0; k < 64; k++) w[k] = (uint8_t)(i * 131 + k * 7 + 1); const Pt p = pt_from_uniform_bytes(w); memcpy(&pts[128 * (size_t)i], &p, 128); }
        const std::vector<MsmMail> m = mails_for(pts.data(), n, 5);
        for (int path = 0; path < 2; path++) {
            out[path] = 0;
            if (path == 0 && !host_ifma_available()) continue;
            PtFe acc = ptfe_identity();
            (void)msm_mail_sum(m.data(), 0, (int)n, 5, acc, 0u, path == 0);
            const auto t0 = std::chrono::steady_clock::now();
            for (uint32_t r = 0; r < reps; r++) { acc = ptfe_identity(); (void)msm_mail_sum(m.data(), 0, (int)n, 5, acc, 0u, path == 0); }
            out[path] = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / ((double)reps * n);
        }
        return OTTI_OK;
    });
}
int32_t otti_host_microbench(double out[10]) {
    return guarded([&] {
        if (!out) throw Error(OTTI_ERR_BAD_ARG, "null out pointer");
        auto g = gens_new(16, 16, 1);
        auto now = [] { return std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        Shake256 xof; xof.absorb("otti-host-microbench", 20);
        uint8_t w[64]; xof.squeeze(w, 64); Fr s = fr_from_bytes_wide(w); xof.squeeze(w, 64); Fr s2 = fr_from_bytes_wide(w);
        xof.squeeze(w, 64); const Pt rnd = pt_from_uniform_bytes(w);
        const int R = 2000; double t0; volatile uint8_t sink = 0;
        { PtFe acc = ptfe_from(rnd); t0 = now(); for (int i = 0; i < R; i++) { g->small_tables[0].accumulate(acc, s); s = fr_add(s, s2); } out[0] = (now() - t0) / R; uint8_t b[32]; pt_encode(b, ptfe_to(acc)); sink ^= b[0]; }
        { uint8_t b[32]; Pt p = rnd; t0 = now(); for (int i = 0; i < R; i++) { pt_encode(b, p); p.X.v[0] ^= b[0] & 1; } out[1] = (now() - t0) / R; sink ^= b[1]; }
        { uint64_t st[25] = {1}; t0 = now(); for (int i = 0; i < 10 * R; i++) keccak_f1600(st); out[2] = (now() - t0) / (10 * R); sink ^= (uint8_t)st[3]; }
        { Transcript tr("bench", 5); uint8_t b[32] = {7}; t0 = now(); for (int i = 0; i < R; i++) { tr.append_point("comm_poly", b); Fr c = tr.challenge_scalar("challenge_nextround"); b[0] ^= (uint8_t)c.v[0]; } out[3] = (now() - t0) / R; sink ^= b[0]; }
        { Fr a = s, b = s2; t0 = now(); for (int i = 0; i < 100 * R; i++) a = fr_mul(a, b); out[4] = (now() - t0) / (100 * R); sink ^= (uint8_t)a.v[0]; }
        { Fr a = s; t0 = now(); for (int i = 0; i < R / 10; i++) a = fr_inv(fr_add(a, s2)); out[5] = (now() - t0) / (R / 10); sink ^= (uint8_t)a.v[0]; }
        {   // hand one empty task to a helper thread and wait for it
            SpinPool::Session session; SpinPool &pool = SpinPool::get();
            out[6] = 0;
            if (pool.workers() > 0) { std::atomic<int> n{0}; std::function<void()> f = [&] { n.fetch_add(1, std::memory_order_relaxed); }; for (int i = 0; i < 100; i++) { pool.submit(0, f); pool.wait(0); }
                t0 = now(); for (int i = 0; i < R; i++) { pool.submit(0, f); pool.wait(0); } out[6] = (now() - t0) / R; }
            // one zero-knowledge sum-check round's host work as the prover runs it (cubic round, 4 coefficients), without a device
            const int rounds = 200;
            Transcript tr("bench", 5); RandomTape tape(w);
            SumcheckState st; sumcheck_draw_tape(st, tape, rounds, 4);
            for (auto &p : st.pre) { Term t = {g->sc_4.h, st.blinds_poly[0]}; p.bp_h = g->commit_terms(&t, 1); p.be_h = p.bp_h; p.rb_h = p.bp_h; p.delta = p.bp_h; p.to_fe(); pt_encode(p.delta_c.b, p.delta); }
            st.claim = s; st.blind_claim = s2; pt_encode(st.comm_claim.b, rnd);
            ZKSumcheckProof pf; pf.comm_polys.resize(rounds); pf.comm_evals.resize(rounds); pf.proofs.resize(rounds);
            double tb = 0, tf = 0;
            for (int j = 0; j < rounds; j++) {
                Fr ev[4] = {s, fr_sub(st.claim, s), s2, fr_mul(s, s2)};
                t0 = now(); RoundPart1 p1 = sumcheck_round_begin(pf, j, ev, 4, st, *g, g->sc_4, tr); tb += now() - t0;
                t0 = now(); sumcheck_round_finish(pf, j, p1, st, *g, g->sc_4, tr); tf += now() - t0;
                s = fr_add(s, p1.r_j);
            }
            out[7] = tb / rounds; out[8] = tf / rounds; out[9] = pool.workers() + 1;
        }
        (void)sink;
        return OTTI_OK;
    });
}

}  // extern "C"
