// The device ingest's reader (otti_amd/csrc/zkif_walk.h) as a host program, for the address and undefined-behaviour sanitizers: the functions the
// kernels of k_ingest.hip run — count per constraint, emit per entry, the error keys — run here over .zkif files, in the loaders' shared frame
// (zkif.h), and are compared with zkif_load + instance_new: the same verdict and code for every file, equal lists where both accept.  Every message
// is copied to a heap block of exactly its length rounded up to four bytes (what the walker is allowed to read), so a load out of bounds is a report.
// usage: zkif_walk_check <manifest>      manifest lines:  <tag> <circuit> <inputs> <witness or ->       tag "mutant" lines are counted separately
// Own main, host sources only (linked as tests/san/Makefile links them); never loaded into Python, never run on a GPU.
#include "../otti_amd/csrc/spartan.h"
#include "../otti_amd/csrc/zkif.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using namespace otti;
otti_r1cs *zkif_load_impl(const char *circuit_path, const char *inputs_path, const char *witness_path);
extern "C" void otti_r1cs_free(otti_r1cs *r) { if (!r) return; free(r->A); free(r->B); free(r->C); free(r->vars32); free(r->inputs32); free(r); }

struct Lists { std::vector<uint32_t> row[3], col[3]; std::vector<Fr> val[3]; size_t nc = 0, nv = 0, ni = 0; };

// the walker's pass: what k_ingest.hip does with threads, sequentially
static void walker_pass(const ZkifCircuit &zc, Lists &L) {
    const size_t nvp = next_pow2(std::max(zc.num_vars, zc.num_inputs + 1));
    std::vector<std::vector<uint32_t>> blocks(zc.msgs.size());          // uint32_t: 4-byte aligned, length rounded up to 4 and not a byte more
    std::vector<ZwMsg> msgs = zc.msgs;
    for (size_t j = 0; j < msgs.size(); j++) {
        blocks[j].resize((size_t)(msgs[j].size + 3) / 4);
        memcpy(blocks[j].data(), zc.msgs[j].base, (size_t)msgs[j].size);
        msgs[j].base = reinterpret_cast<const uint8_t *>(blocks[j].data());
    }
    uint64_t err = kZwNoError;
    std::vector<uint32_t> cnt[3]; for (auto &c : cnt) c.assign((size_t)zc.rows, 0);
    for (const ZwMsg &m : msgs)
        for (uint64_t i = 0; i < m.count; i++) {
            Zw z{m.base, m.size, kZwNoError}; uint32_t c3[3];
            zw_count(z, m, i, c3);
            for (int k = 0; k < 3; k++) cnt[k][(size_t)(m.first_row + i)] = c3[k];
            if (z.err < err) err = z.err;
        }
    for (int k = 0; k < 3; k++) {
        uint64_t p = 0;
        for (const ZwMsg &m : msgs)
            for (uint64_t i = 0; i < m.count; i++)
                for (uint64_t e = 0; e < cnt[k][(size_t)(m.first_row + i)]; e++, p++) {
                    Zw z{m.base, m.size, kZwNoError}; uint64_t id; Fr raw = fr_zero(), v = fr_zero(); uint32_t col = 0;
                    if (zw_emit(z, m, i, k, e, id, raw.v)) {
                        col = zw_col(z, zc.col_of, zc.n_ids, id, zc.num_vars, nvp - zc.num_vars, zw_key_parse(m.first_row + i, k, 1, e, 0));
                        if (!fr_raw_is_canonical(raw.v)) z.fail(zw_key_noncanonical(k, p)); else v = fr_mul(raw, fr_R2());
                    } else z.fail(0);                                    // count and emit disagree: sorts first, reported as a mismatch of codes
                    L.row[k].push_back((uint32_t)(m.first_row + i)); L.col[k].push_back(col); L.val[k].push_back(v);
                    if (z.err < err) err = z.err;
                }
    }
    L.nc = (size_t)zc.rows; L.nv = zc.num_vars; L.ni = zc.num_inputs;
    if (err != kZwNoError) throw Error(zw_key_code(err), "walker refused");
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <manifest>\n", argv[0]); return 2; }
    FILE *mf = fopen(argv[1], "r"); if (!mf) { perror(argv[1]); return 2; }
    char tag[64], c[4096], i[4096], w[4096];
    int files = 0, mismatches = 0, refused[2] = {0, 0}, accepted[2] = {0, 0};
    while (fscanf(mf, "%63s %4095s %4095s %4095s", tag, c, i, w) == 4) {
        const char *wp = strcmp(w, "-") ? w : nullptr; const int mutant = !strcmp(tag, "mutant");
        int host_code = 0, walk_code = 0; Lists H, W;
        try {
            otti_r1cs *r = zkif_load_impl(c, i, wp);
            struct Guard { otti_r1cs *r; ~Guard() { otti_r1cs_free(r); } } guard{r};
            auto I = instance_new(r->num_cons, r->num_vars, r->num_inputs, r->A, r->nA, r->B, r->nB, r->C, r->nC);
            for (int k = 0; k < 3; k++) { H.row[k] = I->mat(k).row; H.col[k] = I->mat(k).col; H.val[k] = I->mat(k).val; }
            H.nc = r->num_cons; H.nv = r->num_vars; H.ni = r->num_inputs;
        } catch (const Error &e) { host_code = e.code; }
        try {
            otti_r1cs *r = zkif_load_with(c, i, wp, [&](const ZkifCircuit &zc, otti_r1cs *, const ZkifLap &) { walker_pass(zc, W); });
            otti_r1cs_free(r);
        } catch (const Error &e) { walk_code = e.code; }
        bool same = host_code == walk_code;
        if (same && !host_code) {
            same = H.nc == W.nc && H.nv == W.nv && H.ni == W.ni;
            for (int k = 0; k < 3 && same; k++)
                same = H.row[k] == W.row[k] && H.col[k] == W.col[k] && H.val[k].size() == W.val[k].size() &&
                       (H.val[k].empty() || !memcmp(H.val[k].data(), W.val[k].data(), H.val[k].size() * sizeof(Fr)));
        }
        files++; (host_code ? refused : accepted)[mutant]++;
        if (!same) { mismatches++; printf("MISMATCH %s %s: host %d, walker %d\n", tag, c, host_code, walk_code); }
        else printf("%s %s %d\n", tag, c, host_code);
    }
    fclose(mf);
    printf("cases: %d refused, %d accepted\nmutants: %d refused, %d accepted\n%d files, %d mismatches\n", refused[0], accepted[0], refused[1], accepted[1], files, mismatches);
    return mismatches ? 1 : 0;
}
