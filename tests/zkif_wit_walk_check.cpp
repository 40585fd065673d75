// The witness ingest's reader (otti_amd/csrc/zkif_wit_walk.h) as a host program, for the address and undefined-behaviour sanitizers: what the
// kernel of k_wit_ingest.hip does with a thread per assigned variable — read id and value, map the id, mark the bitmap, judge the value, record the
// smallest error key — done here sequentially, in the device loader's frame (zkif.h zkif_witness_with), and compared with the host pair: zkif_load
// on the three files, then the upload's checks (a public input >= l, then a witness value >= l).  The same verdict and code for every file, the
// same assignment where both accept.  The two-file host loader (zkif_load_assignment) is held against the same reference.  Every message is copied
// to a heap block of exactly its length rounded up to four bytes (what the reader is allowed to load), so a load out of bounds is a report.
// usage: zkif_wit_walk_check <manifest>     manifest lines:  <tag> <circuit> <inputs> <witness> <num_vars or -> <num_inputs or ->
//        the last two: the dimensions of the instance the witness is for.  tag "mutant" lines are counted separately; on a "dims" line the files are
//        sound and of OTHER dimensions: the host pair accepts them and both loaders must say OTTI_ERR_BAD_ARG.
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

struct Assignment { std::vector<uint8_t> vars, inputs; };

// the upload's checks behind a loader: the public inputs first, then the variables
static void upload_checks(const otti_r1cs *r, Assignment &a) {
    Fr x;
    for (size_t i = 0; i < r->ninputs; i++) if (!fr_from_bytes(x, r->inputs32 + 32 * i)) throw Error(OTTI_ERR_INVALID_SCALAR, "non-canonical input");
    for (size_t i = 0; i < r->nvars; i++) if (!fr_from_bytes(x, r->vars32 + 32 * i)) throw Error(OTTI_ERR_INVALID_SCALAR, "non-canonical variable");
    a.vars.assign(r->vars32, r->vars32 + 32 * r->nvars); a.inputs.assign(r->inputs32, r->inputs32 + 32 * r->ninputs);
}

// the kernel's work, sequentially
static void reader_pass(const ZkifWitness &zw, Assignment &a) {
    std::vector<std::vector<uint32_t>> blocks(zw.msgs.size());
    std::vector<WwMsg> msgs = zw.msgs;
    for (size_t j = 0; j < msgs.size(); j++) {
        blocks[j].resize((size_t)(msgs[j].size + 3) / 4);
        memcpy(blocks[j].data(), zw.msgs[j].base, (size_t)msgs[j].size);
        msgs[j].base = reinterpret_cast<const uint8_t *>(blocks[j].data());
    }
    const size_t nvars = zw.have_witness ? zw.num_vars : 0;
    std::vector<uint32_t> seen((zw.num_vars + 31) / 32, 0);
    a.vars.assign(32 * nvars, 0); a.inputs = zw.inputs32;
    uint64_t err = zw.seed, p = 0;
    for (size_t j = 0; j < msgs.size(); j++)
        for (uint64_t i = 0; i < msgs[j].count; i++, p++) {
            const WwMsg &w = msgs[j];
            Zw z{w.base, w.size, kZwNoError}; uint64_t id; Fr raw = fr_zero();
            if (w.first + i != p) z.fail(0);                     // the prefix of the counts is wrong: sorts first, reported as a mismatch of codes
            ww_elem(z, w, j, i, id, raw.v);
            const uint32_t col = ww_col(z, zw.inst_sorted.data(), zw.inst_sorted.size(), id, zw.num_vars, ww_key(WW_INDEX, p));
            if (!fr_raw_is_canonical(raw.v)) z.fail(ww_key(WW_SCALAR, 1 + p));
            if (col != 0xffffffffu) {
                const uint32_t bit = 1u << (col & 31);
                if (seen[col >> 5] & bit) z.fail(ww_key(WW_TWICE, 0));
                else { seen[col >> 5] |= bit; memcpy(a.vars.data() + 32 * (size_t)col, raw.v, 32); }
            }
            if (z.err < err) err = z.err;
        }
    if (p != zw.total) err = 0;
    if (err != kZwNoError) zkif_witness_refuse(zw, err);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <manifest>\n", argv[0]); return 2; }
    FILE *mf = fopen(argv[1], "r"); if (!mf) { perror(argv[1]); return 2; }
    char tag[64], c[4096], i[4096], w[4096], nv[64], ni[64];
    int files = 0, mismatches = 0, refused[2] = {0, 0}, accepted[2] = {0, 0};
    while (fscanf(mf, "%63s %4095s %4095s %4095s %63s %63s", tag, c, i, w, nv, ni) == 6) {
        const int mutant = !strcmp(tag, "mutant"), dims = !strcmp(tag, "dims");
        size_t want[2] = {0, 0}; const bool have_want = strcmp(nv, "-") != 0;
        if (have_want) { want[0] = (size_t)strtoull(nv, nullptr, 10); want[1] = (size_t)strtoull(ni, nullptr, 10); }
        int code[3] = {0, 0, 0}; Assignment A[3];
        try {
            otti_r1cs *r = zkif_load_impl(c, i, w);
            struct Guard { otti_r1cs *r; ~Guard() { otti_r1cs_free(r); } } guard{r};
            upload_checks(r, A[0]);
        } catch (const Error &e) { code[0] = e.code; }
        try {
            otti_r1cs *r = zkif_load_assignment(i, w, have_want ? want : nullptr);
            struct Guard { otti_r1cs *r; ~Guard() { otti_r1cs_free(r); } } guard{r};
            upload_checks(r, A[1]);
        } catch (const Error &e) { code[1] = e.code; }
        try { zkif_witness_with(i, w, have_want ? want : nullptr, [&](const ZkifWitness &zw) { reader_pass(zw, A[2]); }); } catch (const Error &e) { code[2] = e.code; }
        bool same;
        if (dims) same = code[0] == 0 && code[1] == OTTI_ERR_BAD_ARG && code[2] == OTTI_ERR_BAD_ARG;
        else {
            same = code[1] == code[0] && code[2] == code[0];
            if (same && !code[0]) same = A[1].vars == A[0].vars && A[2].vars == A[0].vars && A[1].inputs == A[0].inputs && A[2].inputs == A[0].inputs;
        }
        const int shown = dims ? code[2] : code[0];
        files++; (shown ? refused : accepted)[mutant]++;
        if (!same) { mismatches++; printf("MISMATCH %s %s: host pair %d, two-file loader %d, reader %d\n", tag, w, code[0], code[1], code[2]); }
        else printf("%s %s %d\n", tag, w, shown);
    }
    fclose(mf);
    printf("cases: %d refused, %d accepted\nmutants: %d refused, %d accepted\n%d files, %d mismatches\n", refused[0], accepted[0], refused[1], accepted[1], files, mismatches);
    return mismatches ? 1 : 0;
}
