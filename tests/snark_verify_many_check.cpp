// snark_verify_many (otti_amd/csrc/snark_verify_many.cpp) against snark_verify, item by item, on the host alone: own main, host sources only (no HIP,
// no device: every row sum is summed on the host), built by tests/test_snark_verify_many_host.py once with -fsanitize=address,undefined and once
// with -fsanitize=thread and run directly.
// usage: snark_verify_many_check <commitment.bin> <inputs.bin> <num_nz_entries> <label> <proof.bin>...
// Every proof file is one item with the inputs of the inputs file (32 canonical bytes each; the caller passes good and tampered proofs); the program
// adds the first proof once more with an input changed, with one input too few and with a non-canonical input.  Three checks:
//   * the four steps of EvalProofVerifier in sequence with host sums give snark_verify's code on every item, and a decompress failure handed to a
//     step comes out of it as the verdict;
//   * snark_verify_many with workers 1, 2 and 4, both orders, a list of one and an empty list: 0 mismatches;
//   * the peak number of threads of the process during a call with 4 items (highest of six such calls) and with 24 items at two workers is the same.
#include "../otti_amd/csrc/snark.h"
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

using namespace otti;
extern "C" void otti_r1cs_free(otti_r1cs *r) { if (!r) return; free(r->A); free(r->B); free(r->C); free(r->vars32); free(r->inputs32); free(r); }   // zkif.cpp's, unused here

static std::vector<uint8_t> slurp(const char *p) {
    FILE *f = fopen(p, "rb"); if (!f) { perror(p); exit(2); }
    std::vector<uint8_t> d; uint8_t b[4096]; size_t k; while ((k = fread(b, 1, sizeof b, f)) > 0) d.insert(d.end(), b, b + k); fclose(f); return d;
}
struct Item { std::vector<uint8_t> inputs, proof; size_t ninputs; };

// snark_verify's walk with the evaluation proof taken step by step and every sum made on the host
static int verify_by_steps(const CompComm &comm, const std::vector<Fr> &inputs, const SnarkGens &g, const std::string &label, const std::vector<uint8_t> &proof, int fail_at) {
    try {
        if (inputs.size() != comm.num_inputs) return OTTI_ERR_INVALID_NUM_INPUTS;
        if (comm.num_cons != g.num_cons || comm.num_vars != g.num_vars) return OTTI_ERR_VERIFY_INTERNAL;
        SnarkProof S = SnarkProof::parse(proof.data(), proof.size());
        Transcript tr(label.data(), label.size());
        tr.append_protocol_name("Spartan SNARK proof");
        snark_append_comm(tr, comm);
        std::vector<Fr> rx, ry;
        if (int rc = r1cs_verify_host(S.r1cs, comm.num_cons, comm.num_vars, inputs, S.inst_evals, *g.sat, tr, rx, ry)) return rc;
        tr.append_scalar("Ar_claim", S.inst_evals[0]); tr.append_scalar("Br_claim", S.inst_evals[1]); tr.append_scalar("Cr_claim", S.inst_evals[2]);
        EvalProofVerifier v(S.eval, comm, rx, ry, S.inst_evals, g, tr, 0);
        auto answer = [&](const RowRequest &q, int seam) {
            RowAnswer a; a.sum = pt_identity();
            if (seam == fail_at) { a.code = OTTI_ERR_VERIFY_DECOMPRESS; return a; }
            try { a.sum = row_sum_on_host(q.C, q.n, q.s, false); } catch (const VerifyFail &f) { a.code = f.code; }
            return a;
        };
        RowRequest q = v.begin();
        q = v.after_derefs(answer(q, 0));
        q = v.after_ops(answer(q, 1));
        v.after_mem(answer(q, 2));
        return OTTI_OK;
    } catch (const VerifyFail &f) { return f.code; }
    catch (const Error &e) { return e.code; }
}
static size_t tasks_now() {
    size_t n = 0; DIR *d = opendir("/proc/self/task"); if (!d) return 0;
    while (struct dirent *e = readdir(d)) if (e->d_name[0] != '.') n++;
    closedir(d); return n;
}

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s commitment.bin inputs.bin num_nz_entries label proof.bin...\n", argv[0]); return 2; }
    const std::vector<uint8_t> cb = slurp(argv[1]), in32 = slurp(argv[2]);
    const std::string label = argv[4];
    auto comm = CompComm::parse(cb.data(), cb.size());
    auto G = snark_gens_new(comm->num_cons, comm->num_vars, comm->num_inputs, strtoull(argv[3], nullptr, 10));
    const size_t ninputs = in32.size() / 32;
    std::vector<Item> items;
    for (int a = 5; a < argc; a++) items.push_back({in32, slurp(argv[a]), ninputs});
    if (ninputs) {
        Item changed = items[0]; changed.inputs[0] ^= 1; items.push_back(changed);
        Item fewer = items[0]; fewer.ninputs--; items.push_back(fewer);
        Item wide = items[0]; for (int k = 0; k < 32; k++) wide.inputs[k] = 0xff; items.push_back(wide);
    }
    const size_t n = items.size();
    // what snark_verify says about each item alone (a scalar >= l is refused before it, as the C entry refuses it), and the same walk by steps
    std::vector<int32_t> want(n);
    int mismatches = 0, accepted = 0;
    for (size_t i = 0; i < n; i++) {
        std::vector<Fr> inputs(items[i].ninputs); bool canonical = true;
        for (size_t j = 0; j < items[i].ninputs; j++) canonical = canonical && fr_from_bytes(inputs[j], items[i].inputs.data() + 32 * j);
        want[i] = canonical ? snark_verify(*comm, inputs, *G, label.data(), label.size(), items[i].proof.data(), items[i].proof.size()) : OTTI_ERR_INVALID_SCALAR;
        if (!canonical) continue;
        const int got = verify_by_steps(*comm, inputs, *G, label, items[i].proof, -1);
        if (got != want[i]) { mismatches++; fprintf(stderr, "steps, item %zu: got %d want %d\n", i, got, want[i]); }
    }
    if (want[0] != OTTI_OK) { fprintf(stderr, "the first proof does not verify\n"); return 3; }
    for (int seam = 0; seam < 3; seam++) {                            // a good proof whose sum at this seam is answered with the decompress failure
        std::vector<Fr> inputs(ninputs); for (size_t j = 0; j < ninputs; j++) fr_from_bytes(inputs[j], in32.data() + 32 * j);
        const int got = verify_by_steps(*comm, inputs, *G, label, items[0].proof, seam);
        if (got != OTTI_ERR_VERIFY_DECOMPRESS) { mismatches++; fprintf(stderr, "steps, decompress failure at seam %d: got %d\n", seam, got); }
    }
    for (int32_t w : want) accepted += w == OTTI_OK;
    for (int reversed = 0; reversed < 2; reversed++)
        for (unsigned workers : {1u, 2u, 4u}) {
            std::vector<VerifyItem> v(n); std::vector<int32_t> got(n, 12345);
            for (size_t i = 0; i < n; i++) { const Item &it = items[reversed ? n - 1 - i : i]; v[i] = {it.inputs.data(), it.ninputs, it.proof.data(), it.proof.size()}; }
            snark_verify_many(*comm, *G, label.data(), label.size(), v.data(), n, workers, got.data());
            for (size_t i = 0; i < n; i++) {
                const int32_t w = want[reversed ? n - 1 - i : i];
                if (got[i] != w) { mismatches++; fprintf(stderr, "workers %u%s item %zu: got %d want %d\n", workers, reversed ? " reversed" : "", i, got[i], w); }
            }
        }
    {   // one item equals the single call; no items: nothing is touched
        VerifyItem one = {items[0].inputs.data(), items[0].ninputs, items[0].proof.data(), items[0].proof.size()}; int32_t got = 12345;
        snark_verify_many(*comm, *G, label.data(), label.size(), &one, 1, 0, &got);
        if (got != want[0]) { mismatches++; fprintf(stderr, "a list of one: got %d want %d\n", got, want[0]); }
        snark_verify_many(*comm, *G, label.data(), label.size(), nullptr, 0, 4, nullptr);
    }
    // threads do not grow with the number of proofs: the peak of /proc/self/task, sampled all through a call, for 4 and for 24 good items at two workers.
    // What moves during a call are the helper threads r1cs_verify_host starts and joins per proof; the peak is reached when both workers have
    // theirs at once, which a call of four proofs may be too short to show: it is made six times (as many proofs as the long call walks) and its
    // peak is the highest of them.  A proof that kept a thread while parked would show as 24 against 4.
    size_t peak[2] = {0, 0};
    const size_t counts[2] = {4, 24}, calls[2] = {6, 1};
    for (int k = 0; k < 2; k++) {
        std::vector<VerifyItem> v(counts[k], VerifyItem{items[0].inputs.data(), items[0].ninputs, items[0].proof.data(), items[0].proof.size()});
        for (size_t rep = 0; rep < calls[k]; rep++) {
            std::vector<int32_t> got(counts[k], 12345);
            std::atomic<bool> stop{false}; std::atomic<size_t> top{0};
            std::thread sampler([&] { while (!stop.load(std::memory_order_acquire)) { const size_t t = tasks_now(); if (t > top.load()) top.store(t); } });
            snark_verify_many(*comm, *G, label.data(), label.size(), v.data(), counts[k], 2, got.data());
            stop.store(true, std::memory_order_release); sampler.join();
            peak[k] = std::max(peak[k], top.load());
            for (int32_t r : got) if (r != OTTI_OK) { mismatches++; fprintf(stderr, "%zu good items: a result of %d\n", counts[k], r); }
        }
    }
    if (peak[0] != peak[1] || !peak[0]) { mismatches++; fprintf(stderr, "peak threads: %zu with 4 items, %zu with 24\n", peak[0], peak[1]); }
    printf("snark_verify_many_check: %zu items (%d accepted), steps, workers 1 2 4, both orders, peak threads %zu / %zu, %d mismatches\n", n, accepted, peak[0], peak[1], mismatches);
    return mismatches ? 4 : 0;
}
