// nizk_verify_batch (otti_amd/csrc/verify_batch.cpp) against nizk_verify, item by item, on the host alone: own main, host sources only (no HIP, no
// device: the sum runs on the host cores), built by tests/test_verify_batch_host.py once with -fsanitize=address,undefined and once with
// -fsanitize=thread and run directly.
// usage: verify_batch_host_check <circuit.zkif> <inputs.zkif> <witness.zkif> <label> <proof.bin>...
// Every proof file is one item with the inputs of the inputs file (the caller passes good and tampered proofs); the program adds the first proof
// once more with an input changed, with one input too few and with a non-canonical input.  Workers: 1, 2 and 4, and the list reversed; OS entropy
// and a seed; the good proofs alone (one sum, nothing rerun).
#include "../otti_amd/csrc/spartan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

using namespace otti;
otti_r1cs *zkif_load_impl(const char *circuit_path, const char *inputs_path, const char *witness_path);
extern "C" void otti_r1cs_free(otti_r1cs *r) { if (!r) return; free(r->A); free(r->B); free(r->C); free(r->vars32); free(r->inputs32); free(r); }

static std::vector<uint8_t> slurp(const char *p) {
    FILE *f = fopen(p, "rb"); if (!f) { perror(p); exit(2); }
    std::vector<uint8_t> d; uint8_t b[4096]; size_t k; while ((k = fread(b, 1, sizeof b, f)) > 0) d.insert(d.end(), b, b + k); fclose(f); return d;
}
struct Item { std::vector<uint8_t> inputs, proof; size_t ninputs; };

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s c.zkif i.zkif w.zkif label proof.bin...\n", argv[0]); return 2; }
    const std::string label = argv[4];
    otti_r1cs *r = zkif_load_impl(argv[1], argv[2], argv[3]);
    auto I = instance_new(r->num_cons, r->num_vars, r->num_inputs, r->A, r->nA, r->B, r->nB, r->C, r->nC);
    auto G = gens_new(r->num_cons, r->num_vars, r->num_inputs);
    const std::vector<uint8_t> in32(r->inputs32, r->inputs32 + 32 * r->ninputs);
    std::vector<Item> items;
    for (int a = 5; a < argc; a++) items.push_back({in32, slurp(argv[a]), r->ninputs});
    if (r->ninputs) {
        Item changed = items[0]; changed.inputs[0] ^= 1; items.push_back(changed);
        Item fewer = items[0]; fewer.ninputs--; items.push_back(fewer);
        Item wide = items[0]; for (int k = 0; k < 32; k++) wide.inputs[k] = 0xff; items.push_back(wide);
    }
    const size_t n = items.size();
    std::vector<int32_t> want(n);
    for (size_t i = 0; i < n; i++) {
        std::vector<Fr> inputs(items[i].ninputs); bool canonical = true;
        for (size_t j = 0; j < items[i].ninputs; j++) canonical = canonical && fr_from_bytes(inputs[j], items[i].inputs.data() + 32 * j);
        want[i] = canonical ? nizk_verify(*I, inputs, *G, label.data(), label.size(), items[i].proof.data(), items[i].proof.size()) : OTTI_ERR_INVALID_SCALAR;
    }
    if (want[0] != OTTI_OK) { fprintf(stderr, "the first proof does not verify\n"); return 3; }
    int mismatches = 0, accepted = 0;
    for (int32_t w : want) accepted += w == OTTI_OK;
    uint8_t seed[32]; for (int k = 0; k < 32; k++) seed[k] = (uint8_t)(3 * k + 1);
    for (int reversed = 0; reversed < 2; reversed++)
        for (unsigned workers : {1u, 2u, 4u}) {
            std::vector<VerifyItem> v(n); std::vector<int32_t> got(n, 12345);
            for (size_t i = 0; i < n; i++) { const Item &it = items[reversed ? n - 1 - i : i]; v[i] = {it.inputs.data(), it.ninputs, it.proof.data(), it.proof.size()}; }
            otti_verify_batch_info info;
            nizk_verify_batch(*I, *G, label.data(), label.size(), v.data(), n, workers, reversed ? seed : nullptr, got.data(), &info);
            for (size_t i = 0; i < n; i++) {
                const int32_t w = want[reversed ? n - 1 - i : i];
                if (got[i] != w) { mismatches++; fprintf(stderr, "workers %u%s item %zu: got %d want %d\n", workers, reversed ? " reversed" : "", i, got[i], w); }
            }
            if (info.on_device || info.accepted_first_pass || !info.equations) { mismatches++; fprintf(stderr, "workers %u: a list with bad proofs accepted in one pass, or on a device\n", workers); }
        }
    {   // the good proofs alone: one sum, nothing rerun; one item equals the single call; no items: nothing is touched
        std::vector<VerifyItem> v; for (size_t i = 0; i < n; i++) if (want[i] == OTTI_OK) v.push_back({items[i].inputs.data(), items[i].ninputs, items[i].proof.data(), items[i].proof.size()});
        std::vector<int32_t> got(v.size(), 12345); otti_verify_batch_info info;
        nizk_verify_batch(*I, *G, label.data(), label.size(), v.data(), v.size(), 0, nullptr, got.data(), &info);
        for (int32_t g : got) if (g != OTTI_OK) { mismatches++; fprintf(stderr, "a good proof among good ones: got %d\n", g); }
        if (!info.accepted_first_pass || info.singles_rerun || info.localise_passes) { mismatches++; fprintf(stderr, "good proofs took more than one sum\n"); }
        int32_t one = 12345;
        nizk_verify_batch(*I, *G, label.data(), label.size(), v.data(), 1, 0, nullptr, &one, nullptr);
        if (one != want[0]) { mismatches++; fprintf(stderr, "a list of one: got %d want %d\n", one, want[0]); }
        nizk_verify_batch(*I, *G, label.data(), label.size(), nullptr, 0, 4, nullptr, nullptr, nullptr);
    }
    otti_r1cs_free(r);
    printf("verify_batch_host_check: %zu items (%d accepted), workers 1 2 4, both orders, %d mismatches\n", n, accepted, mismatches);
    return mismatches ? 4 : 0;
}
