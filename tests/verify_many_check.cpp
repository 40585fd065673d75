// nizk_verify_many (otti_amd/csrc/verify_many.cpp) against nizk_verify, item by item, on the host alone: own main, host sources only (no HIP, no
// device: every worker evaluates A, B, C on the host), built by tests/test_verify_many_host.py once with -fsanitize=address,undefined and once with
// -fsanitize=thread and run directly.
// usage: verify_many_check <circuit.zkif> <inputs.zkif> <witness.zkif> <label> <proof.bin>...
// Every proof file is one item with the inputs of the inputs file (the caller passes good and tampered proofs); the program adds the first proof
// once more with an input changed, with one input too few and with a non-canonical input.  Workers: 1, 2 and 4, and the list reversed.
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
    // what nizk_verify says about each item alone (a scalar >= l is refused before it, as the C entry refuses it)
    std::vector<int32_t> want(n);
    for (size_t i = 0; i < n; i++) {
        std::vector<Fr> inputs(items[i].ninputs); bool canonical = true;
        for (size_t j = 0; j < items[i].ninputs; j++) canonical = canonical && fr_from_bytes(inputs[j], items[i].inputs.data() + 32 * j);
        want[i] = canonical ? nizk_verify(*I, inputs, *G, label.data(), label.size(), items[i].proof.data(), items[i].proof.size()) : OTTI_ERR_INVALID_SCALAR;
    }
    if (want[0] != OTTI_OK) { fprintf(stderr, "the first proof does not verify\n"); return 3; }
    int mismatches = 0, accepted = 0;
    for (int32_t w : want) accepted += w == OTTI_OK;
    for (int reversed = 0; reversed < 2; reversed++)
        for (unsigned workers : {1u, 2u, 4u}) {
            std::vector<VerifyItem> v(n); std::vector<int32_t> got(n, 12345);
            for (size_t i = 0; i < n; i++) { const Item &it = items[reversed ? n - 1 - i : i]; v[i] = {it.inputs.data(), it.ninputs, it.proof.data(), it.proof.size()}; }
            nizk_verify_many(*I, *G, label.data(), label.size(), v.data(), n, workers, got.data());
            for (size_t i = 0; i < n; i++) {
                const int32_t w = want[reversed ? n - 1 - i : i];
                if (got[i] != w) { mismatches++; fprintf(stderr, "workers %u%s item %zu: got %d want %d\n", workers, reversed ? " reversed" : "", i, got[i], w); }
            }
        }
    {   // one item equals the single call; no items: nothing is touched
        VerifyItem one = {items[0].inputs.data(), items[0].ninputs, items[0].proof.data(), items[0].proof.size()}; int32_t got = 12345;
        nizk_verify_many(*I, *G, label.data(), label.size(), &one, 1, 0, &got);
        if (got != want[0]) { mismatches++; fprintf(stderr, "a list of one: got %d want %d\n", got, want[0]); }
        nizk_verify_many(*I, *G, label.data(), label.size(), nullptr, 0, 4, nullptr);
    }
    otti_r1cs_free(r);
    printf("verify_many_check: %zu items (%d accepted), workers 1 2 4, both orders, %d mismatches\n", n, accepted, mismatches);
    return mismatches ? 4 : 0;
}
