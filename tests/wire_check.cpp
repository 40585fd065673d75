// The wire code (otti_amd/csrc/wire.cpp) on its own: own main, host sources only, built by tests/test_wire_host.py with
// -fsanitize=address,undefined and run directly.
// usage: wire_check <manifest>      lines:  roundtrip <nizk|snark|comm> <file>   |   refuse <nizk|snark|comm> <file>
// roundtrip: the file parses and serialises back to the same bytes; every proper prefix of it, and the file with one byte appended, is refused
//            as malformed.  Each attempt is parsed from a heap block of exactly its length, so a read past the end is the sanitizer's to report.
// refuse:    the file (a count set past its bound) is refused as malformed, and no single allocation on the way exceeds kRefuseMaxAlloc: the
//            reader checks a count before it makes room for it.
#include "../otti_amd/csrc/snark.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using namespace otti;
extern "C" void otti_r1cs_free(otti_r1cs *r) { if (!r) return; free(r->A); free(r->B); free(r->C); free(r->vars32); free(r->inputs32); free(r); }   // zkif.cpp's, unused here

// the address sanitizer's allocator interface (sanitizer/allocator_interface.h, declared here: the header is not installed everywhere)
extern "C" int __sanitizer_install_malloc_and_free_hooks(void (*malloc_hook)(const volatile void *, size_t), void (*free_hook)(const volatile void *));
static size_t g_peak_alloc = 0;                             // the largest single request since it was last cleared, as the sanitizer's allocator reports it
static void on_malloc(const volatile void *, size_t n) { if (n > g_peak_alloc) g_peak_alloc = n; }
static void on_free(const volatile void *) {}
constexpr size_t kRefuseMaxAlloc = (size_t)1 << 20;          // the smallest bound + 1 that matters claims 32 MiB

static std::vector<uint8_t> slurp(const char *p) {
    FILE *f = fopen(p, "rb"); if (!f) { perror(p); exit(2); }
    std::vector<uint8_t> d; uint8_t b[4096]; size_t k; while ((k = fread(b, 1, sizeof b, f)) > 0) d.insert(d.end(), b, b + k); fclose(f); return d;
}
// 0 and the bytes the parsed object serialises to, or the code the parser refused the input with
static int parse(const std::string &kind, const uint8_t *p, size_t n, std::vector<uint8_t> *again) {
    try {
        std::vector<uint8_t> out;
        if (kind == "nizk") out = NizkProof::parse(p, n).serialize();
        else if (kind == "snark") out = SnarkProof::parse(p, n).serialize();
        else out = CompComm::parse(p, n)->serialize();
        if (again) *again = std::move(out);
        return 0;
    } catch (const Error &e) { return e.code; }
}
// the same from a heap block of exactly n bytes
static int parse_exact(const std::string &kind, const uint8_t *p, size_t n, std::vector<uint8_t> *again = nullptr) {
    uint8_t *q = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(q, p, n);
    const int rc = parse(kind, n ? q : q + 1, n, again);     // n == 0: a pointer with nothing readable behind it
    free(q);
    return rc;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s manifest\n", argv[0]); return 2; }
    FILE *mf = fopen(argv[1], "r"); if (!mf) { perror(argv[1]); return 2; }
    if (!__sanitizer_install_malloc_and_free_hooks(on_malloc, on_free)) { fprintf(stderr, "no allocation hook\n"); return 2; }
    char what[16], kind[16], path[4096];
    int bad = 0; size_t files = 0, prefixes = 0, refused = 0;
    while (fscanf(mf, "%15s %15s %4095s", what, kind, path) == 3) {
        const std::vector<uint8_t> b = slurp(path);
        files++;
        if (!strcmp(what, "refuse")) {
            g_peak_alloc = 0;
            const int rc = parse_exact(kind, b.data(), b.size());
            const size_t peak = g_peak_alloc;
            if (rc != OTTI_ERR_MALFORMED_PROOF || peak > kRefuseMaxAlloc) { bad++; printf("refuse %s: code %d, largest allocation %zu\n", path, rc, peak); }
            else refused++;
            continue;
        }
        std::vector<uint8_t> again;
        g_peak_alloc = 0;
        int rc = parse_exact(kind, b.data(), b.size(), &again);
        if (g_peak_alloc < b.size()) { bad++; printf("roundtrip %s: the allocation hook saw at most %zu bytes\n", path, g_peak_alloc); }   // the copy alone is that large
        if (rc != 0 || again != b) { bad++; printf("roundtrip %s: code %d, %zu bytes back of %zu\n", path, rc, again.size(), b.size()); continue; }
        for (size_t k = 0; k < b.size(); k++) {
            prefixes++;
            if ((rc = parse_exact(kind, b.data(), k)) != OTTI_ERR_MALFORMED_PROOF) { bad++; printf("prefix %zu of %s: code %d\n", k, path, rc); }
        }
        std::vector<uint8_t> longer = b; longer.push_back(0);
        if ((rc = parse_exact(kind, longer.data(), longer.size())) != OTTI_ERR_MALFORMED_PROOF) { bad++; printf("appended byte, %s: code %d\n", path, rc); }
    }
    fclose(mf);
    printf("wire_check: %zu files, %zu prefixes, %zu counts past their bound refused, %d failures\n", files, prefixes, refused, bad);
    return bad ? 4 : 0;
}
