// prove_many_plan.h swept on the host (own main, the header alone): batches of 0 .. 40 witnesses, every has-rows / has-products / sparse pattern of
// up to six, L over 1 .. 2^12 and budgets from nothing to plenty.  Every plan must cover the batch in order with chunks of at most 16, put a
// witness lacking a thing into exactly one tile / job of its chunk — or into none where fewer than two of the chunk lack it — keep tiles to four
// witnesses and jobs to 65535 rows of one MSM variant, and charge no chunk more than the budget; no budget, no front half.
#include "prove_many_plan.h"
#include <cstdio>
#include <cstdlib>

using namespace otti;

static long g_plans = 0, g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static void check(size_t K, size_t N, size_t V, size_t L, const std::vector<PmWitness> &w, uint64_t budget) {
    const PmPlan p = prove_many_plan(K, N, V, L, V / L, w.data(), budget);
    g_plans++;
    size_t at = 0;
    std::vector<int> in_tile(K, 0), in_job(K, 0);
    for (const PmChunk &c : p.chunks) {
        CHECK(c.first == at && c.count >= 1 && c.count <= kProveManyChunk, "chunk at %zu + %zu, expected at %zu", c.first, c.count, at);
        at = c.first + c.count;
        size_t lack_p = 0, lack_r = 0;
        for (size_t i = c.first; i < c.first + c.count && i < K; i++) { lack_p += !w[i].has_products; lack_r += !w[i].has_rows; }
        size_t np = 0, nr = 0;
        for (const PmTile &t : c.tiles) {
            CHECK(t.wit.size() >= 1 && t.wit.size() <= kProveManyTile, "a tile of %zu", t.wit.size());
            for (uint32_t i : t.wit) { CHECK(i >= c.first && i < c.first + c.count && !w[i].has_products, "witness %u in a tile of chunk %zu", i, c.first); if (i < K) in_tile[i]++; np++; }
        }
        for (const PmRowJob &j : c.jobs) {
            CHECK(j.rows == j.wit.size() * L && j.rows >= 1 && j.rows <= kProveManyJobRows, "a job of %zu rows", j.rows);
            for (uint32_t i : j.wit) { CHECK(i >= c.first && i < c.first + c.count && !w[i].has_rows && w[i].sparse == j.sparse, "witness %u in a job of chunk %zu", i, c.first); if (i < K) in_job[i]++; nr++; }
        }
        // all of a chunk's lacking witnesses, or none of them: none only under the fewer-than-two rule
        CHECK(np == (lack_p >= 2 ? lack_p : 0), "chunk %zu: %zu of %zu witnesses lacking products are in tiles", c.first, np, lack_p);
        CHECK(nr == (lack_r >= 2 ? lack_r : 0), "chunk %zu: %zu of %zu witnesses lacking rows are in jobs", c.first, nr, lack_r);
        const uint64_t bytes = np * 96 * (uint64_t)N + (np ? 4 * 2 * (uint64_t)V * 32 : 0) + nr * (128 * (uint64_t)L + 32 * (uint64_t)V);
        CHECK(c.bytes == bytes && bytes <= budget, "chunk %zu charges %llu (plan says %llu) of %llu", c.first, (unsigned long long)bytes, (unsigned long long)c.bytes, (unsigned long long)budget);
        if (!budget) CHECK(c.tiles.empty() && c.jobs.empty(), "a front half without a budget");
    }
    CHECK(at == K, "chunks end at %zu of %zu", at, K);
    for (size_t i = 0; i < K; i++) CHECK(in_tile[i] <= 1 && in_job[i] <= 1, "witness %zu in %d tiles, %d jobs", i, in_tile[i], in_job[i]);
}

int main() {
    uint64_t seed = 88172645463325252ull;
    auto rnd = [&] { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    const size_t Ls[] = {1, 2, 8, 64, 1024, 4096};
    for (size_t L : Ls) {
        const size_t V = L * L, N = V;
        const uint64_t one = 96 * (uint64_t)N + 128 * (uint64_t)L + 32 * (uint64_t)V, tile = 256 * (uint64_t)V;
        const uint64_t budgets[] = {0, 1, one, tile + 2 * one - 1, tile + 2 * one, tile + 3 * one + 5, tile + 16 * one, tile + 17 * one, (uint64_t)8 << 30, ~(uint64_t)0 >> 1};
        for (uint64_t budget : budgets) {
            // every pattern of up to six witnesses at L = 8 (six under three of the budgets, five under all); of up to four at the other sizes,
            // where only the byte counts differ
            const bool six = budget == 0 || budget == tile + 3 * one + 5 || budget == (uint64_t)8 << 30;
            for (size_t K = 0; K <= (L != 8 ? 4u : six ? 6u : 5u); K++)
                for (unsigned pat = 0; pat < (1u << (3 * K)); pat++) {
                    std::vector<PmWitness> w(K);
                    for (size_t i = 0; i < K; i++) { w[i].has_rows = (pat >> (3 * i)) & 1; w[i].has_products = (pat >> (3 * i + 1)) & 1; w[i].sparse = (pat >> (3 * i + 2)) & 1; }
                    check(K, N, V, L, w, budget);
                }
            // longer batches: nothing kept, everything kept, and random flags
            for (size_t K = 7; K <= 40; K++)
                for (int kind = 0; kind < 4; kind++) {
                    std::vector<PmWitness> w(K);
                    for (size_t i = 0; i < K; i++) {
                        const uint64_t r = rnd();
                        w[i].has_rows = kind == 1 || (kind >= 2 && (r & 1)); w[i].has_products = kind == 1 || (kind >= 2 && (r & 2)); w[i].sparse = kind == 3 && (r & 4);
                    }
                    check(K, N, V, L, w, budget);
                }
        }
    }
    {   // the shapes the GPU tests count on: sixteen witnesses of 2^12 variables that keep nothing are one chunk, four tiles, one job of 1024 rows
        std::vector<PmWitness> w(18);
        PmPlan p = prove_many_plan(16, 4096, 4096, 64, 64, w.data(), (uint64_t)8 << 30);
        CHECK(p.chunks.size() == 1 && p.chunks[0].tiles.size() == 4 && p.chunks[0].jobs.size() == 1 && p.chunks[0].jobs[0].rows == 1024, "sixteen of 2^12");
        p = prove_many_plan(18, 64, 64, 8, 8, w.data(), (uint64_t)8 << 30);
        CHECK(p.chunks.size() == 2 && p.chunks[0].count == 16 && p.chunks[1].count == 2 && p.chunks[1].tiles.size() == 1 && p.chunks[1].jobs.size() == 1, "eighteen of 2^6");
        for (int i = 0; i < 16; i++) w[i].sparse = i < 8;
        p = prove_many_plan(16, 8192, 8192, 64, 128, w.data(), (uint64_t)8 << 30);
        CHECK(p.chunks.size() == 1 && p.chunks[0].jobs.size() == 2 && !p.chunks[0].jobs[0].sparse && p.chunks[0].jobs[1].sparse && p.chunks[0].jobs[0].rows == 512, "two variants of 2^13");
        g_plans += 3;
    }
    printf("%ld plans checked, %ld failures\n", g_plans, g_fail);
    return g_fail ? 1 : 0;
}
