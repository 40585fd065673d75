// The front half of nizk_prove_many (prove_many.cpp), planned: which witnesses of a batch have their witness-only work — the unblinded row sums of
// the commitment, and Az, Bz, Cz — formed in joint passes, and how those passes are cut.  Pure arithmetic over the batch's sizes and three flags
// per witness — standard library only, so a host compiler can run it without HIP (tests/prove_many_plan_check.cpp sweeps it).
//   chunks     consecutive witnesses, at most kProveManyChunk, whose front buffers are resident together; the byte budget cuts them shorter.  Charged:
//              96 N per witness lacking products (Az, Bz, Cz), 128 L + 32 V per witness lacking rows (its row sums and its variables' place in the
//              joint job's block), and ONE interleaved tile of 4 * 2V * 32 bytes where a product pass runs.
//   tiles      per chunk, the witnesses lacking products, at most kProveManyTile to a walk over the matrices.
//   row jobs   per chunk, the witnesses lacking rows: one job per MSM variant (`sparse`, as the single proof decides it), each one launch of
//              n * L <= kProveManyJobRows rows; more witnesses than that split the job.
// A chunk in which fewer than two witnesses lack a thing gets no pass for that thing: nothing is shared, and the proof forms it itself, as a single
// proof does.  A witness that is in no tile (no job) forms its products (rows) itself.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace otti {

constexpr size_t kProveManyChunk = 16, kProveManyTile = 4, kProveManyJobRows = 65535;   // the tile is k_sparse.hip's kEvalTile; a launch's rows are a grid's y

struct PmWitness { bool has_rows = false, has_products = false, sparse = false; };
struct PmTile { std::vector<uint32_t> wit; };                          // indices into the batch, ascending
struct PmRowJob { bool sparse = false; std::vector<uint32_t> wit; size_t rows = 0; };   // rows = wit.size() * L
struct PmChunk { size_t first = 0, count = 0; std::vector<PmTile> tiles; std::vector<PmRowJob> jobs; uint64_t bytes = 0; };
struct PmPlan { std::vector<PmChunk> chunks; };                        // the chunks cover [0, K) in order

// what witnesses [first, first + count) cost as one chunk, the fewer-than-two rule applied
inline uint64_t prove_many_chunk_bytes(size_t N, size_t V, size_t L, const PmWitness *w, size_t first, size_t count) {
    uint64_t np = 0, nr = 0;
    for (size_t i = first; i < first + count; i++) { np += !w[i].has_products; nr += !w[i].has_rows; }
    if (np < 2) np = 0;
    if (nr < 2 || L > kProveManyJobRows) nr = 0;                        // (a single witness's rows beyond one launch: no job can hold it)
    return np * 96 * (uint64_t)N + (np ? (uint64_t)kProveManyTile * 2 * V * 32 : 0) + nr * (128 * (uint64_t)L + 32 * (uint64_t)V);
}

inline PmPlan prove_many_plan(size_t K, size_t N, size_t V, size_t L, size_t R, const PmWitness *w, uint64_t budget) {
    (void)R;                                                           // V = L * R: the row length changes no byte count
    PmPlan plan;
    for (size_t first = 0; first < K;) {
        // the longest run from `first` that fits: a chunk always takes one witness (alone it costs nothing: nothing to share)
        size_t count = 1;
        while (first + count < K && count < kProveManyChunk && prove_many_chunk_bytes(N, V, L, w, first, count + 1) <= budget) count++;
        PmChunk c; c.first = first; c.count = count; c.bytes = prove_many_chunk_bytes(N, V, L, w, first, count);
        std::vector<uint32_t> lack_p, lack_r[2];
        for (size_t i = first; i < first + count; i++) {
            if (!w[i].has_products) lack_p.push_back((uint32_t)i);
            if (!w[i].has_rows) lack_r[w[i].sparse ? 1 : 0].push_back((uint32_t)i);
        }
        if (lack_p.size() >= 2)
            for (size_t t0 = 0; t0 < lack_p.size(); t0 += kProveManyTile) {
                PmTile t; t.wit.assign(lack_p.begin() + (long)t0, lack_p.begin() + (long)std::min(lack_p.size(), t0 + kProveManyTile));
                c.tiles.push_back(t);
            }
        const size_t per_job = L ? kProveManyJobRows / L : 0;          // witnesses one launch holds
        if (lack_r[0].size() + lack_r[1].size() >= 2 && per_job)
            for (int s = 0; s < 2; s++)
                for (size_t j0 = 0; j0 < lack_r[s].size(); j0 += per_job) {
                    PmRowJob j; j.sparse = s != 0;
                    j.wit.assign(lack_r[s].begin() + (long)j0, lack_r[s].begin() + (long)std::min(lack_r[s].size(), j0 + per_job));
                    j.rows = j.wit.size() * L;
                    c.jobs.push_back(j);
                }
        plan.chunks.push_back(c);
        first += count;
    }
    return plan;
}

}  // namespace otti
