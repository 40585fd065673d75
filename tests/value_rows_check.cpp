// comm_value_rows (otti_amd/csrc/value_rows.h) on the host against a brute-force marking: every element of [12 N, 15 N) marks the row of the
// L x R layout it lies in, and the marked rows have to be exactly [r0, r1) — for every power-of-two N up to 2^12 with every split L R = 16 N,
// which includes the splits the generators use (R = 2^(m - m / 2), m = log2 16 N) and the R > N ones of N <= 8.  Nothing here needs a GPU.
// Built and run by tests/test_values_host.py (plain g++, standard library only, address and undefined-behaviour sanitizers).
#include "../otti_amd/csrc/value_rows.h"
#include <stdio.h>
#include <vector>

using namespace otti;

int main() {
    size_t layouts = 0, mismatches = 0, r_above_n = 0, gens_splits = 0;
    for (size_t lgN = 1; lgN <= 12; lgN++) {
        const size_t N = (size_t)1 << lgN, m = lgN + 4;
        for (size_t lgR = 0; lgR <= m; lgR++) {
            const size_t R = (size_t)1 << lgR, L = (16 * N) / R;
            std::vector<char> mark(L, 0);
            for (size_t e = 12 * N; e < 15 * N; e++) mark[e / R] = 1;
            const ValueRows v = comm_value_rows(N, L, R);
            bool ok = v.r0 <= v.r1 && v.r1 <= L;
            for (size_t r = 0; r < L && ok; r++) ok = (mark[r] != 0) == (r >= v.r0 && r < v.r1);
            if (R <= N) ok = ok && v.r1 - v.r0 == 3 * N / R;       // whole parts: nothing but values is summed again
            if (!ok) { mismatches++; fprintf(stderr, "N = %zu, L = %zu, R = %zu: rows [%zu, %zu) differ from the marking\n", N, L, R, v.r0, v.r1); }
            layouts++; r_above_n += R > N; gens_splits += lgR == m - m / 2;
        }
    }
    // the three small sizes by hand (R = 2^(m - m / 2)): N = 2: 4 x 8, values in elements 24 .. 29: row 3; N = 4: 8 x 8, 48 .. 59: rows 6, 7;
    // N = 8: 8 x 16, 96 .. 119: rows 6, 7
    const struct { size_t N, L, R, r0, r1; } byhand[] = {{2, 4, 8, 3, 4}, {4, 8, 8, 6, 8}, {8, 8, 16, 6, 8}, {1024, 128, 128, 96, 120}};
    for (const auto &h : byhand) {
        const ValueRows v = comm_value_rows(h.N, h.L, h.R);
        if (v.r0 != h.r0 || v.r1 != h.r1) { mismatches++; fprintf(stderr, "N = %zu by hand: [%zu, %zu), expected [%zu, %zu)\n", h.N, v.r0, v.r1, h.r0, h.r1); }
    }
    const ValueRows none = comm_value_rows(0, 0, 0);
    if (none.r0 != 0 || none.r1 != 0) mismatches++;
    printf("%zu layouts, %zu with R > N, %zu generator splits, %zu mismatches\n", layouts, r_above_n, gens_splits, mismatches);
    return mismatches ? 1 : 0;
}
