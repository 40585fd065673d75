// Which rows of a computation commitment's comm_ops depend on the coefficients of A, B, C (otti_comp_comm_revalue): pure, standard headers only,
// checked on the host against a brute-force marking (tests/value_rows_check.cpp) under the address and undefined-behaviour sanitizers.
//
// comb_ops is 16 N field elements (snark_prover.h DeviceDecomm): fifteen parts of N — addresses and timestamps first — and N zeros; the values
// of A, B, C are parts 12, 13, 14, the elements [12 N, 15 N).  The commitment lays them out as L rows of R elements (L R = 16 N, all powers of
// two) and sums every row by itself, so only the rows whose span [r R, (r + 1) R) meets [12 N, 15 N) move with the coefficients:
//     r0 = floor(12 N / R),  r1 = ceil(15 N / R)           rows [r0, r1)
// R <= N: rows never straddle a part and these are exactly 3 N / R rows.  R > N (N <= 8: one row spans several parts): a row that holds values
// holds addresses or timestamps too and is summed again as a whole.
#pragma once
#include <stddef.h>

namespace otti {

struct ValueRows { size_t r0, r1; };                          // [r0, r1); r1 <= L
inline ValueRows comm_value_rows(size_t N, size_t L, size_t R) {
    ValueRows v{0, 0};
    if (!N || !L || !R) return v;
    v.r0 = 12 * N / R;
    v.r1 = (15 * N + R - 1) / R;
    if (v.r1 > L) v.r1 = L;
    if (v.r0 > v.r1) v.r0 = v.r1;
    return v;
}

}  // namespace otti
