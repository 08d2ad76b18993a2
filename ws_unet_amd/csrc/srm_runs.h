// What the min/max count kernels of the spatial rich model share through srm_sets.h (K50, K54, K55), and what K49 (srm.hip) and K52
// (srm_weighted.hip) still say themselves: the digit of a residual and the binning of a row of 19 digits into the 16
// runs of scan h and the 16 runs of scan v that end in the row.  What a run adds, and whether it counts, is the caller's.
#pragma once
#include "wsu_count.h"

constexpr int RUN_DIGITS = 19, RUN_BINS = 625, RUN_CENTRE = 312;       // a row of a thread's strip; 5^4 bins, four digits 0 at the centre

// bit i of a mask as 0 or -1
__device__ __forceinline__ uint32_t run_bit(uint32_t mask, int i) { return (uint32_t)((int)(mask << (31 - i)) >> 31); }
__device__ __forceinline__ uint32_t run_low_bits(int n) { return (1u << min(max(n, 0), 16)) - 1u; }

// the digit + 2 of a residual R at the step q2 / 2: sign(R) min((4|R| + q2) / (2 q2), 2) is (4|R| >= q2) + (4|R| >= 3 q2) with the sign
__device__ __forceinline__ int run_digit(int R, int q2) {
    const int mag = 4 * abs(R), sgn = R >> 31;
    const int m = (mag >= q2 ? 1 : 0) + (mag >= 3 * q2 ? 1 : 0);
    return (m ^ sgn) - sgn + 2;
}

// One kind of digit at one step: dg, the digits + 2 at the 19 centres of the row.  Scan h (SCAN 0): run i of digits i .. i+3; scan v
// (SCAN 1): digit i + S under the three above it in its column, which `above` holds and takes this row into: byte i of its four words =
// the digits (+2) of the three rows above as a base-5 number.  Each of the 32 bins goes to counter.count<TABLE, SCAN>(bin, i), which
// decides whether run i counts and what it adds.
template <int TABLE, int S, class COUNTER>
__device__ __forceinline__ void run_bins(COUNTER& counter, const int (&dg)[RUN_DIGITS], uint32_t (&above)[4]) {
    int pair[RUN_DIGITS - 1];
#pragma unroll
    for (int t = 0; t < RUN_DIGITS - 1; ++t) pair[t] = dg[t] * 5 + dg[t + 1];
#pragma unroll
    for (int i = 0; i < 16; ++i) counter.template count<TABLE, 0>((uint32_t)(pair[i] * 25 + pair[i + 2]), i);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        uint32_t now = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * g + j;
            const uint32_t bin = ((above[g] >> (8 * j)) & 255u) * 5u + (uint32_t)dg[i + S];
            counter.template count<TABLE, 1>(bin, i);
            now |= (bin % 125u) << (8 * j);
        }
        above[g] = now;
    }
}
