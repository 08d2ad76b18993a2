// K50: the co-occurrence counts of the min/max submodels of the spatial rich model (SRM; Fridrich, Kodovsky, IEEE TIFS 7(3), 2012) on the
// directional first-, second- and third-order residuals, the integer part of ws_unet_amd/srm.py's `features_minmax`.  Not part of the
// reference.  include/wsu.h has the definition: four directional residuals per class and pixel, K49's digit -2 .. 2 of each at one step
// q2; a set of residuals has the digits lo = min and hi = max over its members; a table counts per run of four positions along a row
// (scan h) or down a column (scan v) the four lo digits at their bin and the four hi digits at the bin of their negation: 118 tables of
// 625 bins, 236 updates per pixel.
//
// 118 tables are 295 000 bytes, more than a CU's LDS, so the work is cut by (class, q2) into MM_SLICES = 8 slices of 14 (S1, S3: seven
// sets) or 16 (S2: eight) tables, 35 000 or 40 000 bytes: blockIdx.z is the slice, and a workgroup is K49's otherwise -- the strip tile of
// wsu_count.h, a thread walking SS_TRT rows of its strip (srm_sets.h has the code, which K54 and K55 share):
//   * a step has the rows rho-UP .. rho+UP in registers (CtRow each; UP = 2 for S3, else 1) and computes the four members' digits at
//     the 19 centres of row rho, columns c - S + t (S = 1 for S3, whose E reads two columns to the right; else 0), ONCE, a byte each in
//     19 words; a set's lo and hi are v_min3 / v_max3 over the bytes it takes, and hi is negated (4 - hi in digits + 2), so both
//     halves count through the same code;
//   * scan h: the 16 runs of that row, run i from digits i .. i+3; scan v: the run that ENDS in this row at column c + i, from a byte
//     per set, half and column that holds the three digits above as a base-5 number.  The run's top row is rho - 3, so a thread takes
//     SS_TRT + 3 steps: steps 0 .. SS_TRT-1 count scan h, steps 3 .. SS_TRT+2 scan v, and every run belongs to exactly one thread;
//   * one set of tables per workgroup that its four waves add to with LDS atomics, except the centre bins, where a smooth or saturated
//     plane sends every update (lo = hi = 0): a thread notes in HotBins fields the updates that went to ANOTHER bin, and the centre
//     bin gets what is left of the thread's counted updates, which are a closed form of its rows and column masks.
// Registers, what was compiled and dropped, and the measurements: DESIGN.md 4-srmmm, profiles/r38/.
#include "srm_sets.h"

namespace {

constexpr int MM_TABLES = 118, MM_SLICES = 8, MM_SLICE_TABLES = 16;

// the members of a set as bits: S1 / S3 W, E, N, S; S2 h, v, d, m
constexpr int MA = 1, MB = 2, MC = 4, MD = 8;
// the sets' members in order: S1 / S3 WE, NS, WENS, WNE, ESW, SWN, NES; S2 hv, hvdm, hvd, hvm, hd, hm, vd, vm
constexpr int MM_SETS_13[7] = {MA | MB, MC | MD, MA | MB | MC | MD, MA | MC | MB, MB | MD | MA, MD | MA | MC, MC | MB | MD};
constexpr int MM_SETS_2[8] = {MA | MB, MA | MB | MC | MD, MA | MB | MC, MA | MB | MD, MA | MC, MA | MD, MB | MC, MB | MD};

template <int CLS> struct MmSpec {                      // CLS 1, 2, 3: the directional residuals of that order
    static constexpr int UP = CLS == 3 ? 2 : 1, S = CLS == 3 ? 1 : 0, WORDS = 1, SETS = CLS == 2 ? 8 : 7;
    static constexpr int members(int set) { return CLS == 2 ? MM_SETS_2[set] : MM_SETS_13[set]; }
    // S2: h reaches 1 left and right, v 1 up and down, d and m 1 to every side.  S1 / S3: W, E, N, S point to the sides 2, 3, 0, 1; a
    // first-order residual reaches 1 to its side, a third-order one 2 to its side and 1 to the opposite one
    static constexpr int reach(int k, int side) {
        if (CLS == 2) return k >= 2 || (k == 0) == (side >= 2) ? 1 : 0;
        return side == (k ^ 2) ? (CLS == 3 ? 2 : 1) : side == (k ^ 3) && CLS == 3 ? 1 : 0;
    }
    template <class PX> static __device__ __forceinline__ void digits(PX px, int q2, uint32_t (&P)[WORDS][SS_DIGITS]) {
        auto pack = [](int a, int b, int cc, int d) { return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)cc << 16 | (uint32_t)d << 24; };
        if constexpr (CLS == 1) {
            // W(t) = -g(t), E(t) = g(t + 1) with g(t) = X[t] - X[t-1]: the digit is odd, 4 - d in digits + 2
            int g[SS_DIGITS + 1];
#pragma unroll
            for (int t = 0; t < SS_DIGITS + 1; ++t) g[t] = run_digit(px(0, t) - px(0, t - 1), q2);
#pragma unroll
            for (int t = 0; t < SS_DIGITS; ++t)
                P[0][t] = pack(4 - g[t], g[t + 1], run_digit(px(-1, t) - px(0, t), q2), run_digit(px(1, t) - px(0, t), q2));
        } else if constexpr (CLS == 2) {
#pragma unroll
            for (int t = 0; t < SS_DIGITS; ++t) {
                const int x2 = 2 * px(0, t);
                P[0][t] = pack(run_digit(px(0, t - 1) - x2 + px(0, t + 1), q2), run_digit(px(-1, t) - x2 + px(1, t), q2),
                               run_digit(px(-1, t - 1) - x2 + px(1, t + 1), q2), run_digit(px(-1, t + 1) - x2 + px(1, t - 1), q2));
            }
        } else {
            // W(t) = -k(t), E(t) = k(t + 1) with k(t) = X[t-2] - 3 X[t-1] + 3 X[t] - X[t+1], which is E at the centre t - 1
            int k[SS_DIGITS + 1];
#pragma unroll
            for (int t = 0; t < SS_DIGITS + 1; ++t) k[t] = run_digit(px(0, t - 2) - 3 * px(0, t - 1) + 3 * px(0, t) - px(0, t + 1), q2);
#pragma unroll
            for (int t = 0; t < SS_DIGITS; ++t)
                P[0][t] = pack(4 - k[t], k[t + 1], run_digit(px(1, t) - 3 * px(0, t) + 3 * px(-1, t) - px(-2, t), q2),
                               run_digit(px(-1, t) - 3 * px(0, t) + 3 * px(1, t) - px(2, t), q2));
        }
    }
};

// one slice: class CLS at the step q2, its tables to counts[row ..]
template <int CLS>
__device__ __forceinline__ void mm_slice(uint32_t* __restrict__ hist, const uint8_t* __restrict__ img, unsigned long long* __restrict__ counts,
                                         size_t row, int q2, int h, int w, int tiles_c) {
    ss_slice<MmSpec<CLS>, 0, MmSpec<CLS>::SETS>(hist, img, counts, row, q2, h, w, tiles_c);
}

__global__ __launch_bounds__(CT_THREADS) void srm_minmax_counts_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ counts,
                                                                       int h, int w, int tiles_c) {
    __shared__ uint32_t hist[MM_SLICE_TABLES * SS_BINS];
    const int nn = blockIdx.y, slice = blockIdx.z;      // slices 0, 1: S1 at q2 = 2, 4; 2 .. 4: S2 at 4, 6, 8; 5 .. 7: S3 at 6, 9, 12
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const size_t row = (size_t)nn * MM_TABLES * SS_BINS;
    if (slice < 2) mm_slice<1>(hist, img, counts, row + (size_t)(14 * slice) * SS_BINS, 2 + 2 * slice, h, w, tiles_c);
    else if (slice < 5) mm_slice<2>(hist, img, counts, row + (size_t)(28 + 16 * (slice - 2)) * SS_BINS, 2 * slice, h, w, tiles_c);
    else mm_slice<3>(hist, img, counts, row + (size_t)(76 + 14 * (slice - 5)) * SS_BINS, 3 * slice - 9, h, w, tiles_c);
}

}  // namespace

extern "C" {

int wsu_srm_minmax_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream) {
    return count_launch_slices("srm_minmax_counts", "srm_minmax_counts memset", "srm_minmax_counts_kernel", srm_minmax_counts_kernel,
                               CT_THREADS, 0, x_u8, counts, (size_t)MM_TABLES * SS_BINS, n, h, w, 0, SS_ROWS, CT_COLS, MM_SLICES, stream);
}

}  // extern "C"
