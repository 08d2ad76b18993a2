// K54: the co-occurrence counts of the fan submodels of the spatial rich model (SRM; Fridrich, Kodovsky, IEEE TIFS 7(3), 2012): the first-
// and third-order min/max submodels over perpendicular pairs and over three, four and five adjacent ones of the eight directional
// residuals, the integer part of ws_unet_amd/srm.py's `features_fans`.  Not part of the reference.  include/wsu.h has the definition:
// 20 sets per (class, q2), 200 tables of 625 bins, 400 updates per pixel.
//
// A (class, q2) is 40 tables = 100 000 bytes, so it is cut into FAN_GROUPS = 4 slices of five sets = 10 tables = 25 000 bytes: blockIdx.z
// is the slice, 20 of them, and a workgroup is srm_sets.h's (K50's organisation).  Every slice computes the eight members' digits at the
// 19 centres of its row again, a byte each in two words per centre.  Registers, what was compiled and dropped, and the measurements:
// DESIGN.md 4-srmfull, profiles/r41/.
#include "srm_sets.h"

namespace {

constexpr int FAN_SETS = 20, FAN_GROUPS = 4, FAN_GROUP_SETS = FAN_SETS / FAN_GROUPS, FAN_TABLES = 5 * 2 * FAN_SETS, FAN_SLICES = 5 * FAN_GROUPS;
// the members as bits, counter-clockwise
constexpr int E = 1, NE = 2, N = 4, NW = 8, W = 16, SW = 32, S_ = 64, SE = 128;
// the sets in order: the perpendicular pairs; the 3-fans centred on a diagonal; the 4-fans that hold N or S with both neighbours, then
// those that hold E or W with both; the 5-fans centred on a diagonal
constexpr int FAN_MEMBERS[FAN_SETS] = {
    E | N, N | W, W | S_, S_ | E,
    E | NE | N, N | NW | W, W | SW | S_, S_ | SE | E,
    E | NE | N | NW, NE | N | NW | W, W | SW | S_ | SE, SW | S_ | SE | E,
    N | NW | W | SW, NW | W | SW | S_, S_ | SE | E | NE, SE | E | NE | N,
    SE | E | NE | N | NW, NE | N | NW | W | SW, NW | W | SW | S_ | SE, SW | S_ | SE | E | NE};

template <int CLS> struct FanSpec {                     // CLS 1: X[p+d] - X[p]; CLS 3: X[p-d] - 3 X[p] + 3 X[p+d] - X[p+2d]
    static constexpr int UP = CLS == 3 ? 2 : 1, S = CLS == 3 ? 1 : 0, WORDS = 2;
    static constexpr int members(int set) { return FAN_MEMBERS[set]; }
    // the step (dr, dc) of direction k = E, NE, N, NW, W, SW, S, SE
    static constexpr int dr(int k) { return k == 0 || k == 4 ? 0 : k < 4 ? -1 : 1; }
    static constexpr int dc(int k) { return k == 2 || k == 6 ? 0 : k < 2 || k == 7 ? 1 : -1; }
    // a first-order residual reaches 1 along its direction, a third-order one 2 along it and 1 against it
    static constexpr int reach(int k, int side) {
        const int along = side == 0 ? -dr(k) : side == 1 ? dr(k) : side == 2 ? -dc(k) : dc(k);
        return along > 0 ? (CLS == 3 ? 2 : 1) : along < 0 && CLS == 3 ? 1 : 0;
    }
    template <class PX> static __device__ __forceinline__ void digits(PX px, int q2, uint32_t (&P)[WORDS][SS_DIGITS]) {
#pragma unroll
        for (int t = 0; t < SS_DIGITS; ++t) {
            const int x = px(0, t);
            P[0][t] = P[1][t] = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int R = CLS == 1 ? px(dr(k), t + dc(k)) - x
                                       : px(-dr(k), t - dc(k)) - 3 * x + 3 * px(dr(k), t + dc(k)) - px(2 * dr(k), t + 2 * dc(k));
                P[k >> 2][t] |= (uint32_t)run_digit(R, q2) << (8 * (k & 3));
            }
        }
    }
};

template <int CLS, int GROUP>
__device__ __forceinline__ void fan_group(uint32_t* hist, const uint8_t* img, unsigned long long* counts, size_t row, int q2, int h, int w, int tiles_c) {
    ss_slice<FanSpec<CLS>, GROUP * FAN_GROUP_SETS, FAN_GROUP_SETS>(hist, img, counts, row + (size_t)(2 * GROUP * FAN_GROUP_SETS) * SS_BINS, q2, h, w,
                                                                   tiles_c);
}
template <int CLS>
__device__ __forceinline__ void fan_class(uint32_t* hist, const uint8_t* img, unsigned long long* counts, size_t row, int q2, int group, int h, int w,
                                          int tiles_c) {
    if (group == 0) fan_group<CLS, 0>(hist, img, counts, row, q2, h, w, tiles_c);
    else if (group == 1) fan_group<CLS, 1>(hist, img, counts, row, q2, h, w, tiles_c);
    else if (group == 2) fan_group<CLS, 2>(hist, img, counts, row, q2, h, w, tiles_c);
    else fan_group<CLS, 3>(hist, img, counts, row, q2, h, w, tiles_c);
}

__global__ __launch_bounds__(CT_THREADS) void srm_fan_counts_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ counts,
                                                                    int h, int w, int tiles_c) {
    __shared__ uint32_t hist[2 * FAN_GROUP_SETS * SS_BINS];
    const int nn = blockIdx.y, cq = blockIdx.z / FAN_GROUPS, group = blockIdx.z % FAN_GROUPS;   // cq 0, 1: S1 at q2 = 2, 4; 2 .. 4: S3 at 6, 9, 12
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const size_t row = ((size_t)nn * FAN_TABLES + (size_t)cq * 2 * FAN_SETS) * SS_BINS;
    if (cq < 2) fan_class<1>(hist, img, counts, row, 2 + 2 * cq, group, h, w, tiles_c);
    else fan_class<3>(hist, img, counts, row, 3 * cq, group, h, w, tiles_c);
}

}  // namespace

extern "C" {

int wsu_srm_fan_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream) {
    return count_launch_slices("srm_fan_counts", "srm_fan_counts memset", "srm_fan_counts_kernel", srm_fan_counts_kernel, CT_THREADS, 0, x_u8,
                               counts, (size_t)FAN_TABLES * SS_BINS, n, h, w, 0, SS_ROWS, CT_COLS, FAN_SLICES, stream);
}

}  // extern "C"
