// K55: the co-occurrence counts of the EDGE3x3 and EDGE5x5 classes of the spatial rich model (SRM; Fridrich, Kodovsky, IEEE TIFS 7(3),
// 2012): the half of the 3x3 (KB) or 5x5 (KV) kernel on one side of its centre row or column as four residuals U, D, L, R, and the min/max
// tables over eleven sets of them, the integer part of ws_unet_amd/srm.py's `features_edge`.  Not part of the reference.  include/wsu.h
// has the definition: 132 tables of 625 bins, 264 updates per pixel.
//
// A (class, q2) is 22 tables = 55 000 bytes, cut into two slices of six and five sets (12 and 10 tables, 30 000 bytes at the most):
// blockIdx.z is the slice, 12 of them, and a workgroup is srm_sets.h's (K50's organisation).  A singleton set goes through the same
// two updates with lo = hi.  Registers, what was compiled and dropped, and the measurements: DESIGN.md 4-srmfull, profiles/r41/.
#include "srm_sets.h"

namespace {

constexpr int EDGE_SETS = 11, EDGE_FIRST = 6, EDGE_TABLES = 6 * 2 * EDGE_SETS, EDGE_SLICES = 6 * 2;
constexpr int U = 1, D = 2, L = 4, R = 8;               // the members as bits
constexpr int EDGE_MEMBERS[EDGE_SETS] = {U, D, L, R, U | L, U | R, D | L, D | R, U | D, L | R, U | D | L | R};
constexpr int EDGE_KB[3][3] = {{-1, 2, -1}, {2, -4, 2}, {-1, 2, -1}};
constexpr int EDGE_KV[5][5] = {{-1, 2, -2, 2, -1}, {2, -6, 8, -6, 2}, {-2, 8, -12, 8, -2}, {2, -6, 8, -6, 2}, {-1, 2, -2, 2, -1}};

template <int K> struct EdgeSpec {                      // K = 1: EDGE3x3, 2: EDGE5x5
    static constexpr int UP = K, S = K - 1, WORDS = 1;
    static constexpr int members(int set) { return EDGE_MEMBERS[set]; }
    static constexpr int weight(int i, int j) { return K == 1 ? EDGE_KB[K + i][K + j] : EDGE_KV[K + i][K + j]; }   // of the kernel's tap (i, j) around its centre
    // U reaches K up, left and right and nothing down; D, L and R are U turned
    static constexpr int reach(int k, int side) { return (k == 0 && side == 1) || (k == 1 && side == 0) || (k == 2 && side == 3) || (k == 3 && side == 2) ? 0 : K; }
    template <class PX> static __device__ __forceinline__ void digits(PX px, int q2, uint32_t (&P)[WORDS][SS_DIGITS]) {
#pragma unroll
        for (int t = 0; t < SS_DIGITS; ++t) {
            int u = 0, d = 0, l = 0, r = 0;             // U: rows -K .. 0 of the kernel; D: U flipped; L: U transposed; R: L mirrored
#pragma unroll
            for (int i = -K; i <= 0; ++i)
#pragma unroll
                for (int j = -K; j <= K; ++j) {
                    u += weight(i, j) * px(i, t + j);
                    d += weight(i, j) * px(-i, t + j);
                    l += weight(i, j) * px(j, t + i);
                    r += weight(i, j) * px(j, t - i);
                }
            P[0][t] = (uint32_t)run_digit(u, q2) | (uint32_t)run_digit(d, q2) << 8 | (uint32_t)run_digit(l, q2) << 16 | (uint32_t)run_digit(r, q2) << 24;
        }
    }
};

template <int K>
__device__ __forceinline__ void edge_class(uint32_t* hist, const uint8_t* img, unsigned long long* counts, size_t row, int q2, int second, int h, int w,
                                           int tiles_c) {
    if (!second) ss_slice<EdgeSpec<K>, 0, EDGE_FIRST>(hist, img, counts, row, q2, h, w, tiles_c);
    else ss_slice<EdgeSpec<K>, EDGE_FIRST, EDGE_SETS - EDGE_FIRST>(hist, img, counts, row + (size_t)(2 * EDGE_FIRST) * SS_BINS, q2, h, w, tiles_c);
}

__global__ __launch_bounds__(CT_THREADS) void srm_edge_counts_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ counts,
                                                                     int h, int w, int tiles_c) {
    __shared__ uint32_t hist[2 * EDGE_FIRST * SS_BINS];
    const int nn = blockIdx.y, cq = blockIdx.z >> 1, second = blockIdx.z & 1;   // cq 0 .. 2: EDGE3x3 at q2 = 8, 12, 16; 3 .. 5: EDGE5x5 at 24, 36, 48
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const size_t row = ((size_t)nn * EDGE_TABLES + (size_t)cq * 2 * EDGE_SETS) * SS_BINS;
    if (cq < 3) edge_class<1>(hist, img, counts, row, 8 + 4 * cq, second, h, w, tiles_c);
    else edge_class<2>(hist, img, counts, row, 12 * (cq - 1), second, h, w, tiles_c);
}

}  // namespace

extern "C" {

int wsu_srm_edge_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream) {
    return count_launch_slices("srm_edge_counts", "srm_edge_counts memset", "srm_edge_counts_kernel", srm_edge_counts_kernel, CT_THREADS, 0, x_u8,
                               counts, (size_t)EDGE_TABLES * SS_BINS, n, h, w, 0, SS_ROWS, CT_COLS, EDGE_SLICES, stream);
}

}  // extern "C"
