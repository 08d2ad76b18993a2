// K25 / K26: the counting halves of the structural LSB-replacement payload estimators (ws_unet_amd/ws/structural.py): the trace-set table
// of Sample Pairs Analysis (Dumitrescu, Wu, Wang 2003) and the regular / singular group counts of RS analysis (Fridrich, Goljan, Du 2001).
//
//   K25  pairs (u, v) of an image: every horizontally adjacent (x[r][c], x[r][c+1]) and every vertically adjacent (x[r][c], x[r+1][c]).
//        d = |u - v|, m = d >> 1, hi = max(u, v):
//          tables[n][0][m] (E) += 1   d even
//          tables[n][1][m] (X) += 1   d odd, hi even    (the halves u >> 1, v >> 1 differ by m + 1)
//          tables[n][2][m] (Y) += 1   d odd, hi odd     (the halves differ by m)
//   K26  groups G = x[r][4g .. 4g+3], g < w / 4;  f(G) = |g1-g0| + |g2-g1| + |g3-g2|;  F1(v) = v ^ 1,  F-1(v) = ((v + 1) ^ 1) - 1
//        (0 -> -1, 255 -> 256, not clamped);  G_M = F1 on g1, g2;  G_-M = F-1 on g1, g2:
//          counts[n][0..3] = #{f(G_M) > f(G)}, #{f(G_M) < f(G)}, #{f(G_-M) > f(G)}, #{f(G_-M) < f(G)}
//          counts[n][4..7] = the same four with G ^ 1 (every LSB flipped) in the place of G.
//
// Both are count kernels on the strip tile of wsu_count.h, which has the tile, the loads, the register counters and the flush.  K25 counts
// into one private LDS histogram of 384 uint32 bins per wave with LDS atomics (a tile has 2 * CT_ROWS * CT_COLS = 32 768 pairs at the most,
// far below 2^32) -- except the three m = 0 bins (d = 0 and the two kinds of d = 1), which take 29-45 % of a fixture cover's pairs and ALL of
// a constant plane's: those are HotBins fields.  As per-wave `__ballot` + popcount sums they cost 116 scalar spills (680 with the row loop
// unrolled) with 32 pairs per row in flight, and measured 1.3-1.5 x slower.  K26 has no histogram: its eight counters ARE ballots and
// popcounts, wave-uniform sums in scalar registers (no spill there, and measured 4 % faster than per-lane counters).  All loop bounds are
// uniform and a missing pixel only clears a predicate, so whole waves execute every ballot.  profiles/r22/README.md has the A/Bs (register
// path against all-atomics, per-lane against ballot counters) on the fixture covers and on a constant plane.
#include "wsu_count.h"

namespace {

constexpr int SPA_BINS = 3 * 128, RS_COUNTS = 8;
static_assert(2ll * CT_ROWS * CT_COLS < (1ll << 32), "a tile's 32-bit bins must hold every pair of the tile");
using SpaHot = HotBins<3, 10, 2 * 16 * CT_TRT>;         // one field per class; a thread sees 32 * CT_TRT pairs

// one pair: an m = 0 pair goes to the thread's register counters, every other pair to the wave's LDS histogram
__device__ __forceinline__ void spa_count(int u, int v, bool valid, uint32_t* __restrict__ hist, SpaHot& hot) {
    const int d = abs(u - v), m = d >> 1, hi = max(u, v);
    const int cls = (d & 1) ? 1 + (hi & 1) : 0;
    hot.add(cls, valid && m == 0);
    if (valid && m != 0) atomicAdd(&hist[cls * 128 + m], 1u);
}

__global__ __launch_bounds__(CT_THREADS) void spa_tables_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ tables,
                                                                int h, int w, int tiles_c) {
    __shared__ uint32_t hist[CT_WAVES][SPA_BINS];
    const int nn = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < CT_WAVES * SPA_BINS; i += CT_THREADS) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const CtStrip st = ct_strip(tiles_c, w, 1);
    const int rem = st.rem;
    const long long r0 = st.r0;
    const uint8_t* img = xu8 + (size_t)nn * h * w + st.c;
    const bool col_in = rem > 0;
    const uint32_t pix = (1u << min(rem, 16)) - 1u, pairs_h = (1u << max(rem - 1, 0)) - 1u;      // bit i: pixel i / its right neighbour is in the row
    SpaHot hot;
    u32x4 cur = mk_u4(0u, 0u, 0u, 0u);
    if (col_in && r0 < h) cur = ct_load_strip(img + (size_t)r0 * w, rem);
#pragma unroll 1
    for (int k = 0; k < CT_TRT; ++k) {
        const long long r = r0 + k;
        const bool row_in = col_in && r < h, below = col_in && r + 1 < h;
        const uint32_t mh = row_in ? pairs_h : 0u, mv = below ? pix : 0u;
        const int right = row_in && rem > 16 ? (int)img[(size_t)r * w + 16] : 0;
        u32x4 next = mk_u4(0u, 0u, 0u, 0u);
        if (below) next = ct_load_strip(img + (size_t)(r + 1) * w, rem);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int u = ct_px(cur, i);
            spa_count(u, i < 15 ? ct_px(cur, i + 1) : right, (mh >> i) & 1u, hist[wave], hot);
            spa_count(u, ct_px(next, i), (mv >> i) & 1u, hist[wave], hot);
        }
        cur = next;
    }
    hot.fold(hist[wave], 128);
    count_flush<CT_WAVES>(&hist[0][0], SPA_BINS, tables, (size_t)nn * SPA_BINS);
}

__device__ __forceinline__ int rs_f(int g0, int g1, int g2, int g3) { return abs(g1 - g0) + abs(g2 - g1) + abs(g3 - g2); }
__device__ __forceinline__ int rs_fneg(int v) { return ((v + 1) ^ 1) - 1; }

// lanes of the wave for which p holds; every lane of the wave must get here
__device__ __forceinline__ uint32_t rs_popc(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// one group per lane, of the plane (flip = 0) or of the plane with every LSB flipped (flip = 1): the wave's cnt[0..3] += R_M, S_M, R_-M, S_-M
__device__ __forceinline__ void rs_count(int g0, int g1, int g2, int g3, int flip, bool valid, uint32_t* cnt) {
    g0 ^= flip; g1 ^= flip; g2 ^= flip; g3 ^= flip;
    const int f = rs_f(g0, g1, g2, g3), fp = rs_f(g0, g1 ^ 1, g2 ^ 1, g3), fn = rs_f(g0, rs_fneg(g1), rs_fneg(g2), g3);
    cnt[0] += rs_popc(valid && fp > f);
    cnt[1] += rs_popc(valid && fp < f);
    cnt[2] += rs_popc(valid && fn > f);
    cnt[3] += rs_popc(valid && fn < f);
}

__global__ __launch_bounds__(CT_THREADS) void rs_counts_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ counts,
                                                               int h, int w, int tiles_c) {
    __shared__ uint32_t part[CT_WAVES][RS_COUNTS];
    const int nn = blockIdx.y, tid = threadIdx.x;
    const CtStrip st = ct_strip(tiles_c, w, 1);
    const int rem = st.rem;
    const uint8_t* img = xu8 + (size_t)nn * h * w + st.c;
    uint32_t cnt[RS_COUNTS];
#pragma unroll
    for (int q = 0; q < RS_COUNTS; ++q) cnt[q] = 0u;
#pragma unroll 1
    for (int k = 0; k < CT_TRT; ++k) {
        const long long r = st.r0 + k;
        const bool row_in = rem > 0 && r < h;
        u32x4 cur = mk_u4(0u, 0u, 0u, 0u);
        if (row_in) cur = ct_load_strip(img + (size_t)r * w, rem);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bool valid = row_in && 4 * g + 4 <= rem;                  // the trailing w % 4 columns belong to no group
            const int g0 = ct_px(cur, 4 * g), g1 = ct_px(cur, 4 * g + 1), g2 = ct_px(cur, 4 * g + 2), g3 = ct_px(cur, 4 * g + 3);
            rs_count(g0, g1, g2, g3, 0, valid, cnt);
            rs_count(g0, g1, g2, g3, 1, valid, cnt + 4);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < RS_COUNTS; ++q) part[tid >> 6][q] = cnt[q];
    }
    count_flush<CT_WAVES>(&part[0][0], RS_COUNTS, counts, (size_t)nn * RS_COUNTS);
}

}  // namespace

extern "C" {

int wsu_spa_tables(const uint8_t* x_u8, unsigned long long* tables, int n, int h, int w, void* stream) {
    return count_launch("spa_tables", "spa_tables memset", "spa_tables_kernel", spa_tables_kernel, CT_THREADS, 0, x_u8, tables, SPA_BINS, n, h, w, 0, CT_ROWS, CT_COLS, stream);
}

int wsu_rs_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream) {
    return count_launch("rs_counts", "rs_counts memset", "rs_counts_kernel", rs_counts_kernel, CT_THREADS, 0, x_u8, counts, RS_COUNTS, n, h, w, 0, CT_ROWS, CT_COLS, stream);
}

}  // extern "C"
