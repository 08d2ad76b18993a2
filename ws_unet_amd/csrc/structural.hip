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
// Both count exact integers, so their bits depend on no order.  One workgroup owns a tile of ST_ROWS x ST_COLS pixels of one image:
// 32 strips of 16 columns by 8 row groups, a thread walking its strip down ST_TRT rows.  A strip of a row is ONE 16-byte load where the
// strip lies inside the row and its address is a multiple of 16; every other strip (the ragged last one of a row, and every strip of a row
// whose base an odd or `w % 4 != 0` width has shifted) is sixteen byte loads with the column clamped into the row.  A pixel or a
// neighbour outside the image only clears a predicate; every load is inside the image.
//
// K25 counts into one private LDS histogram of 384 uint32 bins per wave with LDS atomics (a tile has 2 * ST_ROWS * ST_COLS = 32 768 pairs
// at the most, far below 2^32) -- except the three m = 0 bins (d = 0 and the two kinds of d = 1), which take 29-45 % of a fixture cover's
// pairs and ALL of a constant plane's: same-address LDS atomics serialise, so those are counted in registers and reach the histogram as
// three adds per wave.  K25's register counters are per LANE (three fields of one VGPR, summed over the wave by shuffles at the end), not
// per-wave `__ballot` + popcount sums: the compiler keeps each ballot's 64-bit mask in a scalar register pair until its popcount is
// needed, and with 32 pairs per row in flight that cost 116 scalar spills (680 with the row loop unrolled) and measured 1.3-1.5 x slower.
// K26 has no histogram: its eight counters ARE ballots and popcounts, wave-uniform sums in scalar registers (no spill there, and
// measured 4 % faster than per-lane counters).  All loop bounds are uniform and a missing pixel only clears a predicate, so whole waves
// execute every ballot.  A workgroup flushes its non-zero sums with one 64-bit vector atomic each; the entry points zero the output on
// the stream first.  profiles/r22/README.md has the A/Bs (register path against all-atomics, per-lane against ballot counters) on the
// fixture covers and on a constant plane.
#include "wsu_device.h"

namespace {

constexpr int ST_TRT = 4, ST_STRIPS = 32, ST_GROUPS = 8, ST_THREADS = ST_STRIPS * ST_GROUPS, ST_WAVES = ST_THREADS / 64;
constexpr int ST_COLS = ST_STRIPS * 16, ST_ROWS = ST_GROUPS * ST_TRT;
constexpr int SPA_BINS = 3 * 128, RS_COUNTS = 8;
static_assert(2ll * ST_ROWS * ST_COLS < (1ll << 32), "a tile's 32-bit bins must hold every pair of the tile");

// sixteen pixels p[0 .. 15] of a row that has `rem` >= 1 pixels left from p on, as four little-endian words; a pixel past the row reads as
// the row's last one (the index is clamped, not branched on: sixteen independent loads) and is never counted by the callers.
__device__ __forceinline__ u32x4 st_load_strip(const uint8_t* __restrict__ p, int rem) {
    if (rem >= 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const u32x4*>(p);
    uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i)
        v[i >> 2] |= (uint32_t)p[min(i, rem - 1)] << (8 * (i & 3));
    return mk_u4(v[0], v[1], v[2], v[3]);
}

// a thread's strip: its first column and how many of the row's pixels lie at or after it (0: the strip is outside the image; capped at 17,
// one past the strip, which is all a caller asks)
__device__ __forceinline__ long long st_strip(int tiles_c, int w, int& rem) {
    const long long c = (long long)(blockIdx.x % tiles_c) * ST_COLS + (threadIdx.x & (ST_STRIPS - 1)) * 16;
    rem = (int)min(max((long long)w - c, 0ll), 17ll);
    return c;
}

__device__ __forceinline__ int st_px(const u32x4& s, int i) { return (int)((s[i >> 2] >> (8 * (i & 3))) & 255u); }

// sum over the wave, valid in its lane 0
__device__ __forceinline__ uint32_t st_wave_sum(uint32_t s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return s;
}

// one pair: an m = 0 pair goes to the thread's register counters (three 10-bit fields of `hot`, one per class: a thread sees
// 32 * ST_TRT pairs), every other pair to the wave's LDS histogram
constexpr int SPA_FIELD = 10;
static_assert(2 * 16 * ST_TRT < (1 << SPA_FIELD), "a thread's m = 0 counters must hold every pair of the thread");
__device__ __forceinline__ void spa_count(int u, int v, bool valid, uint32_t* __restrict__ hist, uint32_t& hot) {
    const int d = abs(u - v), m = d >> 1, hi = max(u, v);
    const int cls = (d & 1) ? 1 + (hi & 1) : 0;
    hot += valid && m == 0 ? 1u << (SPA_FIELD * cls) : 0u;
    if (valid && m != 0) atomicAdd(&hist[cls * 128 + m], 1u);
}

__global__ __launch_bounds__(ST_THREADS) void spa_tables_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ tables,
                                                                int h, int w, int tiles_c) {
    __shared__ uint32_t hist[ST_WAVES][SPA_BINS];
    const int nn = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < ST_WAVES * SPA_BINS; i += ST_THREADS) (&hist[0][0])[i] = 0u;
    __syncthreads();
    int rem;
    const long long c = st_strip(tiles_c, w, rem);
    const long long r0 = (long long)(blockIdx.x / tiles_c) * ST_ROWS + (tid / ST_STRIPS) * ST_TRT;      // past h in the last tile's idle groups
    const uint8_t* img = xu8 + (size_t)nn * h * w + c;
    const bool col_in = rem > 0;
    const uint32_t pix = (1u << min(rem, 16)) - 1u, pairs_h = (1u << max(rem - 1, 0)) - 1u;      // bit i: pixel i / its right neighbour is in the row
    uint32_t hot = 0u;
    u32x4 cur = mk_u4(0u, 0u, 0u, 0u);
    if (col_in && r0 < h) cur = st_load_strip(img + (size_t)r0 * w, rem);
#pragma unroll 1
    for (int k = 0; k < ST_TRT; ++k) {
        const long long r = r0 + k;
        const bool row_in = col_in && r < h, below = col_in && r + 1 < h;
        const uint32_t mh = row_in ? pairs_h : 0u, mv = below ? pix : 0u;
        const int right = row_in && rem > 16 ? (int)img[(size_t)r * w + 16] : 0;
        u32x4 next = mk_u4(0u, 0u, 0u, 0u);
        if (below) next = st_load_strip(img + (size_t)(r + 1) * w, rem);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int u = st_px(cur, i);
            spa_count(u, i < 15 ? st_px(cur, i + 1) : right, (mh >> i) & 1u, hist[wave], hot);
            spa_count(u, st_px(next, i), (mv >> i) & 1u, hist[wave], hot);
        }
        cur = next;
    }
#pragma unroll
    for (int cls = 0; cls < 3; ++cls) {
        const uint32_t s = st_wave_sum((hot >> (SPA_FIELD * cls)) & ((1u << SPA_FIELD) - 1u));
        if ((tid & 63) == 0 && s) atomicAdd(&hist[wave][cls * 128], s);
    }
    __syncthreads();
    for (int b = tid; b < SPA_BINS; b += ST_THREADS) {
        uint32_t s = 0u;
#pragma unroll
        for (int k = 0; k < ST_WAVES; ++k) s += hist[k][b];
        if (s) atomicAdd(&tables[(size_t)nn * SPA_BINS + b], (unsigned long long)s);
    }
}

__device__ __forceinline__ int rs_f(int g0, int g1, int g2, int g3) { return abs(g1 - g0) + abs(g2 - g1) + abs(g3 - g2); }
__device__ __forceinline__ int rs_fneg(int v) { return ((v + 1) ^ 1) - 1; }

// lanes of the wave for which p holds; every lane of the wave must get here
__device__ __forceinline__ uint32_t st_popc(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// one group per lane, of the plane (flip = 0) or of the plane with every LSB flipped (flip = 1): the wave's cnt[0..3] += R_M, S_M, R_-M, S_-M
__device__ __forceinline__ void rs_count(int g0, int g1, int g2, int g3, int flip, bool valid, uint32_t* cnt) {
    g0 ^= flip; g1 ^= flip; g2 ^= flip; g3 ^= flip;
    const int f = rs_f(g0, g1, g2, g3), fp = rs_f(g0, g1 ^ 1, g2 ^ 1, g3), fn = rs_f(g0, rs_fneg(g1), rs_fneg(g2), g3);
    cnt[0] += st_popc(valid && fp > f);
    cnt[1] += st_popc(valid && fp < f);
    cnt[2] += st_popc(valid && fn > f);
    cnt[3] += st_popc(valid && fn < f);
}

__global__ __launch_bounds__(ST_THREADS) void rs_counts_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ counts,
                                                               int h, int w, int tiles_c) {
    __shared__ uint32_t part[ST_WAVES][RS_COUNTS];
    const int nn = blockIdx.y, tid = threadIdx.x;
    int rem;
    const long long c = st_strip(tiles_c, w, rem);
    const long long r0 = (long long)(blockIdx.x / tiles_c) * ST_ROWS + (tid / ST_STRIPS) * ST_TRT;
    const uint8_t* img = xu8 + (size_t)nn * h * w + c;
    uint32_t cnt[RS_COUNTS];
#pragma unroll
    for (int q = 0; q < RS_COUNTS; ++q) cnt[q] = 0u;
#pragma unroll 1
    for (int k = 0; k < ST_TRT; ++k) {
        const long long r = r0 + k;
        const bool row_in = rem > 0 && r < h;
        u32x4 cur = mk_u4(0u, 0u, 0u, 0u);
        if (row_in) cur = st_load_strip(img + (size_t)r * w, rem);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bool valid = row_in && 4 * g + 4 <= rem;                  // the trailing w % 4 columns belong to no group
            const int g0 = st_px(cur, 4 * g), g1 = st_px(cur, 4 * g + 1), g2 = st_px(cur, 4 * g + 2), g3 = st_px(cur, 4 * g + 3);
            rs_count(g0, g1, g2, g3, 0, valid, cnt);
            rs_count(g0, g1, g2, g3, 1, valid, cnt + 4);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < RS_COUNTS; ++q) part[tid >> 6][q] = cnt[q];
    }
    __syncthreads();
    if (tid < RS_COUNTS) {
        uint32_t s = 0u;
#pragma unroll
        for (int k = 0; k < ST_WAVES; ++k) s += part[k][tid];
        if (s) atomicAdd(&counts[(size_t)nn * RS_COUNTS + tid], (unsigned long long)s);
    }
}

// the grid of both kernels: (row tiles x column tiles, n); 0 after the argument error has been set
long long st_tiles(const char* who, int n, int h, int w, int* tiles_c) {
    if (n < 1 || n > 65535 || h < 1 || w < 1) { wsu_set_error("%s: bad shape n=%d h=%d w=%d", who, n, h, w); return 0; }
    const long long tr = ((long long)h + ST_ROWS - 1) / ST_ROWS, tc = ((long long)w + ST_COLS - 1) / ST_COLS;
    if (tr * tc > 0x7fffffffll) { wsu_set_error("%s: image of %d x %d has too many tiles", who, h, w); return 0; }
    *tiles_c = (int)tc;
    return tr * tc;
}

}  // namespace

extern "C" {

int wsu_spa_tables(const uint8_t* x_u8, unsigned long long* tables, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && tables, "spa_tables: null pointer");
    int tiles_c = 0;
    const long long tiles = st_tiles("spa_tables", n, h, w, &tiles_c);
    if (!tiles) return WSU_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(tables, 0, (size_t)n * SPA_BINS * sizeof(unsigned long long), s) != hipSuccess) return wsu_check_launch("spa_tables memset");
    hipLaunchKernelGGL(spa_tables_kernel, dim3((unsigned)tiles, n), dim3(ST_THREADS), 0, s, x_u8, tables, h, w, tiles_c);
    return wsu_check_launch("spa_tables_kernel");
}

int wsu_rs_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && counts, "rs_counts: null pointer");
    int tiles_c = 0;
    const long long tiles = st_tiles("rs_counts", n, h, w, &tiles_c);
    if (!tiles) return WSU_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(counts, 0, (size_t)n * RS_COUNTS * sizeof(unsigned long long), s) != hipSuccess) return wsu_check_launch("rs_counts memset");
    hipLaunchKernelGGL(rs_counts_kernel, dim3((unsigned)tiles, n), dim3(ST_THREADS), 0, s, x_u8, counts, h, w, tiles_c);
    return wsu_check_launch("rs_counts_kernel");
}

}  // extern "C"
