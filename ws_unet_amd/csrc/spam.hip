// K36: the co-occurrence counts of the subtractive pixel adjacency matrix (SPAM; Pevny, Bas, Fridrich, IEEE TIFS 5(2), 2010), the integer half
// of the feature-based detector of ws_unet_amd/spam.py.  Not part of the reference.
//
//   A direction is a step (dr, dc); the four counted ones, in this order: 0 right (0,+1), 1 down (+1,0), 2 down-right (+1,+1), 3 down-left (+1,-1).
//   D_k(r,c) = clip(x[r + k dr][c + k dc] - x[r + (k+1) dr][c + (k+1) dc], -T, T), k = 0 .. order.  A position (r,c) counts for a direction when
//   all order + 2 pixels of its run lie in the image; it adds 1 to bin  sum_k (D_k + T) B^(order-k),  B = 2T + 1  (D_0 the most significant
//   digit; a difference beyond +-T is clipped into the border bins, not dropped).  counts[n][dir][B^(order+1)].  The four opposite steps need no
//   counting: they see the same runs backwards with every sign flipped (ws_unet_amd.spam.opposite permutes the bins).
//
// Exact integers, so the bits depend on no order.  One workgroup owns a tile of SM_ROWS x SM_COLS positions of one image, laid out as K25's
// (structural.hip): 32 strips of 16 columns by 8 row groups, a thread walking its strip down SM_TRT rows.  The thread keeps a window of
// order + 2 rows in registers, each row as six words: the strip's 16 pixels and the four columns on either side of it (three of them are read
// at order 2).  A row is loaded by one of two paths: whole words where the strip lies inside the row on a 4-byte boundary (the strip as ONE
// 16-byte load where its address is a multiple of 16, the side words as 4-byte loads), else 24 byte loads with the column clamped into the
// row (ragged strips, rows that an odd width has shifted).  No load is outside the image; a run that leaves it only clears a predicate.
//
// The counts go to a private LDS histogram of 4 x B^(order+1) uint32 bins per wave with LDS atomics -- except the all-zero-difference bin of
// each direction (the centre bin), which a constant plane sends EVERY update to: same-address LDS atomics serialise (K25's header has the
// measurement), so those four are counted per lane in the four 8-bit fields of one VGPR and reach the histogram as four adds per wave.
// A workgroup flushes its non-zero sums with one 64-bit vector atomic each; the entry point zeroes the output on the stream first.
// WSU_SPAM_HOT_BINS=0 builds the all-atomics arm of the A/B of tools/bench_spam.py; the product is built without it.
#include "wsu_device.h"

#ifndef WSU_SPAM_HOT_BINS
#define WSU_SPAM_HOT_BINS 1
#endif

namespace {

constexpr int SM_TRT = 4, SM_STRIPS = 32, SM_GROUPS = 8, SM_THREADS = SM_STRIPS * SM_GROUPS, SM_WAVES = SM_THREADS / 64;
constexpr int SM_COLS = SM_STRIPS * 16, SM_ROWS = SM_GROUPS * SM_TRT;
constexpr int SM_DIRS = 4, SM_FIELD = 8;
constexpr bool SM_HOT = WSU_SPAM_HOT_BINS != 0;
static_assert((long long)SM_ROWS * SM_COLS < (1ll << 32), "a tile's 32-bit bins must hold every position of the tile");
static_assert(16 * SM_TRT < (1 << SM_FIELD), "a thread's centre-bin counters must hold every position of the thread");
static_assert(SM_DIRS * SM_FIELD <= 32, "the four centre-bin counters share one register");

// a strip's row: columns c-4 .. c-1 (left), c .. c+15 (mid), c+16 .. c+19 (right), little-endian
struct SmRow { uint32_t left; u32x4 mid; uint32_t right; };

__device__ __forceinline__ SmRow sm_no_row() { SmRow r; r.left = 0u; r.mid = mk_u4(0u, 0u, 0u, 0u); r.right = 0u; return r; }

// the window row of the strip at column c < w of the image row `row`, by ONE decision per row (a decision per word made every word wait for
// the one before it).  Words: the strip is whole (c + 16 <= w), its address a multiple of 4 and the word right of it whole or wholly outside
// the row.  A side word outside the row (left of the first strip, right of a strip that ends the row) belongs to no counted run, so the
// strip's own first / last word is read in its place.  Bytes: everything else, 24 loads with the column clamped into the row.
__device__ __forceinline__ SmRow sm_load_row(const uint8_t* __restrict__ row, long long c, int w) {
    const uint8_t* p = row + c;
    SmRow r;
    if ((c + 20 <= w || c + 16 == w) && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        r.left = *reinterpret_cast<const uint32_t*>(p - (c > 0 ? 4 : 0));
        r.right = *reinterpret_cast<const uint32_t*>(p + (c + 20 <= w ? 16 : 12));
        if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            r.mid = *reinterpret_cast<const u32x4*>(p);
        } else {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
            r.mid = mk_u4(q[0], q[1], q[2], q[3]);
        }
    } else {
        uint32_t v[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 24; ++i) v[i >> 2] |= (uint32_t)row[min(max(c - 4 + i, 0ll), (long long)w - 1)] << (8 * (i & 3));
        r.left = v[0];
        r.mid = mk_u4(v[1], v[2], v[3], v[4]);
        r.right = v[5];
    }
    return r;
}

// pixel at column c + i of the row, i = -4 .. 19
__device__ __forceinline__ int sm_px(const SmRow& r, int i) {
    const uint32_t wd = i < 0 ? r.left : i < 16 ? r.mid[i >> 2] : r.right;
    return (int)((wd >> (8 * (i & 3))) & 255u);
}

// sum over the wave, valid in its lane 0
__device__ __forceinline__ uint32_t sm_wave_sum(uint32_t s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return s;
}

// the run from window position (row 0, column c + i) along (DR, DC): its bin, counted when `valid`
template <int ORDER, int DIR, int DR, int DC>
__device__ __forceinline__ void sm_count(const SmRow (&win)[ORDER + 2], int i, bool valid, int T, int B, int centre, uint32_t* __restrict__ hist,
                                         uint32_t& hot) {
    int bin = 0;
#pragma unroll
    for (int k = 0; k <= ORDER; ++k) {
        const int d = sm_px(win[k * DR], i + k * DC) - sm_px(win[(k + 1) * DR], i + (k + 1) * DC);
        bin = bin * B + min(max(d, -T), T) + T;
    }
    if (SM_HOT) {
        hot += valid && bin == centre ? 1u << (SM_FIELD * DIR) : 0u;
        if (valid && bin != centre) atomicAdd(&hist[bin], 1u);
    } else if (valid) {
        atomicAdd(&hist[bin], 1u);
    }
}

template <int ORDER>
__global__ __launch_bounds__(SM_THREADS) void spam_counts_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ counts,
                                                                 int h, int w, int tiles_c, int T, int bins) {
    extern __shared__ uint32_t hist[];                  // [SM_WAVES][SM_DIRS][bins]
    constexpr int REACH = ORDER + 1;                    // a run's last pixel is this many steps from its first
    const int nn = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, B = 2 * T + 1, centre = (bins - 1) / 2;
    const long long c = (long long)(blockIdx.x % tiles_c) * SM_COLS + (tid & (SM_STRIPS - 1)) * 16;
    const long long r0 = (long long)(blockIdx.x / tiles_c) * SM_ROWS + (tid / SM_STRIPS) * SM_TRT;      // past h in the last tile's idle groups
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const bool col_in = c < w;
    const int rem = (int)min(max((long long)w - c, 0ll), (long long)(16 + REACH));
    // bit i: column c + i is in the row / so is c + i + REACH / so is c + i - REACH (c is a multiple of 16: only the first strip lacks columns)
    const uint32_t m_in = (1u << min(rem, 16)) - 1u, m_right = (1u << max(rem - REACH, 0)) - 1u;
    const uint32_t m_left = c > 0 ? m_in : m_in & ~((1u << REACH) - 1u);
    uint32_t* hw = hist + wave * SM_DIRS * bins;
    uint32_t hot = 0u;
    SmRow win[ORDER + 2];
#pragma unroll
    for (int j = 0; j < ORDER + 2; ++j) win[j] = col_in && r0 + j < h ? sm_load_row(img + (size_t)(r0 + j) * w, c, w) : sm_no_row();
    for (int i = tid; i < SM_WAVES * SM_DIRS * bins; i += SM_THREADS) hist[i] = 0u;      // (behind the window's loads)
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < SM_TRT; ++k) {
        const long long r = r0 + k;
        const bool row_in = col_in && r < h, below = col_in && r + REACH < h;
        const uint32_t mh = row_in ? m_right : 0u, mv = below ? m_in : 0u, md = below ? m_right : 0u, ma = below ? m_left : 0u;
        SmRow next = sm_no_row();
        if (k + 1 < SM_TRT && col_in && r + REACH + 1 < h) next = sm_load_row(img + (size_t)(r + REACH + 1) * w, c, w);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sm_count<ORDER, 0, 0, 1>(win, i, (mh >> i) & 1u, T, B, centre, hw, hot);
            sm_count<ORDER, 1, 1, 0>(win, i, (mv >> i) & 1u, T, B, centre, hw + bins, hot);
            sm_count<ORDER, 2, 1, 1>(win, i, (md >> i) & 1u, T, B, centre, hw + 2 * bins, hot);
            sm_count<ORDER, 3, 1, -1>(win, i, (ma >> i) & 1u, T, B, centre, hw + 3 * bins, hot);
        }
#pragma unroll
        for (int j = 0; j < ORDER + 1; ++j) win[j] = win[j + 1];
        win[ORDER + 1] = next;
    }
    if (SM_HOT) {
#pragma unroll
        for (int dir = 0; dir < SM_DIRS; ++dir) {
            const uint32_t s = sm_wave_sum((hot >> (SM_FIELD * dir)) & ((1u << SM_FIELD) - 1u));
            if ((tid & 63) == 0 && s) atomicAdd(&hw[dir * bins + centre], s);
        }
    }
    __syncthreads();
    for (int b = tid; b < SM_DIRS * bins; b += SM_THREADS) {
        uint32_t s = 0u;
#pragma unroll
        for (int k = 0; k < SM_WAVES; ++k) s += hist[k * SM_DIRS * bins + b];
        if (s) atomicAdd(&counts[(size_t)nn * SM_DIRS * bins + b], (unsigned long long)s);
    }
}

}  // namespace

extern "C" {

int wsu_spam_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, int order, int T, void* stream) {
    WSU_REQUIRE(x_u8 && counts, "spam_counts: null pointer");
    WSU_REQUIRE(order == 1 || order == 2, "spam_counts: order=%d outside {1,2}", order);
    WSU_REQUIRE(T >= 1 && T <= (order == 1 ? 8 : 4), "spam_counts: T=%d outside 1..%d at order %d", T, order == 1 ? 8 : 4, order);
    WSU_REQUIRE(n >= 1 && n <= 65535 && h >= 1 && w >= 1, "spam_counts: bad shape n=%d h=%d w=%d", n, h, w);
    const long long tr = ((long long)h + SM_ROWS - 1) / SM_ROWS, tc = ((long long)w + SM_COLS - 1) / SM_COLS;
    WSU_REQUIRE(tr * tc <= 0x7fffffffll, "spam_counts: image of %d x %d has too many tiles", h, w);
    const int B = 2 * T + 1, bins = order == 1 ? B * B : B * B * B;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(counts, 0, (size_t)n * SM_DIRS * bins * sizeof(unsigned long long), s) != hipSuccess) return wsu_check_launch("spam_counts memset");
    const size_t lds = (size_t)SM_WAVES * SM_DIRS * bins * sizeof(uint32_t);         // at most 46 656 bytes (order 2, T 4)
    if (order == 1)
        hipLaunchKernelGGL(spam_counts_kernel<1>, dim3((unsigned)(tr * tc), n), dim3(SM_THREADS), lds, s, x_u8, counts, h, w, (int)tc, T, bins);
    else
        hipLaunchKernelGGL(spam_counts_kernel<2>, dim3((unsigned)(tr * tc), n), dim3(SM_THREADS), lds, s, x_u8, counts, h, w, (int)tc, T, bins);
    return wsu_check_launch("spam_counts_kernel");
}

}  // extern "C"
