// K36: the co-occurrence counts of the subtractive pixel adjacency matrix (SPAM; Pevny, Bas, Fridrich, IEEE TIFS 5(2), 2010), the integer half
// of the feature-based detector of ws_unet_amd/spam.py.  Not part of the reference.
//
//   A direction is a step (dr, dc); the four counted ones, in this order: 0 right (0,+1), 1 down (+1,0), 2 down-right (+1,+1), 3 down-left (+1,-1).
//   D_k(r,c) = clip(x[r + k dr][c + k dc] - x[r + (k+1) dr][c + (k+1) dc], -T, T), k = 0 .. order.  A position (r,c) counts for a direction when
//   all order + 2 pixels of its run lie in the image; it adds 1 to bin  sum_k (D_k + T) B^(order-k),  B = 2T + 1  (D_0 the most significant
//   digit; a difference beyond +-T is clipped into the border bins, not dropped).  counts[n][dir][B^(order+1)].  The four opposite steps need no
//   counting: they see the same runs backwards with every sign flipped (ws_unet_amd.spam.opposite permutes the bins).
//
// A count kernel on the strip tile of wsu_count.h, which has the tile, the loads, the register counters and the flush.  The thread keeps a
// window of order + 2 rows in registers, each a CtRow: the strip's 16 pixels and the four columns on either side of it (three of them are
// read at order 2).  The counts go to a private LDS histogram of 4 x B^(order+1) uint32 bins per wave with LDS atomics -- except the
// all-zero-difference bin of each direction (the centre bin), which a constant plane sends EVERY update to: those four are HotBins fields
// (profiles/r29 has the A/B against all LDS atomics).
#include "wsu_count.h"

namespace {

constexpr int SM_DIRS = 4;
static_assert((long long)CT_ROWS * CT_COLS < (1ll << 32), "a tile's 32-bit bins must hold every position of the tile");
using SmHot = HotBins<SM_DIRS, 8, 16 * CT_TRT>;         // one field per direction; a thread sees 16 * CT_TRT positions

// the run from window position (row 0, column c + i) along (DR, DC): its bin, counted when `valid`
template <int ORDER, int DIR, int DR, int DC>
__device__ __forceinline__ void sm_count(const CtRow (&win)[ORDER + 2], int i, bool valid, int T, int B, int centre, uint32_t* __restrict__ hist,
                                         SmHot& hot) {
    int bin = 0;
#pragma unroll
    for (int k = 0; k <= ORDER; ++k) {
        const int d = ct_px(win[k * DR], i + k * DC) - ct_px(win[(k + 1) * DR], i + (k + 1) * DC);
        bin = bin * B + min(max(d, -T), T) + T;
    }
    hot.add(DIR, valid && bin == centre);
    if (valid && bin != centre) atomicAdd(&hist[bin], 1u);
}

template <int ORDER>
__global__ __launch_bounds__(CT_THREADS) void spam_counts_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ counts,
                                                                 int h, int w, int tiles_c, int T, int bins) {
    extern __shared__ uint32_t hist[];                  // [CT_WAVES][SM_DIRS][bins]
    constexpr int REACH = ORDER + 1;                    // a run's last pixel is this many steps from its first
    const int nn = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, B = 2 * T + 1, centre = (bins - 1) / 2;
    const CtStrip st = ct_strip(tiles_c, w, REACH);
    const long long c = st.c, r0 = st.r0;
    const int rem = st.rem;
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const bool col_in = c < w;
    // bit i: column c + i is in the row / so is c + i + REACH / so is c + i - REACH (c is a multiple of 16: only the first strip lacks columns)
    const uint32_t m_in = (1u << min(rem, 16)) - 1u, m_right = (1u << max(rem - REACH, 0)) - 1u;
    const uint32_t m_left = c > 0 ? m_in : m_in & ~((1u << REACH) - 1u);
    uint32_t* hw = hist + wave * SM_DIRS * bins;
    SmHot hot;
    CtRow win[ORDER + 2];
#pragma unroll
    for (int j = 0; j < ORDER + 2; ++j) win[j] = col_in && r0 + j < h ? ct_load_row(img + (size_t)(r0 + j) * w, c, w) : ct_no_row();
    for (int i = tid; i < CT_WAVES * SM_DIRS * bins; i += CT_THREADS) hist[i] = 0u;      // (behind the window's loads)
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < CT_TRT; ++k) {
        const long long r = r0 + k;
        const bool row_in = col_in && r < h, below = col_in && r + REACH < h;
        const uint32_t mh = row_in ? m_right : 0u, mv = below ? m_in : 0u, md = below ? m_right : 0u, ma = below ? m_left : 0u;
        CtRow next = ct_no_row();
        if (k + 1 < CT_TRT && col_in && r + REACH + 1 < h) next = ct_load_row(img + (size_t)(r + REACH + 1) * w, c, w);
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
    hot.fold(hw + centre, bins);
    count_flush<CT_WAVES>(hist, SM_DIRS * bins, counts, (size_t)nn * SM_DIRS * bins);
}

}  // namespace

extern "C" {

int wsu_spam_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, int order, int T, void* stream) {
    WSU_REQUIRE(order == 1 || order == 2, "spam_counts: order=%d outside {1,2}", order);
    WSU_REQUIRE(T >= 1 && T <= (order == 1 ? 8 : 4), "spam_counts: T=%d outside 1..%d at order %d", T, order == 1 ? 8 : 4, order);
    const int B = 2 * T + 1, bins = order == 1 ? B * B : B * B * B;
    const size_t lds = (size_t)CT_WAVES * SM_DIRS * bins * sizeof(uint32_t);         // at most 46 656 bytes (order 2, T 4)
    return count_launch("spam_counts", "spam_counts memset", "spam_counts_kernel", order == 1 ? spam_counts_kernel<1> : spam_counts_kernel<2>,
                        CT_THREADS, lds, x_u8, counts, (size_t)SM_DIRS * bins, n, h, w, 0, CT_ROWS, CT_COLS, stream, T, bins);
}

}  // extern "C"
