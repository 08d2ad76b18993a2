// K24: the moments of the least-squares 3x3 pixel predictor (ws_unet_amd/ols.py).
//
//   At every interior pixel (r, c) of an image, 1 <= r <= h-2, 1 <= c <= w-2, with xab = x[r-1+a][c-1+b]:
//     v = [x00 x01 x02 x12 x22 x21 x20 x10 x11]      the ring order of the flattened 8-tap filters (_defs/filters.py:57-67), centre last
//   moments[n][45] = sum over the interior of v_i * v_j, 0 <= i <= j <= 8, row-major upper triangle: the Gram matrix A = X^T X of the
//   eight neighbours, b = X^T y (the column j = 8) and y^T y (the last entry).  The host solves A k = b in float64.
//
// The sums are exact unsigned integers, so their bits depend on no order.  One workgroup owns a tile of OLS_TR x OLS_TC interior pixels,
// one column per thread, walking down the rows with a 3x3 register window (three byte loads per pixel).  32-bit accumulators suffice for
// the WHOLE tile, not only for a thread: a product is at most 255 * 255 = 65 025, and 2^32 / 65 025 = 66 051.3, so a 32-bit sum holds
// 66 051 products whatever the pixels; a tile has OLS_TR * OLS_TC = 16 384 of them (a thread's own accumulator sees at most OLS_TR = 64).
// The tile's 45 sums leave through the wave fold, the flush and the launch set-up of the count kernels (wsu_count.h).
// HBM-bound in principle (1 B per pixel); at 45 integer multiply-adds per pixel the VALU is the longer pole.
#include "wsu_count.h"

namespace {

constexpr int OLS_TR = 64, OLS_TC = 256, OLS_M = 45;
static_assert((long long)OLS_TR * OLS_TC * 255 * 255 < (1ll << 32), "a tile's 32-bit sums must hold every product of the tile");

__global__ __launch_bounds__(OLS_TC) void ols_moments_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ moments,
                                                             int h, int w, int tiles_c) {
    __shared__ uint32_t part[OLS_TC / 64][OLS_M];
    const int nn = blockIdx.y, tid = threadIdx.x;
    const int r0 = 1 + (int)(blockIdx.x / tiles_c) * OLS_TR, c = 1 + (int)(blockIdx.x % tiles_c) * OLS_TC + tid;
    const int r1 = min(r0 + OLS_TR, h - 1);                     // one past the tile's last interior row
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    uint32_t acc[OLS_M];
#pragma unroll
    for (int m = 0; m < OLS_M; ++m) acc[m] = 0u;
    if (c <= w - 2) {
        const uint8_t* p = img + (size_t)(r0 - 1) * w + (c - 1);
        uint32_t t0 = p[0], t1 = p[1], t2 = p[2];               // row r-1
        p += w;
        uint32_t m0 = p[0], m1 = p[1], m2 = p[2];               // row r
        for (int r = r0; r < r1; ++r) {
            p += w;
            const uint32_t b0 = p[0], b1 = p[1], b2 = p[2];     // row r+1
            const uint32_t v[9] = {t0, t1, t2, m2, b2, b1, b0, m0, m1};
            int m = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j) acc[m++] += v[i] * v[j];
            t0 = m0; t1 = m1; t2 = m2;
            m0 = b0; m1 = b1; m2 = b2;
        }
    }
#pragma unroll
    for (int m = 0; m < OLS_M; ++m) {
        const uint32_t s = wave_sum(acc[m]);
        if ((tid & 63) == 0) part[tid >> 6][m] = s;
    }
    count_flush<OLS_TC / 64>(&part[0][0], OLS_M, moments, (size_t)nn * OLS_M);
}

}  // namespace

extern "C" {

int wsu_ols_moments(const uint8_t* x_u8, unsigned long long* moments, int n, int h, int w, void* stream) {
    return count_launch("ols_moments", "ols_moments memset", "ols_moments_kernel", ols_moments_kernel, OLS_TC, 0, x_u8, moments, OLS_M, n, h, w, 1, OLS_TR, OLS_TC, stream);
}

}  // extern "C"
