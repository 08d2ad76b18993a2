// K56, K57: the 5x5 least-squares pixel predictor of Ker and Boehme's improved WS (ws_unet_amd/ols5.py) -- its moments and its prediction.
//
//   The 25 variables at a pixel (r, c) with a full 5x5 window, 2 <= r <= h-3, 2 <= c <= w-3:
//     v[0..23] = the 24 neighbours x[r-2+a][c-2+b] in raster order of (a, b), the centre skipped;  v[24] = the centre x[r][c]
//
// K56  moments[n][325] = sum over those pixels of v_p * v_q, 0 <= p <= q <= 24, row-major upper triangle: K24's layout with 25 variables
//   in place of 9 -- the Gram matrix A = X^T X of the neighbours, b = X^T y (the column q = 24) and y^T y (the last entry).  The sums are
//   exact unsigned integers, so their bits depend on no order.  One workgroup owns a tile of O5_TR x O5_TC such pixels, one column per
//   thread, walking down the rows with a 5x5 register window (five byte loads per pixel).  325 accumulators do not fit a thread, so the
//   triangle is cut by its first index p into O5_SLICES slices of 72 .. 91 sums (o5_first), one workgroup per tile AND slice (grid z):
//   each walks the tile again and keeps only its rows of the triangle.  32-bit accumulators suffice for the whole tile as in K24
//   (16 384 products of at most 65 025); the sums leave through the wave fold, the flush and the launch set-up of the count kernels
//   (wsu_count.h).  No load is outside the image: the tile's windows reach rows r0-2 .. r1+1 <= h-1 and columns c-2 .. c+2 <= w-1.
//
// K57  x_hat (and x_bias) full frames in pixel units from 24 float32 taps, shared or one row per image, in K11's float32 operation
//   sequence (plain operators, one rounding each; q(u) = (float)u / 255.0f from a table of 256 quotients, one IEEE division per thread):
//     frame border               0
//     ring 1 (the 5x5 window leaves the image)   KB's 3x3 taps, conv9_f32<true> on q, times 255.0f: what K11 computes for pixel_filter = KB
//     elsewhere                  acc = 0; for k = 23 .. 0: acc = acc + taps[k] * q(v[k]); x_hat = acc * 255.0f
//   x_bias: the same with qb(u) = (u & 1) ? -q(1) : q(1), the predictor applied to x_bar - x.  A thread owns one column of a tile of
//   P5_TR x P5_TC pixels and slides a 5x5 window of quotients down it; window positions outside the image repeat the nearest pixel and
//   are read by no case that uses them.  Every output element is written, by plain vector stores.
#pragma clang fp contract(off)
#include "wsu_count.h"
#include "wsu_metric.h"

namespace {

// ---- K56 ------------------------------------------------------------------------------------------------------------------------------
constexpr int O5_TR = 64, O5_TC = 256, O5_V = 25, O5_M = O5_V * (O5_V + 1) / 2, O5_SLICES = 4;
static_assert((long long)O5_TR * O5_TC * 255 * 255 < (1ll << 32), "a tile's 32-bit sums must hold every product of the tile");
// slice s holds the rows o5_first(s) <= p < o5_first(s + 1) of the triangle; row p starts at o5_offset(p) and has 25 - p sums
constexpr int o5_first(int s) { return s <= 0 ? 0 : s == 1 ? 3 : s == 2 ? 7 : s == 3 ? 12 : O5_V; }
constexpr int o5_offset(int p) { return p * O5_V - p * (p - 1) / 2; }
constexpr int o5_sums(int s) { return o5_offset(o5_first(s + 1)) - o5_offset(o5_first(s)); }
constexpr int O5_PART = 91;                                      // the longest slice
static_assert(o5_offset(O5_V) == O5_M && O5_M == 325, "the slices cover the triangle");
static_assert(o5_sums(0) <= O5_PART && o5_sums(1) <= O5_PART && o5_sums(2) <= O5_PART && o5_sums(3) <= O5_PART, "a slice fits the partial table");
// variable k's place in the 5x5 window in raster order
constexpr int o5_at(int k) { return k == 24 ? 12 : k < 12 ? k : k + 1; }

template <int S> __device__ __forceinline__ void ols5_slice(const uint8_t* __restrict__ img, unsigned long long* __restrict__ moments,
                                                            uint32_t* part, int nn, int w, int r0, int r1, int c, bool live) {
    constexpr int P0 = o5_first(S), P1 = o5_first(S + 1), M = o5_sums(S);
    const int tid = threadIdx.x;
    uint32_t acc[M];
#pragma unroll
    for (int m = 0; m < M; ++m) acc[m] = 0u;
    if (live) {
        const uint8_t* p = img + (size_t)(r0 - 2) * w + (c - 2);
        uint32_t wn[25];                                        // rows r-2 .. r+2 of the window; the last one is loaded in the loop
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b < 5; ++b) wn[a * 5 + b] = p[b];
            p += w;
        }
        for (int r = r0; r < r1; ++r) {
#pragma unroll
            for (int b = 0; b < 5; ++b) wn[20 + b] = p[b];      // row r+2
            p += w;
            int m = 0;
#pragma unroll
            for (int i = P0; i < P1; ++i)
#pragma unroll
                for (int j = i; j < O5_V; ++j) acc[m++] += __umul24(wn[o5_at(i)], wn[o5_at(j)]);   // bytes: one 24-bit multiply-add
#pragma unroll
            for (int i = 0; i < 20; ++i) wn[i] = wn[i + 5];
        }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const uint32_t s = wave_sum(acc[m]);
        if ((tid & 63) == 0) part[(tid >> 6) * M + m] = s;
    }
    count_flush<O5_TC / 64>(part, M, moments, (size_t)nn * O5_M + o5_offset(P0));
}

__global__ __launch_bounds__(O5_TC) void ols_moments5_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ moments,
                                                              int h, int w, int tiles_c) {
    __shared__ uint32_t part[(O5_TC / 64) * O5_PART];
    const int nn = blockIdx.y;
    const int r0 = 2 + (int)(blockIdx.x / tiles_c) * O5_TR, c = 2 + (int)(blockIdx.x % tiles_c) * O5_TC + (int)threadIdx.x;
    const int r1 = min(r0 + O5_TR, h - 2);                      // one past the tile's last row with a full window
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const bool live = c <= w - 3;
    switch (blockIdx.z) {                                       // (uniform over the workgroup)
        case 0: ols5_slice<0>(img, moments, part, nn, w, r0, r1, c, live); break;
        case 1: ols5_slice<1>(img, moments, part, nn, w, r0, r1, c, live); break;
        case 2: ols5_slice<2>(img, moments, part, nn, w, r0, r1, c, live); break;
        default: ols5_slice<3>(img, moments, part, nn, w, r0, r1, c, live); break;
    }
}

// ---- K57 ------------------------------------------------------------------------------------------------------------------------------
constexpr int P5_TR = 16, P5_TC = 256, P5_TAPS = 24;

__global__ __launch_bounds__(P5_TC) void predict5x5_kernel(const uint8_t* __restrict__ xu8, const float* __restrict__ taps, int per_image,
                                                            float* __restrict__ xhat, float* __restrict__ xbias, int h, int w, int tiles_c) {
    __shared__ float unit[256];
    const int tid = threadIdx.x, nn = blockIdx.y;
    unit[tid] = (float)tid / 255.0f;
    __syncthreads();
    const int r0 = (int)(blockIdx.x / tiles_c) * P5_TR, c = (int)(blockIdx.x % tiles_c) * P5_TC + tid;
    if (c >= w) return;
    const int r1 = min(r0 + P5_TR, h);
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    float* hat = xhat + (size_t)nn * h * w;
    float* bias = xbias ? xbias + (size_t)nn * h * w : nullptr;
    const float* tp = taps + (per_image ? (size_t)nn * P5_TAPS : (size_t)0);
    float t[P5_TAPS];
#pragma unroll
    for (int k = 0; k < P5_TAPS; ++k) t[k] = tp[k];
    const Taps3x3<float> kb = kb_taps_f32();
    const float b1 = unit[1];
    int cc[5];                                                  // the window's columns, kept inside the row
#pragma unroll
    for (int b = 0; b < 5; ++b) cc[b] = min(max(c - 2 + b, 0), w - 1);
    float q[25], qb[25];                                        // q(u) and qb(u) of rows r-2 .. r+2, rows kept inside the image
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const uint8_t* row = img + (size_t)min(max(r0 - 2 + a, 0), h - 1) * w;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const uint32_t u = row[cc[b]];
            q[a * 5 + b] = unit[u];
            qb[a * 5 + b] = (u & 1u) ? -b1 : b1;
        }
    }
    const bool side = c == 0 || c == w - 1, near = c == 1 || c == w - 2;
    for (int r = r0; r < r1; ++r) {
        const uint8_t* row = img + (size_t)min(r + 2, h - 1) * w;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const uint32_t u = row[cc[b]];
            q[20 + b] = unit[u];
            qb[20 + b] = (u & 1u) ? -b1 : b1;
        }
        float y = 0.f, yb = 0.f;
        if (side || r == 0 || r == h - 1) {
            // the frame border: no statistic reads it
        } else if (near || r == 1 || r == h - 2) {
            float v[3][3], vb[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    v[i][j] = q[(i + 1) * 5 + (j + 1)];
                    vb[i][j] = qb[(i + 1) * 5 + (j + 1)];
                }
            y = conv9_f32<true>(kb, v) * 255.0f;
            if (bias) yb = conv9_f32<true>(kb, vb) * 255.0f;
        } else {
            float acc = 0.f;
#pragma unroll
            for (int k = P5_TAPS - 1; k >= 0; --k) acc = acc + t[k] * q[o5_at(k)];
            y = acc * 255.0f;
            if (bias) {
                float accb = 0.f;
#pragma unroll
                for (int k = P5_TAPS - 1; k >= 0; --k) accb = accb + t[k] * qb[o5_at(k)];
                yb = accb * 255.0f;
            }
        }
        hat[(size_t)r * w + c] = y;
        if (bias) bias[(size_t)r * w + c] = yb;
#pragma unroll
        for (int i = 0; i < 20; ++i) {
            q[i] = q[i + 5];
            qb[i] = qb[i + 5];
        }
    }
}

}  // namespace

extern "C" {

int wsu_ols_moments5(const uint8_t* x_u8, unsigned long long* moments, int n, int h, int w, void* stream) {
    return count_launch_slices("ols_moments5", "ols_moments5 memset", "ols_moments5_kernel", ols_moments5_kernel, O5_TC, 0, x_u8, moments, O5_M,
                               n, h, w, 2, O5_TR, O5_TC, O5_SLICES, stream);
}

int wsu_predict5x5(const uint8_t* x_u8, const float* taps, int per_image, float* x_hat, float* x_bias, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && taps && x_hat, "predict5x5: null pointer");
    WSU_REQUIRE(n >= 1 && n <= 65535 && h >= 3 && w >= 3, "predict5x5: bad shape n=%d h=%d w=%d", n, h, w);
    const long long tr = ((long long)h + P5_TR - 1) / P5_TR, tc = ((long long)w + P5_TC - 1) / P5_TC;
    WSU_REQUIRE(tr * tc <= 0x7fffffffll, "predict5x5: image of %d x %d has too many tiles", h, w);
    hipLaunchKernelGGL(predict5x5_kernel, dim3((unsigned)(tr * tc), n), dim3(P5_TC), 0, static_cast<hipStream_t>(stream), x_u8, taps, per_image,
                       x_hat, x_bias, h, w, (int)tc);
    return wsu_check_launch("predict5x5_kernel");
}

}  // extern "C"
