// K48: the directional wavelet cost map that S-UNIWARD and WOW share (include/wsu.h gives the definition, tests/costs_np.py restates it):
//
//   X~       = the cover as float64, numpy.pad(mode='symmetric') (the periodic fold of K20)
//   r_b[y,n] = sum_v b[v] X~[y, n+8-v]              W_k[m,n] = sum_u a_k[u] r_bk[m+8-u, n]          (a,b) = (l,h), (h,l), (h,h)
//   g_k      = 1 / (|W_k| + sigma)  (S-UNIWARD)     |W_k|  (WOW)
//   t_k[m,j] = sum_v |b_k[v]| g_k[m, j-8+v]         xi_k[i,j] = sum_u |a_k[u]| t_k[i-8+u, j]
//   rho      = (xi_1 + xi_2) + xi_3  (S-UNIWARD)    (1/xi_1 + 1/xi_2) + 1/xi_3  (WOW);   rho <= clamp ? rho : clamp
//
// Every sum starts at +0.0 and takes its 16 taps in ascending order, a product and its addition are two roundings, the divisions are
// IEEE divisions and no library function is called: the plane equals the numpy restatement bit for bit, whatever the batch.
//
// One workgroup of 256 threads per 32 x 32 output tile.  In the tile's own coordinates (window row wy = image row r0 - 15 + wy):
//   xs  63 x 63 bytes   the window, staged through the fold or, well inside the image, as 16-byte row segments (hill_stage_window)
//   R   63 x 48         one row-filtered plane at a time: r_h serves bands 1 and 3, then r_l replaces it for band 2
//   gT  48 x 48         g_k, transposed (column-major), so that the row back-projection reads down its lanes
//   tT  32 x 48         t_k, transposed; the column back-projection leaves xi_k in registers, four rows of one column per thread
// 48 = the 47 rows / columns a tile needs, rounded up to whole runs of four: a thread makes four consecutive outputs of a filter from 19
// inputs it reads once.  gT and tT have the odd row stride 49, so lanes that walk a column of the transposed planes fall in different
// LDS banks.  58.2 KB of LDS: two workgroups per compute unit.  The taps are compile-time constants (no table in memory).
#pragma clang fp contract(off)
#include "wsu_metric.h"

namespace {

// The Daubechies-8 scaling filter p[0..15] (tools/db8_taps.py derives it and rounds it so that the float64 values' eight moments vanish to
// 2.4e-13; ws_unet_amd.costs.DB8 holds the same literals)
constexpr double DB8[16] = {
    0.054415842243104008, 0.31287159091429984, 0.67563073629728998, 0.58535468365420684,
    -0.015829105256349302, -0.28401554296154691, 0.00047248457391328307, 0.12874742662047847,
    -0.017369301001807547, -0.044088253930794755, 0.013981027917398282, 0.0087460940474057766,
    -0.0048703529934515741, -0.00039174037337694705, 0.00067544940645056922, -0.00011747678412476953};

constexpr int F_L = 0, F_H = 1;        // l[j] = p[15 - j],  h[j] = (-1)^(j+1) p[j]
template <int F, bool ABS, int J> struct Tap {
    static constexpr double raw = F == F_L ? DB8[15 - J] : ((J & 1) ? DB8[J] : -DB8[J]);
    static constexpr double value = (ABS && raw < 0) ? -raw : raw;
};

constexpr int WT = 32;                 // output tile
constexpr int WX = WT + 31;            // staged window: 15 before the tile, 14 behind it, one more for the whole runs
constexpr int WXS = WT + 32;           // its LDS row stride in bytes; window column wc lives at wc + 1
constexpr int WM = WT + 16;            // columns of R, rows and columns of g, rows of t
constexpr int WS = WM + 1;             // row stride of the transposed planes
constexpr int RUNS = WM / 4;

// four consecutive outputs of a 16-tap filter from the 19 inputs under them.  FWD: o[e] = sum_v c[v] x[e + 15 - v] (the transform's
// convolution); else o[e] = sum_v c[v] x[e + v] (the back-projection's correlation)
template <int F, bool ABS, bool FWD> __device__ __forceinline__ void fir4(const double (&x)[19], double (&o)[4]) {
    WSU_STATIC_FOR(4, e, {
        double s = 0.0;
        WSU_STATIC_FOR(16, v, { s = s + Tap<F, ABS, v>::value * x[FWD ? e + 15 - v : e + v]; });
        o[e] = s;
    });
}

// r_b of the staged window: R[wy][q] = sum_v b[v] xs[wy][q + 15 - v]
template <int FB> __device__ __forceinline__ void row_transform(const uint8_t* xs, double* R, int tid) {
    for (int i = tid; i < WX * RUNS; i += 256) {
        const int run = i % RUNS, wy = i / RUNS;
        const uint32_t* rw = reinterpret_cast<const uint32_t*>(xs + wy * WXS) + run;      // bytes 1 .. 19 of these five words
        uint32_t wd[5];
        WSU_STATIC_FOR(5, k, { wd[k] = rw[k]; });
        double x[19], o[4];
        WSU_STATIC_FOR(19, k, { x[k] = (double)((wd[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xFFu); });
        fir4<FB, false, true>(x, o);
        WSU_STATIC_FOR(4, e, { R[wy * WM + run * 4 + e] = o[e]; });
    }
}

// one band: W_k from R, g_k, t_k, and xi_k of this thread's four pixels (column tid % 32, rows 4 (tid / 32) ..)
template <int KIND, int FA, int FB> __device__ __forceinline__ void band(const double* R, double* gT, double* tT, double sigma, int tid,
                                                                         double (&xi)[4]) {
    for (int i = tid; i < WM * RUNS; i += 256) {
        const int q = i % WM, p0 = (i / WM) * 4;
        double x[19], o[4];
        WSU_STATIC_FOR(19, k, { x[k] = R[(p0 + k) * WM + q]; });
        fir4<FA, false, true>(x, o);
        WSU_STATIC_FOR(4, e, {
            const double a = __builtin_fabs(o[e]);
            gT[q * WS + p0 + e] = KIND == WSU_COST_WOW ? a : 1.0 / (a + sigma);
        });
    }
    __syncthreads();
    for (int i = tid; i < WM * (WT / 4); i += 256) {
        const int p = i % WM, j0 = (i / WM) * 4;
        double x[19], o[4];
        WSU_STATIC_FOR(19, k, { x[k] = gT[(j0 + k) * WS + p]; });
        fir4<FB, true, false>(x, o);
        WSU_STATIC_FOR(4, e, { tT[(j0 + e) * WS + p] = o[e]; });
    }
    __syncthreads();
    {
        const int jj = tid % WT, i0 = (tid / WT) * 4;
        double x[19];
        WSU_STATIC_FOR(19, k, { x[k] = tT[jj * WS + i0 + k]; });
        fir4<FA, true, false>(x, xi);
    }
}

template <int KIND> __global__ __launch_bounds__(256) void wavelet_cost_kernel(const uint8_t* __restrict__ x, double* __restrict__ rho,
                                                                               int h, int w, int vec_in, double sigma, double clamp) {
    __shared__ __attribute__((aligned(16))) uint8_t xs[WX * WXS];
    __shared__ double R[WX * WM];
    __shared__ double gT[WM * WS];
    __shared__ double tT[WT * WS];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * WT, r0 = blockIdx.y * WT, nn = blockIdx.z;
    const uint8_t* img = x + (size_t)nn * h * w;

    // ---- the window: rows r0 - 15 .. r0 + 47, columns c0 - 15 .. c0 + 47
    hill_stage_window<WT, 15, WX>(img, xs, r0, c0, h, w, vec_in, tid);
    __syncthreads();
    double xi1[4], xi2[4], xi3[4];
    row_transform<F_H>(xs, R, tid);
    __syncthreads();
    band<KIND, F_L, F_H>(R, gT, tT, sigma, tid, xi1);          // (a,b)_1 = (l,h)
    band<KIND, F_H, F_H>(R, gT, tT, sigma, tid, xi3);          // (a,b)_3 = (h,h): the barriers inside `band` order every reuse of gT and tT
    row_transform<F_L>(xs, R, tid);                            // (every thread is past band 3's reads of R: the barrier after them)
    __syncthreads();
    band<KIND, F_H, F_L>(R, gT, tT, sigma, tid, xi2);          // (a,b)_2 = (h,l)

    const int col = c0 + tid % WT, row0 = r0 + (tid / WT) * 4;
    if (col >= w) return;
    WSU_STATIC_FOR(4, e, {
        double v = KIND == WSU_COST_WOW ? (1.0 / xi1[e] + 1.0 / xi2[e]) + 1.0 / xi3[e] : (xi1[e] + xi2[e]) + xi3[e];
        v = v <= clamp ? v : clamp;                            // inf / nan / > clamp -> clamp
        if (row0 + e < h) rho[((size_t)nn * h + row0 + e) * w + col] = v;
    });
}

}  // namespace

extern "C" int wsu_wavelet_cost_f64(const uint8_t* x_u8, double* rho, int kind, double sigma, double clamp, int n, int h, int w,
                                    void* stream) {
    WSU_REQUIRE(x_u8 && rho, "wavelet_cost_f64: null pointer");
    WSU_REQUIRE(kind == WSU_COST_SUNIWARD || kind == WSU_COST_WOW, "wavelet_cost_f64: kind=%d is neither WSU_COST_SUNIWARD nor WSU_COST_WOW", kind);
    WSU_REQUIRE(kind != WSU_COST_SUNIWARD || (sigma > 0.0 && sigma < __builtin_inf()), "wavelet_cost_f64: sigma=%g must be positive and finite", sigma);
    WSU_REQUIRE(clamp > 0.0 && clamp < __builtin_inf(), "wavelet_cost_f64: clamp=%g must be positive and finite", clamp);
    WSU_REQUIRE_SHAPE("wavelet_cost_f64", WSU_COUNTER_PIXELS, "counters");
    const int vec_in = (w % 16 == 0) && ((uintptr_t)x_u8 % 16 == 0);
    const dim3 grid((w + WT - 1) / WT, (h + WT - 1) / WT, n);
    if (kind == WSU_COST_WOW)
        hipLaunchKernelGGL(wavelet_cost_kernel<WSU_COST_WOW>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x_u8, rho, h, w, vec_in, sigma, clamp);
    else
        hipLaunchKernelGGL(wavelet_cost_kernel<WSU_COST_SUNIWARD>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x_u8, rho, h, w, vec_in, sigma, clamp);
    return wsu_check_launch("wavelet_cost_kernel");
}
