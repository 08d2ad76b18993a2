// K15: correlation between a predictor's cover estimate made from the stego image and the embedding change,
// src/correlation.py:22-59 `run`:
//
//   d    = (x_s - x_c)[1:-1, 1:-1]        xhat = predictor(x_s)  (H-2, W-2)        dhat = xhat - x_c[1:-1, 1:-1]
//   cov  = sum((dhat - mean dhat) * (d - mean d)) / (n - 1)                          n = (H-2)(W-2)
//   cor  = cov / std(xhat) / std(d)                                                  std: ddof 0; NB xhat, not dhat
//
// Two passes, as numpy computes it: pass 1 gives the means (exact integer sums of d and x_c, an fp64 sum of xhat; mean dhat =
// mean xhat - mean x_c), pass 2 the centred fp64 sums S_hd, S_hh, S_dd.  A one-pass raw-moment form would subtract two sums of
// squares of ~128^2 * n to get a spread of ~1e-3 grey levels, and lose it.  Every sum is fixed-order (per-thread strided, LDS
// tree, 64 row blocks per image, then a sequential sum over the blocks), with no float atomics, so a pair's result does not
// depend on the batch it is in.  Division by zero follows IEEE: x_s == x_c gives 0/0 = NaN, a constant prediction +-inf.
// Memory-bound: 2 B (+ 4 B with x_hat) per pixel and pass; the second pass re-reads what the first one just brought to L2.
// numpy's float64 operation sequence: separately rounded products and sums, plain operators (wsu_metric.h)
#pragma clang fp contract(off)
#include "wsu_metric.h"

namespace {

constexpr int PC_PARTS = 64;            // row blocks (workgroups) per image
constexpr int PC_THREADS = 256;

using CTaps = Taps3x3<double>;

// pass-1 partials per (image, block): {sum d, sum x_c} as int64, {sum xhat} as fp64; pass-2 partials: {S_hd, S_hh, S_dd} fp64
struct PcWs {
    long long* isum;                    // [n][PC_PARTS][2]
    double* hsum;                       // [n][PC_PARTS]
    double* csum;                       // [n][PC_PARTS][3]
};

__device__ __forceinline__ PcWs pc_ws(void* ws, int n) {
    PcWs p;
    p.isum = static_cast<long long*>(ws);
    p.hsum = reinterpret_cast<double*>(p.isum + (size_t)n * PC_PARTS * 2);
    p.csum = p.hsum + (size_t)n * PC_PARTS;
    return p;
}

// the prediction at interior pixel (r, c), r in 1..h-2, c in 1..w-2, widened to fp64
__device__ __forceinline__ double pc_hat(const uint8_t* __restrict__ s, const float* __restrict__ xhat, size_t hbase, int use_filter,
                                         const CTaps& t, int hat_full, float hat_scale, int r, int c, int w) {
    // scipy.signal.convolve(x, K, 'valid'): a true convolution, sum_ab K[a][b] * x[r+1-a][c+1-b], taps in the order K00 .. K22
    if (use_filter) return filter_hat64<true>(t, s, r, c, w);
    return (double)(xhat[hat_index(hat_full, hbase, r, c, w)] * hat_scale);         // K10's float32 xhat = y * 255, then widened
}

// The three means of image nn from its pass-1 partials.  Called by a whole workgroup of >= PC_PARTS threads: the partials are loaded
// in parallel into LDS, then summed by thread 0 in block order (every caller gets the same bits).  Result in means[0..2] =
// {mean d, mean x_c, mean xhat}, valid after the call's final barrier.
__device__ __forceinline__ void pc_means(const PcWs& p, int nn, double count, int tid, long long (*li)[PC_PARTS], double* lh,
                                         double* means) {
    if (tid < PC_PARTS) {
        li[0][tid] = p.isum[((size_t)nn * PC_PARTS + tid) * 2 + 0];
        li[1][tid] = p.isum[((size_t)nn * PC_PARTS + tid) * 2 + 1];
        lh[tid] = p.hsum[(size_t)nn * PC_PARTS + tid];
    }
    __syncthreads();
    if (tid == 0) {
        long long sd = 0, sc = 0;
        double sh = 0.0;
        for (int k = 0; k < PC_PARTS; ++k) { sd += li[0][k]; sc += li[1][k]; sh += lh[k]; }
        means[0] = (double)sd / count;                   // |sums| < 2^53: exact before the division
        means[1] = (double)sc / count;
        means[2] = sh / count;
    }
    __syncthreads();
}

__global__ __launch_bounds__(PC_THREADS) void pair_corr_mean_kernel(
    const uint8_t* __restrict__ xc, const uint8_t* __restrict__ xs, const float* __restrict__ xhat, int use_filter, CTaps taps,
    int hat_full, float hat_scale, void* __restrict__ workspace, int n, int h, int w) {
    __shared__ long long ired[2][PC_THREADS];
    __shared__ double hred[PC_THREADS];
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const uint8_t* c_img = xc + (size_t)nn * h * w;
    const uint8_t* s_img = xs + (size_t)nn * h * w;
    const size_t hbase = hat_base(hat_full, nn, h, w);
    long long sd = 0, sc = 0;
    double sh = 0.0;
    for (int r = 1 + part; r <= h - 2; r += PC_PARTS) {
        for (int c = 1 + tid; c <= w - 2; c += PC_THREADS) {
            const int vc = c_img[(size_t)r * w + c], vs = s_img[(size_t)r * w + c];
            sd += vs - vc;
            sc += vc;
            sh += pc_hat(s_img, xhat, hbase, use_filter, taps, hat_full, hat_scale, r, c, w);
        }
    }
    ired[0][tid] = sd; ired[1][tid] = sc; hred[tid] = sh;
    block_sum<PC_THREADS>(tid, ired[0], ired[1], hred);
    if (tid == 0) {
        const PcWs p = pc_ws(workspace, n);
        p.isum[((size_t)nn * PC_PARTS + part) * 2 + 0] = ired[0][0];
        p.isum[((size_t)nn * PC_PARTS + part) * 2 + 1] = ired[1][0];
        p.hsum[(size_t)nn * PC_PARTS + part] = hred[0];
    }
}

__global__ __launch_bounds__(PC_THREADS) void pair_corr_centred_kernel(
    const uint8_t* __restrict__ xc, const uint8_t* __restrict__ xs, const float* __restrict__ xhat, int use_filter, CTaps taps,
    int hat_full, float hat_scale, void* __restrict__ workspace, int n, int h, int w) {
    __shared__ double red[3][PC_THREADS];
    __shared__ long long li[2][PC_PARTS];
    __shared__ double lh[PC_PARTS], means[3];
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const PcWs p = pc_ws(workspace, n);
    pc_means(p, nn, (double)((long long)(h - 2) * (w - 2)), tid, li, lh, means);
    const double m_d = means[0], m_h = means[2], m_dh = means[2] - means[1];      // mean d, mean xhat, mean dhat
    const uint8_t* c_img = xc + (size_t)nn * h * w;
    const uint8_t* s_img = xs + (size_t)nn * h * w;
    const size_t hbase = hat_base(hat_full, nn, h, w);
    double s_hd = 0.0, s_hh = 0.0, s_dd = 0.0;
    for (int r = 1 + part; r <= h - 2; r += PC_PARTS) {
        for (int c = 1 + tid; c <= w - 2; c += PC_THREADS) {
            const int vc = c_img[(size_t)r * w + c], vs = s_img[(size_t)r * w + c];
            const double hat = pc_hat(s_img, xhat, hbase, use_filter, taps, hat_full, hat_scale, r, c, w);
            const double dd = (double)(vs - vc) - m_d;
            const double hh = hat - m_h;
            const double dh = (hat - (double)vc) - m_dh;
            s_hd += dh * dd;
            s_hh += hh * hh;
            s_dd += dd * dd;
        }
    }
    red[0][tid] = s_hd; red[1][tid] = s_hh; red[2][tid] = s_dd;
    block_sum<PC_THREADS>(tid, red[0], red[1], red[2]);
    if (tid < 3) p.csum[((size_t)nn * PC_PARTS + part) * 3 + tid] = red[tid][0];
}

// one workgroup per image: the block sums in block order (thread 0), then cov / sqrt(S_hh/n) / sqrt(S_dd/n), divided in numpy's order
__global__ __launch_bounds__(PC_PARTS) void pair_corr_finish_kernel(void* __restrict__ workspace, double* __restrict__ cor,
                                                                    double* __restrict__ moments, int n, int h, int w) {
    __shared__ long long li[2][PC_PARTS];
    __shared__ double lh[PC_PARTS], means[3], lc[3][PC_PARTS];
    const int nn = blockIdx.x, tid = threadIdx.x;
    const PcWs p = pc_ws(workspace, n);
    const double count = (double)((long long)(h - 2) * (w - 2));
    for (int j = 0; j < 3; ++j) lc[j][tid] = p.csum[((size_t)nn * PC_PARTS + tid) * 3 + j];
    pc_means(p, nn, count, tid, li, lh, means);          // (its barriers also publish lc)
    if (tid != 0) return;
    double s_hd = 0.0, s_hh = 0.0, s_dd = 0.0;
    for (int k = 0; k < PC_PARTS; ++k) { s_hd += lc[0][k]; s_hh += lc[1][k]; s_dd += lc[2][k]; }
    const double cov = s_hd / (count - 1.0);
    cor[nn] = cov / sqrt(s_hh / count) / sqrt(s_dd / count);
    if (moments) {
        double* m = moments + (size_t)nn * 6;
        m[0] = means[2]; m[1] = means[2] - means[1]; m[2] = means[0]; m[3] = s_hd; m[4] = s_hh; m[5] = s_dd;
    }
}

}  // namespace

extern "C" {

size_t wsu_pair_correlation_workspace_bytes(int n) {
    return n > 0 ? (size_t)n * PC_PARTS * (2 * sizeof(long long) + sizeof(double) + 3 * sizeof(double)) : 0;
}

int wsu_pair_correlation(const uint8_t* xc_u8, const uint8_t* xs_u8, const float* x_hat, const double* pixel_filter, int hat_full,
                         float hat_scale, double* cor, double* moments, void* workspace, size_t workspace_bytes,
                         int n, int h, int w, void* stream) {
    WSU_REQUIRE(xc_u8 && xs_u8 && cor && workspace, "pair_correlation: null pointer");
    WSU_REQUIRE((x_hat != nullptr) != (pixel_filter != nullptr), "pair_correlation: give exactly one of x_hat / pixel_filter");
    WSU_REQUIRE(hat_full == 0 || hat_full == 1, "pair_correlation: hat_full=%d must be 0 or 1", hat_full);
    WSU_REQUIRE(n > 0 && n <= 65535 && h >= 3 && w >= 3, "pair_correlation: bad shape n=%d h=%d w=%d", n, h, w);
    WSU_REQUIRE((long long)h * w <= (1LL << 40), "pair_correlation: %d x %d pixels exceed the exact integer sums", h, w);
    WSU_REQUIRE(workspace_bytes >= wsu_pair_correlation_workspace_bytes(n), "pair_correlation: workspace too small (%zu < %zu bytes)",
                workspace_bytes, wsu_pair_correlation_workspace_bytes(n));
    const CTaps t = taps_from_kernel(pixel_filter);
    const int use_filter = pixel_filter ? 1 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pair_corr_mean_kernel, dim3(PC_PARTS, n), dim3(PC_THREADS), 0, s, xc_u8, xs_u8, x_hat, use_filter, t, hat_full,
                       hat_scale, workspace, n, h, w);
    int rc = wsu_check_launch("pair_corr_mean_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(pair_corr_centred_kernel, dim3(PC_PARTS, n), dim3(PC_THREADS), 0, s, xc_u8, xs_u8, x_hat, use_filter, t, hat_full,
                       hat_scale, workspace, n, h, w);
    rc = wsu_check_launch("pair_corr_centred_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(pair_corr_finish_kernel, dim3(n), dim3(PC_PARTS), 0, s, workspace, cor, moments, n, h, w);
    return wsu_check_launch("pair_corr_finish_kernel");
}

}  // extern "C"
