// K11: the weighted-stego (WS) payload estimate of the caller of the predictor, src/ws/estimate.py:55-136 `attack`:
//
//   x      = cover/stego plane (uint8 values),   x_bar = x ^ 1,    interior = [1:-1, 1:-1]
//   x_hat  = pixel_estimator(x)                                       (:89)  UNet output*255, a host array, or a 3x3 filter
//   mu     = convolve(x,   mean_estimator, 'valid');  mu2 = convolve(x*x, mean_estimator, 'valid')          (:93-94)
//   var    = mu2 - mu^2;   weights = 1/(5+var) (weighted=1) | 5+var (weighted=-1) | 1 (weighted=0)          (:95-110)
//   weights /= sum(weights)
//   beta   = clip( sum(weights * (x - x_bar) * (x - x_hat)), 0, None )                                       (:118-121)
//   if correct_bias:  beta -= beta * sum(weights * (x - x_bar) * pixel_estimator(x_bar - x))                 (:126-128)
//
// Everything per pixel is float32 like the numpy original (separately rounded mul / sub, no contraction: wsu_metric.h); the three sums
// are fp64 in a fixed order (per-thread strided, LDS tree, 64 partial blocks per image, second tree), so a result is
// bitwise reproducible.  With the reference's default mean estimator (AVG, 8 taps of 1/8) mu, mu2 and var are exact in
// float32 for uint8 pixels, whatever the order of the nine products.
// HBM-bound: 1 B (pixel, neighbours hit L1/L2) + 4 B (prediction) [+ 4 B bias prediction] per pixel.  With an in-kernel filter the
// quotients x / 255. come from a 256-entry LDS table (one IEEE division per thread and workgroup; the same bits as dividing per pixel).
// No fused multiply-adds in this file: the WS estimator follows numpy's float32 operation sequence (src/ws/estimate.py:90-121), written
// with plain operators under contract(off) (hipcc's default -ffp-contract=fast would fuse them; see wsu_metric.h for the policy).
#pragma clang fp contract(off)
#include "wsu_metric.h"

namespace {

constexpr int WSA_PARTS = 64;                           // partial blocks per image
using Taps = Taps3x3<float>;
// true convolution, 'valid': out(r,c) = sum_{a,b} K[a][b] * v(r+1-a, c+1-b), summed in the order K00 .. K22
__device__ __forceinline__ float conv9(const Taps& t, const float v[3][3]) { return conv9_f32<true>(t, v); }

__global__ __launch_bounds__(256) void ws_attack_partial_kernel(const uint8_t* __restrict__ xu8, WsSource src, double* __restrict__ partial,
                                                                int h, int w) {
    __shared__ double red[3][256];
    __shared__ float unit[256];                          // u / 255.f of every uint8 value (ws_unit_table)
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const Taps taps = ws_source_taps(src, nn);
    ws_unit_table(src, unit, tid);
    const size_t hbase = hat_base(src.hat_full, nn, h, w);
    double sw = 0.0, sb = 0.0, sc = 0.0;
    for (int r = 1 + part; r <= h - 2; r += WSA_PARTS) {
        for (int c = 1 + tid; c <= w - 2; c += 256) {
            const WsTerms t = ws_pixel_terms(img, src, taps, unit, hbase, r, c, w);
            const float ws = t.wgt * t.s;
            sw += (double)t.wgt;
            sb += (double)(ws * t.res);
            sc += (double)(ws * t.bias);
        }
    }
    red[0][tid] = sw; red[1][tid] = sb; red[2][tid] = sc;
    block_sum<256>(tid, red[0], red[1], red[2]);
    if (tid < 3) partial[((size_t)nn * WSA_PARTS + part) * 3 + tid] = red[tid][0];
}

__global__ __launch_bounds__(64) void ws_attack_finish_kernel(const double* __restrict__ partial, float* __restrict__ beta_hat,
                                                              double* __restrict__ sums, int correct_bias) {
    __shared__ double red[3][WSA_PARTS];
    const int nn = blockIdx.x, tid = threadIdx.x;
    for (int k = 0; k < 3; ++k) red[k][tid] = partial[((size_t)nn * WSA_PARTS + tid) * 3 + k];
    block_sum<WSA_PARTS>(tid, red[0], red[1], red[2]);
    if (tid == 0) {
        const double sw = red[0][0], sb = red[1][0], sc = red[2][0];
        double beta = sb / sw;
        beta = beta < 0.0 ? 0.0 : beta;                                               // np.clip(beta_hat, 0, None): NaN stays NaN
        if (correct_bias) beta -= beta * (sc / sw);
        beta_hat[nn] = (float)beta;
        if (sums) { sums[nn * 3 + 0] = sw; sums[nn * 3 + 1] = sb; sums[nn * 3 + 2] = sc; }
    }
}

__global__ __launch_bounds__(256) void lsb_delta_unit_kernel(const uint8_t* __restrict__ x, float* __restrict__ y, size_t count) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const uint8_t u = x[i];
        y[i] = ((float)(uint8_t)(u ^ 1) - (float)u) / 255.0f;                          // (x_bar - x) / 255.
    }
}

// filters/evaluate.py:136-141 `infere_single`: convolve(x / 255., K, 'valid') * 255. on one fp32 plane
__global__ __launch_bounds__(256) void filter3x3_valid_kernel(const float* __restrict__ x, Taps taps, float* __restrict__ y,
                                                              int n, int h, int w) {
    const int ih = h - 2, iw = w - 2;
    const long long total = (long long)n * ih * iw;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % iw), r = (int)((i / iw) % ih), nn = (int)(i / ((long long)iw * ih));
        const float* p = x + ((size_t)nn * h + r) * w + c;
        float q[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) q[a][b] = p[(size_t)a * w + b] / 255.0f;
        y[i] = conv9(taps, q) * 255.0f;
    }
}

// the two launches behind wsu_ws_attack (one filter, or a prediction) and wsu_ws_attack_taps (one filter per image)
int ws_attack_launch(const uint8_t* x_u8, const WsSource& src, float* beta_hat, double* sums, void* workspace, int n, int h, int w, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(ws_attack_partial_kernel, dim3(WSA_PARTS, n), dim3(256), 0, s, x_u8, src, partial, h, w);
    int rc = wsu_check_launch("ws_attack_partial_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(ws_attack_finish_kernel, dim3(n), dim3(WSA_PARTS), 0, s, partial, beta_hat, sums, src.correct_bias);
    return wsu_check_launch("ws_attack_finish_kernel");
}
}  // namespace

extern "C" {

size_t wsu_ws_attack_workspace_bytes(int n) { return (size_t)n * WSA_PARTS * 3 * sizeof(double); }

int wsu_ws_attack(const uint8_t* x_u8, const float* x_hat, const float* x_bias, const float* pixel_filter, const float* mean_filter,
                  int hat_full, float hat_scale, int weighted, int correct_bias, float* beta_hat, double* sums,
                  void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && beta_hat && workspace, "ws_attack: null pointer");
    WsSource src;
    int rc = ws_source_make(src, "ws_attack", "the estimate", true, x_hat, x_bias, pixel_filter, nullptr, mean_filter, hat_full, hat_scale,
                            weighted, correct_bias, n, h, w, 0);                  // (no cap: K11 indexes with size_t and sums in fp64)
    if (rc) return rc;
    WSU_REQUIRE(workspace_bytes >= wsu_ws_attack_workspace_bytes(n), "ws_attack: workspace too small");
    return ws_attack_launch(x_u8, src, beta_hat, sums, workspace, n, h, w, stream);
}

int wsu_ws_attack_taps(const uint8_t* x_u8, const float* pixel_filters, const float* mean_filter, int weighted, int correct_bias,
                       float* beta_hat, double* sums, void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && pixel_filters && beta_hat && workspace, "ws_attack_taps: null pointer");
    WsSource src;
    int rc = ws_source_make(src, "ws_attack_taps", "the estimate", true, nullptr, nullptr, nullptr, pixel_filters, mean_filter, 1, 255.0f,
                            weighted, correct_bias, n, h, w, 0);
    if (rc) return rc;
    WSU_REQUIRE(workspace_bytes >= wsu_ws_attack_workspace_bytes(n), "ws_attack_taps: workspace too small");
    return ws_attack_launch(x_u8, src, beta_hat, sums, workspace, n, h, w, stream);
}

int wsu_filter3x3_valid_f32(const float* x, const float* filter, float* y, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x && filter && y, "filter3x3_valid: null pointer");
    WSU_REQUIRE(n > 0 && h >= 3 && w >= 3, "filter3x3_valid: bad shape n=%d h=%d w=%d", n, h, w);
    const Taps t = taps_from_kernel(filter);
    const long long total = (long long)n * (h - 2) * (w - 2);
    const long long nblk = (total + 255) / 256;
    hipLaunchKernelGGL(filter3x3_valid_kernel, dim3((unsigned)(nblk < 65536 ? nblk : 65536)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, t, y, n, h, w);
    return wsu_check_launch("filter3x3_valid_kernel");
}

int wsu_lsb_delta_unit_f32(const uint8_t* x, float* y, size_t count, void* stream) {
    WSU_REQUIRE(x && y, "lsb_delta_unit: null pointer");
    if (count == 0) return 0;
    const size_t nblk = (count + 255) / 256;
    hipLaunchKernelGGL(lsb_delta_unit_kernel, dim3((unsigned)(nblk < 65536 ? nblk : 65536)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, y, count);
    return wsu_check_launch("lsb_delta_unit_kernel");
}

}  // extern "C"
