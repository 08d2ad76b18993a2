// K29: per-pixel sums of the WS residual terms ACROSS images (A. D. Ker, "Locating steganographic payload via WS residuals", ACM MM&Sec
// 2008).  Not part of the reference; the per-pixel terms are K11's (ws_pixel_terms, wsu_metric.h), only the direction of the sum differs.
//
//   Images embedded under one stego key carry their payload at the same pixels.  r = (s - s_bar)(s - s_hat) has expectation 1/2 at a
//   used pixel and 0 at an unused one, so the (weighted) mean of r over the images of a pixel separates the two.
//
//   per interior pixel and image, float32, numpy's operation sequence, nothing contracted:
//       wgt = 1 (weighted 0) | 1 / (5 + var) (weighted 1);   r = s * res;   t = wgt * r
//       where t is NaN: nothing is added, else
//       num += q(t),  q = llrint((double)min(max(t, -4096), 4096) * 2^24)  (ws_seq_term, K27's quantiser);   den += llrint((double)wgt * 2^32)
//
// Integer sums make the accumulators independent of the batch split, the image order and the launch shape.  Thread = interior pixel
// (row-major over the interior, so the accumulators are read and written as contiguous 8-byte words), images in a loop with the two
// sums in registers.  With parts = 1 a pixel has one owner, which adds its sums with a plain load and store; with parts > 1 the images are
// dealt round-robin to `parts` workgroups per pixel tile and the sums are added with 64-bit integer atomics (at most two per pixel and
// workgroup).  Measured (profiles/r24): the image loop is a serial chain of loads and arithmetic per thread, so one owner per pixel is bound
// by latency, not by the atomics it saves: at 512 x 512 (1 016 tiles, four waves per SIMD) it takes 1.26 - 1.57 x K11's time, four parts
// 1.02 - 1.14 x; at 64 x 64 (16 tiles) one owner takes 2.9 x the time of 16 parts.  parts = 0 therefore brings the grid to about WSL_FILL
// workgroups.  Traffic as K11's, 1 B + 4 B per pixel and image, plus 32 B of accumulator traffic per pixel and part.
#pragma clang fp contract(off)
#include "wsu_metric.h"

namespace {

constexpr int WSL_FILL = 4096;                           // automatic parts: as many as bring the grid to about this many workgroups (16 waves per SIMD)

// (loose parameters, the struct put together inside: as K27's rows kernel, ws_sequential.hip says why; with a WsSource argument and a local
// copy of the taps this kernel took two more SGPRs and measured 0.1-0.4 us slower than the bound allows, profiles/r35)
__global__ __launch_bounds__(256) void ws_residual_accumulate_kernel(
    const uint8_t* __restrict__ xu8, const float* __restrict__ xhat, Taps3x3<float> mean_taps, Taps3x3<float> pixel_taps,
    const float* __restrict__ image_filters, int use_pixel_filter, int hat_full, float hat_scale, int weighted, long long* __restrict__ num,
    long long* __restrict__ den, int n, int h, int w) {
    __shared__ float unit[256];                          // u / 255.f of every uint8 value (ws_unit_table)
    const WsSource src{xhat, nullptr, image_filters, mean_taps, pixel_taps, use_pixel_filter, hat_full, hat_scale, weighted, 0};
    const int tid = threadIdx.x;
    ws_unit_table(src, unit, tid);
    const int iw = w - 2;
    const long long m = (long long)(h - 2) * iw, i = (long long)blockIdx.x * 256 + tid;
    if (i >= m) return;
    const int r = (int)(i / iw) + 1, c = (int)(i % iw) + 1;
    long long a = 0, b = 0;
    for (int nn = blockIdx.y; nn < n; nn += gridDim.y) {
        if (image_filters) pixel_taps = ws_source_taps(src, nn);     // (src keeps the launch's taps; they are not read once there are per-image ones)
        const WsTerms p = ws_pixel_terms(xu8 + (size_t)nn * h * w, src, pixel_taps, unit, hat_base(hat_full, nn, h, w), r, c, w);
        const float rr = p.s * p.res;
        const float t = p.wgt * rr;
        if (t == t) {                                    // a NaN term adds to neither sum
            a += ws_seq_term(t);
            b += __builtin_llrint((double)p.wgt * 4294967296.0);
        }
    }
    if (gridDim.y == 1) {                                // (uniform over the grid) the pixel's only owner
        num[i] += a;
        den[i] += b;
    } else {
        if (a) atomicAdd(reinterpret_cast<unsigned long long*>(num + i), (unsigned long long)a);
        if (b) atomicAdd(reinterpret_cast<unsigned long long*>(den + i), (unsigned long long)b);
    }
}

}  // namespace

extern "C" {

int wsu_ws_residual_accumulate(const uint8_t* x_u8, const float* x_hat, const float* pixel_filter, const float* pixel_filters,
                               const float* mean_filter, int hat_full, float hat_scale, int weighted, int parts, long long* num, long long* den,
                               int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && num && den, "ws_residual_accumulate: null pointer");
    WsSource src;
    int rc = ws_source_make(src, "ws_residual_accumulate", "the residual means", false, x_hat, nullptr, pixel_filter, pixel_filters, mean_filter,
                            hat_full, hat_scale, weighted, 0, n, h, w, 31);
    if (rc) return rc;
    WSU_REQUIRE(parts >= 0 && parts <= 65535, "ws_residual_accumulate: parts=%d outside 0 (automatic) .. 65535", parts);
    WSU_REQUIRE((uintptr_t)num % 8 == 0 && (uintptr_t)den % 8 == 0, "ws_residual_accumulate: accumulators must be 8-byte aligned");
    const long long blocks = ((long long)(h - 2) * (w - 2) + 255) / 256;
    if (parts == 0) parts = (int)(blocks >= WSL_FILL ? 1 : WSL_FILL / blocks);
    if (parts > n) parts = n;
    hipLaunchKernelGGL(ws_residual_accumulate_kernel, dim3((unsigned)blocks, parts), dim3(256), 0, static_cast<hipStream_t>(stream), x_u8, src.xhat,
                       src.mean_taps, src.pixel_taps, src.image_filters, src.use_pixel_filter, src.hat_full, src.hat_scale, src.weighted, num, den,
                       n, h, w);
    return wsu_check_launch("ws_residual_accumulate_kernel");
}

}  // extern "C"
