// K12-K14: HILL-cost weighted prediction error (wMAE), src/filters/evaluate.py:79-115 `get_filter_residuals_cover` and
// src/predictor_error.py:19-76 `attack`:
//
//   R     = x (*) [[-1,2,-1],[2,-4,2],[-1,2,-1]]          S = box3x3(|R|)          rho0 = 9/S  (+inf where S == 0)
//   cost  = box15x15(rho0) / 225,  inf | nan | > 1e10 -> 1e10                       (every convolution 'same', boundary 'symm')
//   q     = numpy.quantile(cost[1:-1,1:-1], quantile)  ('linear')
//   mae   = mean |x - x_hat|,   wmae = mean |x - x_hat| over cost <= q              (interior [1:-1,1:-1])
//
// The three 'same'/'symm' convolutions equal three 'valid' ones on x padded once by 9 with numpy.pad(mode='symmetric'): the
// kernels are symmetric, so they commute with the reflection.  K12 therefore reads x through one periodic symmetric index fold.
// The box sums are direct fp32 sums (no running differences), so an infinity only ever meets additions.
//
// K13 finds q with an exact radix select over the fp32 bit patterns (positive and finite after the clamp, so monotone as uint32):
// three histogram passes of 11/11/10 bits give a = c_(k); one more pass gives count(c <= a) and min(c > a), hence b = c_(k+1).
// All cross-workgroup traffic is integer atomics, and results pass between kernels only at kernel boundaries: deterministic.
// K14 sums |x - x_hat| in fp64 in a fixed order (per-thread strided, LDS tree, 64 partial blocks per image, second tree).
// numpy's float32 / float64 operation sequences: plain operators, no fused multiply-adds (wsu_metric.h)
#pragma clang fp contract(off)
#include "wsu_metric.h"

namespace {

constexpr int HT = 64;                 // K12 output tile (HT x HT pixels per workgroup, 256 threads)
constexpr int HX = HT + 18;            // staged u8 window (pad 9 on each side)
constexpr int HXS = HT + 32;           // LDS row stride of the window; window column wc lives at wc + 7 (hill_stage_window)
constexpr int HR = HT + 16;            // |R| extent
constexpr int HS = HT + 14;            // S / rho0 extent

constexpr int RS_BINS = 2048;          // K13 radix: 11 / 11 / 10 bits
constexpr int RS_PARTS = 64;           // K13 / K14 workgroups per image
constexpr int PE_PARTS = 64;

__global__ __launch_bounds__(256) void hill_cost_kernel(const uint8_t* __restrict__ x, float* __restrict__ cost, int h, int w,
                                                        int vec_in, int vec_out, float clamp) {
    __shared__ __attribute__((aligned(16))) uint8_t xs[HX * HXS];
    __shared__ float rho[HS * HS];
    __shared__ __attribute__((aligned(16))) float hbuf[HS * HT];       // |R| (int16) first, then the horizontal 15-tap sums
    short* ar = reinterpret_cast<short*>(hbuf);
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * HT, r0 = blockIdx.y * HT, nn = blockIdx.z;
    const uint8_t* img = x + (size_t)nn * h * w;

    // ---- stage the (HT+18)^2 window: 16-byte row segments where the tile is well inside the image, else through the fold
    hill_stage_window<HT>(img, xs, r0, c0, h, w, vec_in, tid);
    __syncthreads();
    // ---- |R| (exact integers, |R| <= 16 * 255)
    for (int i = tid; i < HR * HR; i += 256) {
        const int a = i / HR, b = i % HR;
        const uint8_t* p = xs + a * HXS + b + 7;
        const int r = -(int)p[0] + 2 * (int)p[1] - (int)p[2]
                    + 2 * (int)p[HXS] - 4 * (int)p[HXS + 1] + 2 * (int)p[HXS + 2]
                    - (int)p[2 * HXS] + 2 * (int)p[2 * HXS + 1] - (int)p[2 * HXS + 2];
        ar[i] = (short)(r < 0 ? -r : r);
    }
    __syncthreads();
    // ---- S = box3x3(|R|) (exact), rho0 = 1 / (S/9)
    for (int i = tid; i < HS * HS; i += 256) {
        const int a = i / HS, b = i % HS;
        int s = 0;
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) s += ar[(a + u) * HR + b + v];
        rho[i] = s > 0 ? 9.0f / (float)s : __builtin_inff();
    }
    __syncthreads();
    // ---- horizontal 15-tap direct sums (rows of rho, HT output columns)
    for (int i = tid; i < HS * HT; i += 256) {
        const int a = i / HT, b = i % HT;
        const float* p = rho + a * HS + b;
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 15; ++t) s += p[t];
        hbuf[i] = s;
    }
    __syncthreads();
    // ---- vertical 15-tap direct sums, /225, clamp; four consecutive columns per thread -> one 16-byte store
    const float inv225 = 1.0f / 225.0f;
    for (int i = tid; i < HT * (HT / 4); i += 256) {
        const int a = i / (HT / 4), b = (i % (HT / 4)) * 4;
        f32x4 s = mk_f4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < 15; ++t) s += *reinterpret_cast<const f32x4*>(hbuf + (a + t) * HT + b);
        s *= inv225;
        s.x = s.x <= clamp ? s.x : clamp;          // inf / nan / > clamp -> clamp
        s.y = s.y <= clamp ? s.y : clamp;
        s.z = s.z <= clamp ? s.z : clamp;
        s.w = s.w <= clamp ? s.w : clamp;
        const int r = r0 + a, c = c0 + b;
        if (r >= h) continue;
        float* o = cost + ((size_t)nn * h + r) * w + c;
        if (vec_out && c + 4 <= w) {
            *reinterpret_cast<f32x4*>(o) = s;
        } else {
            if (c < w) o[0] = s.x;
            if (c + 1 < w) o[1] = s.y;
            if (c + 2 < w) o[2] = s.z;
            if (c + 3 < w) o[3] = s.w;
        }
    }
}

// ---- K13 ------------------------------------------------------------------------------------------------------------------
// Workspace (uint32): hist[3][n][RS_BINS], then state[n][4] = {prefix bits, remaining rank, count(c <= a), ~min(c > a) bits}.
__global__ __launch_bounds__(256) void hill_select_hist_kernel(const float* __restrict__ cost, uint32_t* __restrict__ ws, int pass,
                                                               int n, int h, int w) {
    __shared__ uint32_t lh[RS_BINS];
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const RadixDigit ps = radix_digit(pass);
    uint32_t* hist = ws + ((size_t)pass * n + nn) * RS_BINS;
    const uint32_t prefix = pass == 0 ? 0u : ws[(size_t)3 * n * RS_BINS + nn * 4 + 0];
    for (int b = tid; b < RS_BINS; b += 256) lh[b] = 0u;
    __syncthreads();
    const float* img = cost + (size_t)nn * h * w;
    for (int r = 1 + part; r <= h - 2; r += RS_PARTS)
        for (int c = 1 + tid; c <= w - 2; c += 256) {
            const uint32_t u = __float_as_uint(img[(size_t)r * w + c]);
            if ((u & ps.mask) == prefix) atomicAdd(&lh[(u >> ps.shift) & (ps.bins - 1)], 1u);
        }
    __syncthreads();
    for (int b = tid; b < ps.bins; b += 256)
        if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

// one workgroup per image: the bin that holds the remaining rank, by a fixed-order scan of the histogram
__global__ __launch_bounds__(256) void hill_select_pick_kernel(uint32_t* __restrict__ ws, int pass, long long k, int n) {
    __shared__ uint32_t part[256];
    const int nn = blockIdx.x, tid = threadIdx.x;
    uint32_t* st = ws + (size_t)3 * n * RS_BINS + nn * 4;
    radix_pick<uint32_t>(ws + ((size_t)pass * n + nn) * RS_BINS, st, pass == 0 ? (uint32_t)k : st[1], pass, part, tid);
}

// count(c <= a) and min(c > a) for a = c_(k) (stored as the maximum of the complemented bit pattern, so zero is the identity)
__global__ __launch_bounds__(256) void hill_select_next_kernel(const float* __restrict__ cost, uint32_t* __restrict__ ws, int n, int h, int w) {
    __shared__ uint32_t red_c[256], red_m[256];
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    uint32_t* st = ws + (size_t)3 * n * RS_BINS + nn * 4;
    const uint32_t a = st[0];
    const float* img = cost + (size_t)nn * h * w;
    uint32_t cnt = 0, mx = 0;
    for (int r = 1 + part; r <= h - 2; r += RS_PARTS)
        for (int c = 1 + tid; c <= w - 2; c += 256) {
            const uint32_t u = __float_as_uint(img[(size_t)r * w + c]);
            if (u <= a) ++cnt;
            else mx = max(mx, ~u);
        }
    red_c[tid] = cnt; red_m[tid] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { red_c[tid] += red_c[tid + s]; red_m[tid] = max(red_m[tid], red_m[tid + s]); }
        __syncthreads();
    }
    if (tid == 0) {
        if (red_c[0]) atomicAdd(&st[2], red_c[0]);
        if (red_m[0]) atomicMax(&st[3], red_m[0]);
    }
}

// numpy's linear quantile: q = a + (b-a)*g, or b - (b-a)*(1-g) when g >= 0.5 (numpy _lerp), in float64
__global__ __launch_bounds__(64) void hill_select_finish_kernel(const uint32_t* __restrict__ ws, long long k, double g, long long count,
                                                                double* __restrict__ q, int n) {
    const int nn = blockIdx.x * 64 + threadIdx.x;
    if (nn >= n) return;
    const uint32_t* st = ws + (size_t)3 * n * RS_BINS + nn * 4;
    const double a = (double)__uint_as_float(st[0]);
    const double b = (double)__uint_as_float(radix_next_bits(st[0], k, count, (long long)st[2], st[3]));
    const double d = b - a;
    q[nn] = g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

// ---- K14 ------------------------------------------------------------------------------------------------------------------
using DTaps = Taps3x3<double>;

__global__ __launch_bounds__(256) void pred_err_partial_kernel(
    const uint8_t* __restrict__ xu8, const float* __restrict__ xhat, int hat_full, float hat_scale, int use_filter, DTaps taps,
    const float* __restrict__ cost, const double* __restrict__ q, double* __restrict__ partial, int h, int w) {
    __shared__ double red[3][256];
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const float* cimg = cost + (size_t)nn * h * w;
    const size_t hbase = hat_base(hat_full, nn, h, w);
    const double qq = q[nn];
    double sa = 0.0, ss = 0.0, sn = 0.0;
    for (int r = 1 + part; r <= h - 2; r += PE_PARTS) {
        for (int c = 1 + tid; c <= w - 2; c += 256) {
            double ad;
            if (use_filter) {
                // get_filter_residuals: y - x @ filter, float64 (filters/evaluate.py:53-76), taps in the fixed order x00 .. x22
                ad = fabs((double)img[(size_t)r * w + c] - filter_hat64<false>(taps, img, r, c, w));
            } else {
                // K10's float32 residual: the same two roundings per pixel, so K14 and K10 sum the same float32 terms
                ad = (double)fabsf(residual_f32((float)img[(size_t)r * w + c], xhat[hat_index(hat_full, hbase, r, c, w)], hat_scale));
            }
            sa += ad;
            if ((double)cimg[(size_t)r * w + c] <= qq) { ss += ad; sn += 1.0; }
        }
    }
    red[0][tid] = sa; red[1][tid] = ss; red[2][tid] = sn;
    block_sum<256>(tid, red[0], red[1], red[2]);
    if (tid < 3) partial[((size_t)nn * PE_PARTS + part) * 3 + tid] = red[tid][0];
}

__global__ __launch_bounds__(64) void pred_err_finish_kernel(const double* __restrict__ partial, double* __restrict__ mae,
                                                             double* __restrict__ wmae, long long* __restrict__ selected, double count) {
    __shared__ double red[3][PE_PARTS];
    const int nn = blockIdx.x, tid = threadIdx.x;
    for (int k = 0; k < 3; ++k) red[k][tid] = partial[((size_t)nn * PE_PARTS + tid) * 3 + k];
    block_sum<PE_PARTS>(tid, red[0], red[1], red[2]);
    if (tid == 0) {
        mae[nn] = red[0][0] / count;
        wmae[nn] = red[1][0] / red[2][0];
        if (selected) selected[nn] = (long long)red[2][0];
    }
}

}  // namespace

extern "C" {

int wsu_hill_cost(const uint8_t* x_u8, float* cost, float clamp, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && cost, "hill_cost: null pointer");
    WSU_REQUIRE(n > 0 && n <= 65535 && h >= 3 && w >= 3, "hill_cost: bad shape n=%d h=%d w=%d", n, h, w);
    WSU_REQUIRE(clamp > 0.f && clamp < __builtin_inff(), "hill_cost: clamp=%g must be positive and finite", (double)clamp);
    const int vec_in = (w % 16 == 0) && ((uintptr_t)x_u8 % 16 == 0);
    const int vec_out = (w % 4 == 0) && ((uintptr_t)cost % 16 == 0);
    hipLaunchKernelGGL(hill_cost_kernel, dim3((w + HT - 1) / HT, (h + HT - 1) / HT, n), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_u8, cost, h, w, vec_in, vec_out, clamp);
    return wsu_check_launch("hill_cost_kernel");
}

size_t wsu_hill_threshold_workspace_bytes(int n) { return (size_t)n * (3 * RS_BINS + 4) * sizeof(uint32_t); }

int wsu_hill_threshold(const float* cost, long long k, double g, double* q, void* workspace, size_t workspace_bytes,
                       int n, int h, int w, void* stream) {
    WSU_REQUIRE(cost && q && workspace, "hill_threshold: null pointer");
    WSU_REQUIRE(n > 0 && n <= 65535 && h >= 3 && w >= 3, "hill_threshold: bad shape n=%d h=%d w=%d", n, h, w);
    const long long count = (long long)(h - 2) * (w - 2);
    WSU_REQUIRE(count < (1LL << 32), "hill_threshold: %lld interior pixels exceed the 32-bit counters", count);
    WSU_REQUIRE(k >= 0 && k < count, "hill_threshold: rank k=%lld outside [0, %lld)", k, count);
    WSU_REQUIRE(g >= 0.0 && g < 1.0, "hill_threshold: fraction g=%g outside [0, 1)", g);
    WSU_REQUIRE(workspace_bytes >= wsu_hill_threshold_workspace_bytes(n), "hill_threshold: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* ws = static_cast<uint32_t*>(workspace);
    if (hipMemsetAsync(ws, 0, wsu_hill_threshold_workspace_bytes(n), s) != hipSuccess) return wsu_check_launch("hill_threshold memset");
    for (int p = 0; p < 3; ++p) {
        hipLaunchKernelGGL(hill_select_hist_kernel, dim3(RS_PARTS, n), dim3(256), 0, s, cost, ws, p, n, h, w);
        int rc = wsu_check_launch("hill_select_hist_kernel");
        if (rc) return rc;
        hipLaunchKernelGGL(hill_select_pick_kernel, dim3(n), dim3(256), 0, s, ws, p, k, n);
        rc = wsu_check_launch("hill_select_pick_kernel");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(hill_select_next_kernel, dim3(RS_PARTS, n), dim3(256), 0, s, cost, ws, n, h, w);
    int rc = wsu_check_launch("hill_select_next_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(hill_select_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, s, ws, k, g, count, q, n);
    return wsu_check_launch("hill_select_finish_kernel");
}

size_t wsu_prediction_error_workspace_bytes(int n) { return (size_t)n * PE_PARTS * 3 * sizeof(double); }

int wsu_prediction_error(const uint8_t* x_u8, const float* x_hat, const double* pixel_filter, int hat_full, float hat_scale,
                         const float* cost, const double* q, double* mae, double* wmae, long long* selected,
                         void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && cost && q && mae && wmae && workspace, "prediction_error: null pointer");
    WSU_REQUIRE((x_hat != nullptr) != (pixel_filter != nullptr), "prediction_error: give exactly one of x_hat / pixel_filter");
    WSU_REQUIRE(n > 0 && n <= 65535 && h >= 3 && w >= 3, "prediction_error: bad shape n=%d h=%d w=%d", n, h, w);
    WSU_REQUIRE(workspace_bytes >= wsu_prediction_error_workspace_bytes(n), "prediction_error: workspace too small");
    const DTaps t = taps_from_weights(pixel_filter);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(pred_err_partial_kernel, dim3(PE_PARTS, n), dim3(256), 0, s, x_u8, x_hat, hat_full ? 1 : 0, hat_scale,
                       pixel_filter ? 1 : 0, t, cost, q, partial, h, w);
    int rc = wsu_check_launch("pred_err_partial_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(pred_err_finish_kernel, dim3(n), dim3(PE_PARTS), 0, s, partial, mae, wmae, selected,
                       (double)((long long)(h - 2) * (w - 2)));
    return wsu_check_launch("pred_err_finish_kernel");
}

}  // extern "C"
