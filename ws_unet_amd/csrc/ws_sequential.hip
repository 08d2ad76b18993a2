// K27: the WS changepoint for sequentially placed payloads (Ker, "A weighted stego image detector for sequential LSB replacement",
// SPIE 2007).  Not part of the reference; the per-pixel terms are K11's (ws_pixel_terms, wsu_metric.h), only the reduction differs.
//
//   A message written into the first k pixels of a path changes only those.  With the cover estimate (x + x_bar) / 2 for a used pixel
//   and x for an unused one, the weighted squared error against the prediction x_hat is a constant minus
//
//       T(k) = sum_{i <= k} w_i * (r_i - 1/4),     r_i = (x_i - x_bar_i) * (x_i - x_hat_i),     T(0) = 0,
//
//   and the estimate is the k that maximises T.  The path visits the INTERIOR pixels row by row, left to right within a row, rows from
//   the top (order 0) or from the bottom (order 1); M = (H-2)(W-2) positions.
//
//   per pixel, float32, numpy's operation sequence, nothing contracted:
//       wgt = 1 (weighted 0) | 1 / (5 + var) (weighted 1);   r = s * res;   d = r - 0.25f;   t = wgt * d
//       q   = 0 where t is NaN, else llrint((double)min(max(t, -4096), 4096) * 2^24)          (int64, round to nearest even)
//   per image, int64:
//       k = the smallest k in 0..M with T(k) = sum_{i <= k} q_i maximal (k = 0, T = 0, takes part);  t_max = T(k);  t_all = T(M);
//       curve[p] = T at the end of the p-th interior row of the path (optional).
//
// Integer terms make the reduction exact, so the result depends on neither the split of the work nor the batch; |q| <= 2^36 and
// M <= 2^27 keep every sum inside int64.  The maximum-prefix triple (sum, best, arg) of a run of terms combines associatively:
//   (a ++ b).sum = a.sum + b.sum;   (a ++ b).best, arg = a.best, a.arg if a.best >= a.sum + b.best (the earlier position wins a tie),
//   else a.sum + b.best, b.arg -- with arg counted from the start of the whole run, so nothing is shifted.  A single term is
//   (q, max(q, 0), position + (q > 0)); a term past the row's end is 0, which never wins on the right because best >= sum.
// Kernel 1: one WAVE per interior row (4 rows per workgroup, 64 workgroups per image striding the rows), 512 consecutive pixels per step:
//   ws_fold_step (wsu_metric.h: coalesced loads, the wave's own LDS strip, eight consecutive terms per lane, one ordered shuffle tree; why it
//   needs fences and no workgroup barrier stands there); the steps are folded left to right in lane 0 -> one triple per row (arg relative to
//   the row).  The only workgroup barrier is the one behind the LDS quotient table.  Kernel 2: one workgroup per image: thread t folds a
//   contiguous run of rows of the path (read backwards for order 1), an ordered tree over the 256 threads finishes (mp_block_finish); the
//   curve is the rows' inclusive prefix sum.
// Traffic as K11's: 1 B (pixel; the neighbours hit L1 / L2) + 4 B (prediction) per pixel, plus 24 B per row of workspace.  On 512 x 512
// planes both kernels are bound by the per-pixel arithmetic, not by HBM; this one takes 1.2-1.4 x K11's time (profiles/r23).
#pragma clang fp contract(off)
#include "wsu_metric.h"

namespace {

constexpr int WSS_PARTS = 64;                           // kernel 1: workgroups per image, four rows (waves) each per pass

// Loose parameters and the per-image taps written over `pixel_taps` (K27, K29, K33's terms): with a WsSource ARGUMENT the kernel loaded more
// of its arguments before the first branch and every stage measured 0.15-0.2 us slower, one outside the bound (profiles/r35).  The struct is
// put together here instead, so the shared functions serve the kernel all the same, and the device code is the one it had.
__global__ __launch_bounds__(256) void ws_sequential_rows_kernel(
    const uint8_t* __restrict__ xu8, const float* __restrict__ xhat, Taps3x3<float> mean_taps, Taps3x3<float> pixel_taps,
    const float* __restrict__ image_filters, int use_pixel_filter, int hat_full, float hat_scale, int weighted, long long* __restrict__ rows, int h,
    int w) {
    __shared__ float unit[256];                          // u / 255.f of every uint8 value (ws_unit_table)
    __shared__ long long strip[4][WS_FOLD_STRIP];        // per wave: the step's terms
    const WsSource src{xhat, nullptr, image_filters, mean_taps, pixel_taps, use_pixel_filter, hat_full, hat_scale, weighted, 0};
    const int nn = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    if (image_filters) pixel_taps = ws_source_taps(src, nn);                             // (uniform: nn = blockIdx.y)
    ws_unit_table(src, unit, tid);
    const size_t hbase = hat_base(src.hat_full, nn, h, w);
    const int ih = h - 2, iw = w - 2;
    long long* st = strip[wave];
    for (int r = 1 + (int)blockIdx.x * 4 + wave; r <= ih; r += WSS_PARTS * 4) {          // (uniform over the wave)
        MaxPrefix<int> run{0, 0, 0};                                                     // (lane 0's is the row's)
        for (int c0 = 0; c0 < iw; c0 += WS_FOLD_STEP) {
            for (int j = 0; j < WS_FOLD_PER; ++j) {
                const int at = 64 * j + lane, i = c0 + at;
                long long q = 0;                                                         // past the row's end: 0, which never wins on the right
                if (i < iw) {
                    const WsTerms p = ws_pixel_terms(img, src, pixel_taps, unit, hbase, r, i + 1, w);
                    const float rr = p.s * p.res;
                    const float d = rr - 0.25f;
                    const float t = p.wgt * d;
                    q = ws_seq_term(t);
                }
                st[at + at / WS_FOLD_PER] = q;
            }
            // ws_fold_step's text, kept here: as a call of it this kernel takes 81 VGPRs instead of 67 and drops from 7 to 5 waves per SIMD
            // (profiles/r35); the statements are the same and tests/test_gpu_ws_source.py pins that K33, which calls it, agrees.  An edit to
            // ws_fold_step is made here as well.
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int first = c0 + lane * WS_FOLD_PER;
            MaxPrefix<int> e{0, 0, first};
#pragma unroll
            for (int j = 0; j < WS_FOLD_PER; ++j) {
                e.sum += st[lane * WS_FOLD_PITCH + j];
                if (e.sum > e.best) { e.best = e.sum; e.arg = first + j + 1; }           // >: among equal maxima the first
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                       // (the next step's writes stay behind these reads)
            __builtin_amdgcn_wave_barrier();
            run = mp_combine(run, mp_wave(e));
        }
        if (lane == 0) mp_store(rows + ((size_t)nn * ih + (r - 1)) * 3, run);
    }
}

__global__ __launch_bounds__(256) void ws_sequential_finish_kernel(const long long* __restrict__ rows, long long* __restrict__ k,
                                                                   long long* __restrict__ t_max, long long* __restrict__ t_all,
                                                                   long long* __restrict__ curve, int ih, int iw, int order) {
    __shared__ long long seg[256];
    const int nn = blockIdx.x, tid = threadIdx.x;
    const long long* img = rows + (size_t)nn * ih * 3;
    const int per = (ih + 255) / 256;                    // path rows per thread, contiguous
    const long long p0 = (long long)tid * per;
    const long long p1 = p0 + per < ih ? p0 + per : ih;
    MaxPrefix<long long> run{0, 0, p0 * iw};
    for (long long p = p0; p < p1; ++p) {
        run = mp_combine(run, mp_load(img + (order ? ih - 1 - p : p) * 3, p * iw));
    }
    if (curve) {                                         // (uniform over the grid)
        seg[tid] = run.sum;
        __syncthreads();
        long long acc = 0;                               // exclusive prefix of this thread's run (at most 255 adds)
        for (int t = 0; t < tid; ++t) acc += seg[t];
        for (long long p = p0; p < p1; ++p) {
            acc += img[(order ? ih - 1 - p : p) * 3];
            curve[(size_t)nn * ih + p] = acc;
        }
    }
    mp_block_finish(run, tid, nn, k, t_max, t_all);
}

}  // namespace

extern "C" {

size_t wsu_ws_sequential_workspace_bytes(int n, int h) { return n > 0 && h >= 3 ? (size_t)n * (h - 2) * 3 * sizeof(long long) : 0; }

int wsu_ws_sequential(const uint8_t* x_u8, const float* x_hat, const float* pixel_filter, const float* pixel_filters, const float* mean_filter,
                      int hat_full, float hat_scale, int weighted, int order, long long* k, long long* t_max, long long* t_all,
                      long long* curve, void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && k && t_max && t_all && workspace, "ws_sequential: null pointer");
    WsSource src;
    int rc = ws_source_make(src, "ws_sequential", "the sequential statistic", false, x_hat, nullptr, pixel_filter, pixel_filters, mean_filter,
                            hat_full, hat_scale, weighted, 0, n, h, w, 27);
    if (rc) return rc;
    WSU_REQUIRE(order == 0 || order == 1, "ws_sequential: order=%d outside {0 = rows from the top, 1 = rows from the bottom}", order);
    WSU_REQUIRE(workspace_bytes >= wsu_ws_sequential_workspace_bytes(n, h), "ws_sequential: workspace too small");
    WSU_REQUIRE((uintptr_t)workspace % 8 == 0, "ws_sequential: workspace must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ws_sequential_rows_kernel, dim3(WSS_PARTS, n), dim3(256), 0, s, x_u8, src.xhat, src.mean_taps, src.pixel_taps,
                       src.image_filters, src.use_pixel_filter, src.hat_full, src.hat_scale, src.weighted, static_cast<long long*>(workspace), h, w);
    rc = wsu_check_launch("ws_sequential_rows_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(ws_sequential_finish_kernel, dim3(n), dim3(256), 0, s, static_cast<const long long*>(workspace), k, t_max, t_all, curve,
                       h - 2, w - 2, order);
    return wsu_check_launch("ws_sequential_finish_kernel");
}

}  // extern "C"
