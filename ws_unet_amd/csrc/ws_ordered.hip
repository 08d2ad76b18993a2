// K33: the WS changepoint along a path given per image, for payloads placed in the order of an adaptivity criterion (the informed WS attack
// on naive content-adaptive embedding: Schoettle, Korff, Boehme, WIFS 2012).  Not part of the reference; the per-pixel terms are K11's
// (ws_pixel_terms, wsu_metric.h) and the reduction is K27's exact maximum prefix, only the order in which the terms are added differs.
//
//   The path visits the M = (H-2)(W-2) INTERIOR pixels in the order the caller gives: path[i] is the interior raster index
//   (r-1)(W-2) + (c-1) of the i-th pixel.  The first k pixels are used, a used pixel is flipped with probability pi (HILLR: 1, a real
//   message: 1/2).  With the cover estimate s - pi (s - s_bar) for a used pixel the weighted squared error against the prediction is a
//   constant minus a positive multiple of
//
//       T(k) = sum_{i <= k} w_i * (r_i - tau),     tau = pi / 2,     r_i = (s_i - s_bar_i) * (s_i - s_hat_i),     T(0) = 0.
//
//   per pixel, float32, numpy's operation sequence, nothing contracted (tau = 1/4 gives K27's term):
//       wgt = 1 (weighted 0) | 1 / (5 + var) (weighted 1);   r = s * res;   d = r - tau;   t = wgt * d;   q = ws_seq_term(t)   (int64)
//   per image, int64:
//       k = the smallest k in 0..M with T(k) = sum_{i < k} q[path[i]] maximal;  t_max = T(k);  t_all = T(M).
//
// Kernel A (terms): K27's walk without its reduction: one wave per interior row, lane l computes pixels l, 64 + l, .., so the pixel loads
//   and the 8-byte stores of the term plane (N,M) are coalesced.  Kernel B (fold): one wave per chunk of 4 x 512 consecutive path
//   positions.  Per step (ws_fold_step, wsu_metric.h, K27's) the wave reads 512 path entries coalesced (lane l: 64 j + l) and gathers their
//   terms; lane 0 folds the steps -> one triple per chunk, arg counted from the path's start.  Kernel C (finish): one workgroup per image,
//   thread t folds a contiguous run of chunks, an ordered tree over the 256 threads finishes (mp_block_finish).
// A path entry outside 0..M-1 is never dereferenced: it is compared as unsigned against M and contributes a zero term, as does a
// position past the path's end.  Integer terms make the result independent of the split and of the batch; no atomics at all.
// Traffic: A as K27's plus 8 B per pixel written; B 4 B (path) + 8 B (gathered term: the plane of one 512 x 512 image is 2 MB) per pixel.
#pragma clang fp contract(off)
#include "wsu_metric.h"

namespace {

constexpr int WSO_PARTS = 64;                           // kernel A: workgroups per image, four rows (waves) each per pass
constexpr int WSO_STEPS = 4;                            // steps per chunk
constexpr int WSO_CHUNK = WS_FOLD_STEP * WSO_STEPS;     // path positions per wave = per triple of the workspace

// (loose parameters, the struct put together inside: as K27's rows kernel, ws_sequential.hip says why)
__global__ __launch_bounds__(256) void ws_ordered_terms_kernel(
    const uint8_t* __restrict__ xu8, const float* __restrict__ xhat, Taps3x3<float> mean_taps, Taps3x3<float> pixel_taps,
    const float* __restrict__ image_filters, int use_pixel_filter, int hat_full, float hat_scale, int weighted, float tau,
    long long* __restrict__ terms, int h, int w) {
    __shared__ float unit[256];                          // u / 255.f of every uint8 value (ws_unit_table)
    const WsSource src{xhat, nullptr, image_filters, mean_taps, pixel_taps, use_pixel_filter, hat_full, hat_scale, weighted, 0};
    const int nn = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    if (image_filters) pixel_taps = ws_source_taps(src, nn);                             // (uniform: nn = blockIdx.y)
    ws_unit_table(src, unit, tid);
    const size_t hbase = hat_base(src.hat_full, nn, h, w);
    const int ih = h - 2, iw = w - 2;
    long long* out = terms + (size_t)nn * ih * iw;
    for (int r = 1 + (int)blockIdx.x * 4 + wave; r <= ih; r += WSO_PARTS * 4) {          // (uniform over the wave)
        for (int i = lane; i < iw; i += 64) {
            const WsTerms p = ws_pixel_terms(img, src, pixel_taps, unit, hbase, r, i + 1, w);
            const float rr = p.s * p.res;
            const float d = rr - tau;
            const float t = p.wgt * d;
            out[(size_t)(r - 1) * iw + i] = ws_seq_term(t);
        }
    }
}

__global__ __launch_bounds__(256) void ws_ordered_fold_kernel(const long long* __restrict__ terms, const int* __restrict__ path,
                                                              long long* __restrict__ parts, int m, int chunks) {
    __shared__ long long strip[4][WS_FOLD_STRIP];        // per wave: the step's terms
    const int nn = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (int)blockIdx.x * 4 + wave;
    if (chunk >= chunks) return;                         // (uniform over the wave; no workgroup barrier below)
    const long long* q = terms + (size_t)nn * m;
    const int* pa = path + (size_t)nn * m;
    long long* st = strip[wave];
    MaxPrefix<int> run{0, 0, chunk * WSO_CHUNK};         // (lane 0's is the chunk's)
    for (int c0 = chunk * WSO_CHUNK; c0 < (chunk + 1) * WSO_CHUNK && c0 < m; c0 += WS_FOLD_STEP) {
        for (int j = 0; j < WS_FOLD_PER; ++j) {
            const int at = 64 * j + lane, i = c0 + at;
            long long v = 0;                             // past the path's end, or no pixel of the plane: 0, which never wins on the right
            if (i < m) {
                const unsigned p = (unsigned)pa[i];
                if (p < (unsigned)m) v = q[p];
            }
            st[at + at / WS_FOLD_PER] = v;
        }
        run = mp_combine(run, ws_fold_step(st, lane, c0));
    }
    if (lane == 0) mp_store(parts + ((size_t)nn * chunks + chunk) * 3, run);
}

__global__ __launch_bounds__(256) void ws_ordered_finish_kernel(const long long* __restrict__ parts, long long* __restrict__ k,
                                                                long long* __restrict__ t_max, long long* __restrict__ t_all, int chunks) {
    const int nn = blockIdx.x, tid = threadIdx.x;
    const long long* img = parts + (size_t)nn * chunks * 3;
    const int per = (chunks + 255) / 256;                // chunks per thread, contiguous
    const long long p0 = (long long)tid * per;
    const long long p1 = p0 + per < chunks ? p0 + per : chunks;
    MaxPrefix<long long> run{0, 0, p0 * WSO_CHUNK};
    for (long long p = p0; p < p1; ++p) run = mp_combine(run, mp_load(img + p * 3));
    mp_block_finish(run, tid, nn, k, t_max, t_all);
}

long long interior(int h, int w) { return (long long)(h - 2) * (w - 2); }
long long chunks_of(long long m) { return (m + WSO_CHUNK - 1) / WSO_CHUNK; }
size_t terms_bytes(int n, long long m) { return (size_t)n * (size_t)m * sizeof(long long); }

}  // namespace

extern "C" {

size_t wsu_ws_ordered_fold_workspace_bytes(int n, int h, int w) {
    return n > 0 && h >= 3 && w >= 3 ? (size_t)n * (size_t)chunks_of(interior(h, w)) * 3 * sizeof(long long) : 0;
}

size_t wsu_ws_ordered_workspace_bytes(int n, int h, int w) {
    return n > 0 && h >= 3 && w >= 3 ? terms_bytes(n, interior(h, w)) + wsu_ws_ordered_fold_workspace_bytes(n, h, w) : 0;
}

int wsu_ws_ordered_terms(const uint8_t* x_u8, const float* x_hat, const float* pixel_filter, const float* pixel_filters,
                         const float* mean_filter, int hat_full, float hat_scale, int weighted, float tau, long long* terms, int n, int h, int w,
                         void* stream) {
    WSU_REQUIRE(x_u8 && terms, "ws_ordered: null pointer");
    WsSource src;
    int rc = ws_source_make(src, "ws_ordered", "the changepoint statistic", false, x_hat, nullptr, pixel_filter, pixel_filters, mean_filter,
                            hat_full, hat_scale, weighted, 0, n, h, w, 27);
    if (rc) return rc;
    WSU_REQUIRE(tau > 0.0f && tau <= 0.5f, "ws_ordered: tau=%g outside (0, 0.5] (tau = flip rate / 2)", (double)tau);
    WSU_REQUIRE((uintptr_t)terms % 8 == 0, "ws_ordered: terms must be 8-byte aligned");
    hipLaunchKernelGGL(ws_ordered_terms_kernel, dim3(WSO_PARTS, n), dim3(256), 0, static_cast<hipStream_t>(stream), x_u8, src.xhat, src.mean_taps,
                       src.pixel_taps, src.image_filters, src.use_pixel_filter, src.hat_full, src.hat_scale, src.weighted, tau, terms, h, w);
    return wsu_check_launch("ws_ordered_terms_kernel");
}

int wsu_ws_ordered_fold(const long long* terms, const int* path, long long* k, long long* t_max, long long* t_all, void* workspace,
                        size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(terms && path && k && t_max && t_all && workspace, "ws_ordered_fold: null pointer");
    WSU_REQUIRE_INTERIOR("ws_ordered_fold", 27);
    WSU_REQUIRE(workspace_bytes >= wsu_ws_ordered_fold_workspace_bytes(n, h, w), "ws_ordered_fold: workspace too small");
    WSU_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)terms % 8 == 0 && (uintptr_t)path % 4 == 0,
                "ws_ordered_fold: terms and workspace must be 8-byte aligned, path 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int m = (int)interior(h, w), chunks = (int)chunks_of(m);
    hipLaunchKernelGGL(ws_ordered_fold_kernel, dim3((chunks + 3) / 4, n), dim3(256), 0, s, terms, path, static_cast<long long*>(workspace), m,
                       chunks);
    int rc = wsu_check_launch("ws_ordered_fold_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(ws_ordered_finish_kernel, dim3(n), dim3(256), 0, s, static_cast<const long long*>(workspace), k, t_max, t_all, chunks);
    return wsu_check_launch("ws_ordered_finish_kernel");
}

int wsu_ws_ordered(const uint8_t* x_u8, const float* x_hat, const float* pixel_filter, const float* pixel_filters, const float* mean_filter,
                   int hat_full, float hat_scale, int weighted, float tau, const int* path, long long* k, long long* t_max, long long* t_all,
                   void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(path && k && t_max && t_all && workspace, "ws_ordered: null pointer");
    WSU_REQUIRE(workspace_bytes >= wsu_ws_ordered_workspace_bytes(n, h, w), "ws_ordered: workspace too small");
    WSU_REQUIRE((uintptr_t)workspace % 8 == 0, "ws_ordered: workspace must be 8-byte aligned");
    long long* terms = static_cast<long long*>(workspace);
    int rc = wsu_ws_ordered_terms(x_u8, x_hat, pixel_filter, pixel_filters, mean_filter, hat_full, hat_scale, weighted, tau, terms, n, h, w,
                                  stream);
    if (rc) return rc;
    const size_t off = terms_bytes(n, interior(h, w));
    return wsu_ws_ordered_fold(terms, path, k, t_max, t_all, static_cast<char*>(workspace) + off, workspace_bytes - off, n, h, w, stream);
}

}  // extern "C"
