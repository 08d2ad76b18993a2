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
//   positions.  Per step the wave reads 512 path entries coalesced (lane l: 64 j + l), gathers their terms, and passes them through its own
//   LDS strip so that lane l folds the eight CONSECUTIVE terms 8 l .. 8 l + 7 serially; one ordered shuffle tree over the 64 triples
//   finishes the step, lane 0 folds the steps -> one triple per chunk, arg counted from the path's start.  Kernel C (finish): one workgroup
//   per image, thread t folds a contiguous run of chunks, an ordered tree over the 256 threads finishes.
// A path entry outside 0..M-1 is never dereferenced: it is compared as unsigned against M and contributes a zero term, as does a
// position past the path's end.  Integer terms make the result independent of the split and of the batch; no atomics at all.
// Traffic: A as K27's plus 8 B per pixel written; B 4 B (path) + 8 B (gathered term: the plane of one 512 x 512 image is 2 MB) per pixel.
#pragma clang fp contract(off)
#include "wsu_metric.h"

namespace {

constexpr int WSO_PARTS = 64;                           // kernel A: workgroups per image, four rows (waves) each per pass
constexpr int WSO_PER = 8;                              // consecutive path positions a lane folds serially per step
constexpr int WSO_STEP = 64 * WSO_PER;                  // path positions per wave step
constexpr int WSO_STEPS = 4;                            // steps per chunk
constexpr int WSO_CHUNK = WSO_STEP * WSO_STEPS;         // path positions per wave = per triple of the workspace
constexpr int WSO_PITCH = WSO_PER + 1;                  // LDS pitch of a lane's run in 8-byte words (K27's: 72 B)
using Taps = Taps3x3<float>;

__global__ __launch_bounds__(256) void ws_ordered_terms_kernel(
    const uint8_t* __restrict__ xu8, const float* __restrict__ xhat, Taps mean_taps, Taps pixel_taps, const float* __restrict__ image_filters,
    int use_pixel_filter, int hat_full, float hat_scale, int weighted, float tau, long long* __restrict__ terms, int h, int w) {
    __shared__ float unit[256];                          // u / 255.f of every uint8 value (K11)
    const int nn = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    if (image_filters) {                                 // one filter per image (uniform: nn = blockIdx.y)
#pragma unroll
        for (int i = 0; i < 9; ++i) pixel_taps.k[8 - i] = image_filters[(size_t)nn * 9 + i];
    }
    if (use_pixel_filter) {                              // (uniform over the workgroup)
        unit[tid] = (float)tid / 255.0f;
        __syncthreads();
    }
    const size_t hbase = hat_base(hat_full, nn, h, w);
    const int ih = h - 2, iw = w - 2;
    long long* out = terms + (size_t)nn * ih * iw;
    for (int r = 1 + (int)blockIdx.x * 4 + wave; r <= ih; r += WSO_PARTS * 4) {          // (uniform over the wave)
        for (int i = lane; i < iw; i += 64) {
            const WsTerms p = ws_pixel_terms(img, xhat, nullptr, unit, mean_taps, pixel_taps, use_pixel_filter, hat_full, hbase, hat_scale,
                                             weighted, 0, r, i + 1, w);
            const float rr = p.s * p.res;
            const float d = rr - tau;
            const float t = p.wgt * d;
            out[(size_t)(r - 1) * iw + i] = ws_seq_term(t);
        }
    }
}

__global__ __launch_bounds__(256) void ws_ordered_fold_kernel(const long long* __restrict__ terms, const int* __restrict__ path,
                                                              long long* __restrict__ parts, int m, int chunks) {
    __shared__ long long strip[4][64 * WSO_PITCH];       // per wave: the step's terms, term i at i + i / WSO_PER
    const int nn = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (int)blockIdx.x * 4 + wave;
    if (chunk >= chunks) return;                         // (uniform over the wave; no workgroup barrier below)
    const long long* q = terms + (size_t)nn * m;
    const int* pa = path + (size_t)nn * m;
    long long* st = strip[wave];
    MaxPrefix<int> run{0, 0, chunk * WSO_CHUNK};         // (lane 0's is the chunk's)
    for (int c0 = chunk * WSO_CHUNK; c0 < (chunk + 1) * WSO_CHUNK && c0 < m; c0 += WSO_STEP) {
        for (int j = 0; j < WSO_PER; ++j) {
            const int at = 64 * j + lane, i = c0 + at;
            long long v = 0;                             // past the path's end, or no pixel of the plane: 0, which never wins on the right
            if (i < m) {
                const unsigned p = (unsigned)pa[i];
                if (p < (unsigned)m) v = q[p];
            }
            st[at + at / WSO_PER] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int first = c0 + lane * WSO_PER;
        MaxPrefix<int> e{0, 0, first};
#pragma unroll
        for (int j = 0; j < WSO_PER; ++j) {
            e.sum += st[lane * WSO_PITCH + j];
            if (e.sum > e.best) { e.best = e.sum; e.arg = first + j + 1; }               // >: among equal maxima the first
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                           // (the next step's writes stay behind these reads)
        __builtin_amdgcn_wave_barrier();
        run = mp_combine(run, mp_wave(e));
    }
    if (lane == 0) {
        long long* o = parts + ((size_t)nn * chunks + chunk) * 3;
        o[0] = run.sum; o[1] = run.best; o[2] = run.arg;
    }
}

__global__ __launch_bounds__(256) void ws_ordered_finish_kernel(const long long* __restrict__ parts, long long* __restrict__ k,
                                                                long long* __restrict__ t_max, long long* __restrict__ t_all, int chunks) {
    __shared__ MaxPrefix<long long> wv[4];
    const int nn = blockIdx.x, tid = threadIdx.x;
    const long long* img = parts + (size_t)nn * chunks * 3;
    const int per = (chunks + 255) / 256;                // chunks per thread, contiguous
    const long long p0 = (long long)tid * per;
    const long long p1 = p0 + per < chunks ? p0 + per : chunks;
    MaxPrefix<long long> run{0, 0, p0 * WSO_CHUNK};
    for (long long p = p0; p < p1; ++p) run = mp_combine(run, MaxPrefix<long long>{img[p * 3], img[p * 3 + 1], img[p * 3 + 2]});
    run = mp_wave(run);
    if ((tid & 63) == 0) wv[tid >> 6] = run;
    __syncthreads();
    if (tid == 0) {
        const MaxPrefix<long long> all = mp_combine(mp_combine(wv[0], wv[1]), mp_combine(wv[2], wv[3]));
        k[nn] = all.arg; t_max[nn] = all.best; t_all[nn] = all.sum;
    }
}

long long interior(int h, int w) { return (long long)(h - 2) * (w - 2); }
long long chunks_of(long long m) { return (m + WSO_CHUNK - 1) / WSO_CHUNK; }
size_t terms_bytes(int n, long long m) { return (size_t)n * (size_t)m * sizeof(long long); }

}  // namespace

#define WSO_REQUIRE_SHAPE(what)                                                                                        \
    WSU_REQUIRE(n > 0 && n <= 65535 && h >= 3 && w >= 3, what ": bad shape n=%d h=%d w=%d", n, h, w);                  \
    WSU_REQUIRE(interior(h, w) <= (1LL << 27), what ": %lld interior pixels per image exceed 2^27", interior(h, w))

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
    WSU_REQUIRE((x_hat != nullptr) + (pixel_filter != nullptr) + (pixel_filters != nullptr) == 1,
                "ws_ordered: give exactly one of x_hat / pixel_filter / pixel_filters");
    WSU_REQUIRE(weighted != -1, "ws_ordered: weighted=-1 (weights 5 + var) is not defined for the changepoint statistic");
    WSU_REQUIRE(weighted == 0 || weighted == 1, "ws_ordered: weighted=%d outside {0,1}", weighted);
    WSU_REQUIRE(weighted == 0 || mean_filter, "ws_ordered: weighted estimate needs mean_filter");
    WSU_REQUIRE(tau > 0.0f && tau <= 0.5f, "ws_ordered: tau=%g outside (0, 0.5] (tau = flip rate / 2)", (double)tau);
    WSO_REQUIRE_SHAPE("ws_ordered");
    WSU_REQUIRE((uintptr_t)terms % 8 == 0, "ws_ordered: terms must be 8-byte aligned");
    const int filtered = x_hat ? 0 : 1;
    hipLaunchKernelGGL(ws_ordered_terms_kernel, dim3(WSO_PARTS, n), dim3(256), 0, static_cast<hipStream_t>(stream), x_u8, x_hat,
                       taps_from_kernel(mean_filter), taps_from_kernel(pixel_filter), pixel_filters, filtered, filtered ? 1 : hat_full,
                       filtered ? 255.0f : hat_scale, weighted, tau, terms, h, w);
    return wsu_check_launch("ws_ordered_terms_kernel");
}

int wsu_ws_ordered_fold(const long long* terms, const int* path, long long* k, long long* t_max, long long* t_all, void* workspace,
                        size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(terms && path && k && t_max && t_all && workspace, "ws_ordered_fold: null pointer");
    WSO_REQUIRE_SHAPE("ws_ordered_fold");
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
