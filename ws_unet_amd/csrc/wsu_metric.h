// Device helpers shared by the metric kernels K10-K18, K27, K29, K32 and K33 and the simulators K20, K37, K38 and K45-K47 (pointwise.hip K10 + WS meter,
// ws_attack.hip, ws_sequential.hip, ws_ordered.hip, ws_locate.hip, jpeg_history.hip, hill.hip, correlation.hip, error_boxes.hip, embed.hip, ternary.hip, stc_layers.hip): the one definition each of a 3x3 predictor's
// taps, the prediction at a pixel, the float32 residual, the WS statistics' prediction source (WsSource: the kernel argument, its host-side
// maker and checks, the per-image taps, the quotient table) and per-pixel terms, the maximum-prefix triple with its workspace form, block
// finish and the ordered fold of a wave step, the HILL cost's input window, the fixed-order block sum, the +-1 sender's exponentials and the radix-select steps.  (The simulators' pixel loop: wsu_embed.h.)
//
// Rounding policy: these functions restate numpy's float32 / float64 operation sequences with PLAIN operators, one rounding each.  That
// holds only under `#pragma clang fp contract(off)`, which is per translation unit: every including .hip file sets it BEFORE this
// include.  The __f*_rn header intrinsics are no substitute: the pragma does not reach them, they carry hipcc's default contraction and
// fuse with a neighbouring add (tests/test_isa_lint.py counts the f32 FMAs of every kernel that uses this header).
#pragma once
#include "wsu_device.h"

// ---- a 3x3 linear predictor --------------------------------------------------------------------------------------------------------
// k[a*3+b] is the weight of x[r-1+a][c-1+b] (correlation layout).  The reference's kernel arrays K[a][b] (NAMED_FILTERS_2D, applied as a
// true convolution to x[r+1-a][c+1-b]) are the same nine numbers reversed.
template <typename T> struct Taps3x3 { T k[9]; };
template <typename T> inline Taps3x3<T> taps_from_weights(const T* wgt) {         // host; null -> zeros
    Taps3x3<T> t{};
    for (int i = 0; i < 9; ++i) t.k[i] = wgt ? wgt[i] : T(0);
    return t;
}
template <typename T> inline Taps3x3<T> taps_from_kernel(const T* kern) {         // host; K[a][b] of a true convolution; null -> zeros
    Taps3x3<T> t{};
    for (int i = 0; i < 9; ++i) t.k[8 - i] = kern ? kern[i] : T(0);
    return t;
}

// the KB filter's K[a][b] (filters.NAMED_FILTERS_2D['KB']); symmetric, so K and the taps of the correlation layout are the same numbers
// (K32's and K57's in-kernel KB prediction)
__device__ __forceinline__ Taps3x3<float> kb_taps_f32() {
    Taps3x3<float> t;
#pragma unroll
    for (int i = 0; i < 9; ++i) t.k[i] = i == 4 ? 0.0f : (i & 1) ? 0.5f : -0.25f;
    return t;
}

// The sum order is part of a result's bits: REVERSE = false visits x[r-1][c-1] first (x @ filter, K14 / K16), REVERSE = true visits
// x[r+1][c+1] first, i.e. K00 .. K22 of scipy's convolve (K11 / K15).  v[i][j] = x[r-1+i][c-1+j].
template <bool REVERSE> __device__ __forceinline__ float conv9_f32(const Taps3x3<float>& t, const float v[3][3]) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int j = REVERSE ? 8 - i : i;
        acc = acc + t.k[j] * v[j / 3][j % 3];
    }
    return acc;
}
// float64 taps on the uint8 plane `img` (row stride w) at interior pixel (r, c)
template <bool REVERSE> __device__ __forceinline__ double filter_hat64(const Taps3x3<double>& t, const uint8_t* __restrict__ img,
                                                                       int r, int c, int w) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int j = REVERSE ? 8 - i : i;
        acc += t.k[j] * (double)img[(size_t)(r - 1 + j / 3) * w + (c - 1 + j % 3)];
    }
    return acc;
}

// where the prediction at interior pixel (r, c) of image nn lives: (N,H,W) full frames (hat_full) or (N,H-2,W-2) interiors.  The image's
// base is a separate function so that a kernel computes it once, outside its pixel loops.
__device__ __forceinline__ size_t hat_base(int hat_full, int nn, int h, int w) {
    return hat_full ? (size_t)nn * h * w : (size_t)nn * (h - 2) * (w - 2);
}
__device__ __forceinline__ size_t hat_index(int hat_full, size_t base, int r, int c, int w) {
    return hat_full ? base + (size_t)r * w + c : base + (size_t)(r - 1) * (w - 2) + (c - 1);
}

// "K10's float32 residual": x - fl32(y * scale), two roundings (src/unet/evaluate.py:51,125-132)
__device__ __forceinline__ float residual_f32(float x, float y, float scale) {
    const float xhat = y * scale;
    return x - xhat;
}

// ---- the WS statistics' prediction source and per-pixel terms (K11, K27, K29, K33) -------------------------------------------------------
// What a statistic kernel needs to know about its predictor and weights: K11's kernel argument, by value; K27, K29 and K33 put it together
// from their loose parameters (ws_sequential.hip says why).  Exactly one source is set:
// `xhat` (a prediction on the device, N full frames or N interiors: hat_full, multiplied by hat_scale), `pixel_taps` (one 3x3 filter,
// evaluated in the kernel) or `image_filters` (DEVICE, one filter per image, K[a][b] like taps_from_kernel's input); use_pixel_filter says
// whether it is a filter.  weighted: 0 | 1 | -1 (K11 only); xbias / correct_bias: K11 only.  ws_source_make (below) is the only maker.
struct WsSource {
    const float* __restrict__ xhat;
    const float* __restrict__ xbias;
    const float* __restrict__ image_filters;
    Taps3x3<float> mean_taps, pixel_taps;
    int use_pixel_filter, hat_full;
    float hat_scale;
    int weighted, correct_bias;
};
// the pixel taps of image nn: the source's own, or row nn of image_filters reversed (uniform where nn is)
__device__ __forceinline__ Taps3x3<float> ws_source_taps(const WsSource& src, int nn) {
    Taps3x3<float> t = src.pixel_taps;
    if (src.image_filters) {
#pragma unroll
        for (int i = 0; i < 9; ++i) t.k[8 - i] = src.image_filters[(size_t)nn * 9 + i];
    }
    return t;
}
// One 256-thread workgroup fills unit[u] = u / 255.f for every uint8 value, with its barrier, where the source is a filter (uniform over the
// workgroup): one IEEE division per thread instead of nine per pixel, the same bits as dividing per pixel.
__device__ __forceinline__ void ws_unit_table(const WsSource& src, float* unit, int tid) {
    if (src.use_pixel_filter) {
        unit[tid] = (float)tid / 255.0f;
        __syncthreads();
    }
}

// At interior pixel (r, c) of the uint8 plane `img` (row stride w), in numpy's float32 operation sequence (src/ws/estimate.py:90-121):
//   wgt  = 1 (weighted 0) | 1 / (5 + var) (weighted > 0) | 5 + var (weighted < 0),  var = conv(x*x, mean) - conv(x, mean)^2
//   s    = x - x_bar = +-1
//   res  = x - x_hat,  x_hat = conv(x / 255., taps) * 255. (use_pixel_filter; taps = ws_source_taps, `unit` = ws_unit_table's) or
//          xhat[o] * hat_scale, o = hat_index(hat_full, hbase, ...), hbase = hat_base(hat_full, nn, h, w)
//   bias = the predictor applied to x_bar - x (correct_bias only, else 0)
// Convolutions are true convolutions summed K00 .. K22 (conv9_f32<true>).
struct WsTerms { float wgt, s, res, bias; };
__device__ __forceinline__ WsTerms ws_pixel_terms(const uint8_t* __restrict__ img, const WsSource& src, const Taps3x3<float>& taps,
                                                  const float* unit, size_t hbase, int r, int c, int w) {
    float v[3][3], v2[3][3];
    uint8_t u[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            u[i][j] = img[(size_t)(r - 1 + i) * w + (c - 1 + j)];
            v[i][j] = (float)u[i][j];
            v2[i][j] = v[i][j] * v[i][j];
        }
    WsTerms o;
    o.wgt = 1.0f;
    if (src.weighted != 0) {
        const float mu = conv9_f32<true>(src.mean_taps, v);
        const float mu2 = conv9_f32<true>(src.mean_taps, v2);
        const float mu_sq = mu * mu;
        const float var = mu2 - mu_sq;
        const float t = 5.0f + var;
        o.wgt = src.weighted > 0 ? 1.0f / t : t;
    }
    const float x = v[1][1];
    o.s = x - (float)(uint8_t)(u[1][1] ^ 1);                                          // x - x_bar = +-1
    o.bias = 0.f;
    if (src.use_pixel_filter) {
        float q[3][3], qb[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                q[i][j] = unit[u[i][j]];                                                // x / 255. (filters/evaluate.py:136-141)
                qb[i][j] = (u[i][j] & 1) ? -unit[1] : unit[1];                          // (x_bar - x) / 255. = -+1 / 255.
            }
        o.res = residual_f32(x, conv9_f32<true>(taps, q), 255.0f);
        if (src.correct_bias) o.bias = conv9_f32<true>(taps, qb) * 255.0f;
    } else {
        const size_t at = hat_index(src.hat_full, hbase, r, c, w);
        o.res = residual_f32(x, src.xhat[at], src.hat_scale);
        if (src.correct_bias) o.bias = src.xbias[at] * src.hat_scale;
    }
    return o;
}

// The one maker of a WsSource, and the argument checks every statistic entry shares (host; returns WSU_ERR_ARG with "<who>: ..." set).
// `what` names the statistic in the texts ("the sequential statistic"); attack = K11, the only entry with weights 5 + var (weighted = -1)
// and a bias correction.  n, h, w: the planes; a plane may have at most 2^cap_bits interior pixels (WSU_REQUIRE_INTERIOR, wsu_device.h; 0: no cap).
// A filter predicts full frames in pixel units, whatever hat_full / hat_scale say.
inline int ws_source_make(WsSource& src, const char* who, const char* what, bool attack, const float* x_hat, const float* x_bias,
                          const float* pixel_filter, const float* pixel_filters, const float* mean_filter, int hat_full, float hat_scale,
                          int weighted, int correct_bias, int n, int h, int w, int cap_bits) {
    WSU_REQUIRE((x_hat != nullptr) + (pixel_filter != nullptr) + (pixel_filters != nullptr) == 1,
                "%s: give exactly one of x_hat / pixel_filter / pixel_filters", who);
    WSU_REQUIRE(attack || weighted != -1, "%s: weighted=-1 (weights 5 + var) is not defined for %s", who, what);
    WSU_REQUIRE(weighted >= (attack ? -1 : 0) && weighted <= 1, "%s: weighted=%d outside %s", who, weighted, attack ? "{-1,0,1}" : "{0,1}");
    WSU_REQUIRE(weighted == 0 || mean_filter, "%s: weighted estimate needs mean_filter", who);
    WSU_REQUIRE(attack || (!correct_bias && !x_bias), "%s: a bias correction is not defined for %s", who, what);
    WSU_REQUIRE(!correct_bias || !x_hat || x_bias, "%s: correct_bias needs x_bias = pixel_estimator(x_bar - x)", who);
    WSU_REQUIRE_INTERIOR(who, cap_bits);
    const bool filtered = !x_hat;
    src = WsSource{x_hat, x_bias, pixel_filters, taps_from_kernel(mean_filter), taps_from_kernel(pixel_filter), filtered ? 1 : 0,
                   filtered ? 1 : hat_full, filtered ? 255.0f : hat_scale, weighted, correct_bias};
    return 0;
}

// The fixed-point form of a float32 term t (K27, K29, K33): 0 where t is NaN, else llrint((double)min(max(t, -4096), 4096) * 2^24), round to
// nearest even.  |q| <= 2^36, so sums of such terms are exact integers whatever their order.
__device__ __forceinline__ long long ws_seq_term(float t) {
    if (t != t) return 0;                               // NaN
    const float c = t < -4096.0f ? -4096.0f : t > 4096.0f ? 4096.0f : t;
    return __builtin_llrint((double)c * 16777216.0);
}

// ---- the maximum-prefix triple of a run of fixed-point terms (K27, K33) ---------------------------------------------------------------
// (sum, best, arg): the run's sum, the largest of its prefix sums (the empty prefix, 0, takes part) and the position behind the FIRST
// prefix that reaches it, counted from the start of the whole sequence, so that combining shifts nothing.  Runs combine associatively,
// left before right; a single term q at position p is (q, max(q, 0), p + (q > 0)), and a term of 0 never wins on the right.
template <typename A> struct MaxPrefix { long long sum, best; A arg; };
template <typename A> __device__ __forceinline__ MaxPrefix<A> mp_combine(const MaxPrefix<A>& a, const MaxPrefix<A>& b) {
    const long long cand = a.sum + b.best;
    const bool keep = a.best >= cand;                   // >=: among equal maxima the first
    return MaxPrefix<A>{a.sum + b.sum, keep ? a.best : cand, keep ? a.arg : b.arg};
}
// lane 0 receives the wave's 64 triples combined in lane order (lane l holds lanes l .. l + 2 off - 1 after the step `off` where that range
// exists; the other lanes' values are not used)
template <typename A> __device__ __forceinline__ MaxPrefix<A> mp_wave(MaxPrefix<A> a) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        MaxPrefix<A> b;
        b.sum = __shfl_down(a.sum, off, 64);
        b.best = __shfl_down(a.best, off, 64);
        b.arg = __shfl_down(a.arg, off, 64);
        a = mp_combine(a, b);
    }
    return a;
}

// One 256-thread workgroup (one image), thread t holding the triple of the t-th contiguous run of the sequence: an ordered tree over each
// wave, the four waves combined in order, and thread 0 stores k / t_max / t_all of image nn (the tail of K27's and K33's finish kernels).
__device__ __forceinline__ void mp_block_finish(MaxPrefix<long long> run, int tid, int nn, long long* __restrict__ k,
                                                long long* __restrict__ t_max, long long* __restrict__ t_all) {
    __shared__ MaxPrefix<long long> wv[4];
    run = mp_wave(run);
    if ((tid & 63) == 0) wv[tid >> 6] = run;
    __syncthreads();
    if (tid == 0) {
        const MaxPrefix<long long> all = mp_combine(mp_combine(wv[0], wv[1]), mp_combine(wv[2], wv[3]));
        k[nn] = all.arg; t_max[nn] = all.best; t_all[nn] = all.sum;
    }
}
// a triple in the int64 workspace: three consecutive words; `shift` moves a loaded arg to the start of the whole sequence
template <typename A> __device__ __forceinline__ void mp_store(long long* __restrict__ at, const MaxPrefix<A>& t) {
    at[0] = t.sum; at[1] = t.best; at[2] = t.arg;
}
__device__ __forceinline__ MaxPrefix<long long> mp_load(const long long* __restrict__ at, long long shift = 0) {
    return MaxPrefix<long long>{at[0], at[1], at[2] + shift};
}

// ---- the ordered fold of one wave step (K27's rows, K33's chunks) ---------------------------------------------------------------------
// A wave takes WS_FOLD_STEP consecutive positions of a sequence per step.  Lane l computes (or gathers) the terms at c0 + l, c0 + 64 + l, ..,
// so the loads are coalesced; the terms cross the wave's own LDS strip so that lane l then folds the WS_FOLD_PER CONSECUTIVE terms
// 8 l .. 8 l + 7 serially (the textbook running maximum), and one ordered shuffle tree over the wave's 64 triples finishes the step.  (A
// tree over single terms instead costs 2 x K11's time: six dependent steps of five cross-lane moves per pixel.)  No workgroup barrier: a
// wave's strip is its own, LDS executes a wave's accesses in order, and a wavefront fence keeps the compiler from moving a read above the
// writes of the other lanes, or the next step's writes above these reads.
constexpr int WS_FOLD_PER = 8;                          // consecutive positions a lane folds serially per step
constexpr int WS_FOLD_STEP = 64 * WS_FOLD_PER;          // positions per wave step
constexpr int WS_FOLD_PITCH = WS_FOLD_PER + 1;          // LDS pitch of a lane's run in 8-byte words: 72 B, a half-wave's b64 reads hit 32 different bank pairs
constexpr int WS_FOLD_STRIP = 64 * WS_FOLD_PITCH;       // 8-byte words of a wave's strip: term i of the step at i + i / WS_FOLD_PER
// Every lane has written its WS_FOLD_PER terms of the step (the term at offset at = 64 j + lane to st[at + at / WS_FOLD_PER]; 0 past the
// sequence's end, which never wins on the right) to `st`, the wave's strip; c0: the position of the step's first term, counted like the result's arg.  Lane 0's return value is
// the step's triple.
__device__ __forceinline__ MaxPrefix<int> ws_fold_step(const long long* st, int lane, int c0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int first = c0 + lane * WS_FOLD_PER;
    MaxPrefix<int> e{0, 0, first};
#pragma unroll
    for (int j = 0; j < WS_FOLD_PER; ++j) {
        e.sum += st[lane * WS_FOLD_PITCH + j];
        if (e.sum > e.best) { e.best = e.sum; e.arg = first + j + 1; }                   // >: among equal maxima the first
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                               // (the next step's writes stay behind these reads)
    __builtin_amdgcn_wave_barrier();
    return mp_wave(e);
}

// ---- the HILL cost's input window (K12 fp32, K20 fp64) -----------------------------------------------------------------------------
// numpy.pad(mode='symmetric') index, repeated reflection (period 2n): -1 -> 0, -2 -> 1, n -> n-1, ...
__device__ __forceinline__ int sym_fold(int j, int n) {
    const int p = 2 * n;
    int m = j % p;
    m = m < 0 ? m + p : m;
    return m < n ? m : p - 1 - m;
}
// One 256-thread workgroup stages the X x X uint8 window of the tile at (r0, c0) -- x padded 'symmetric', BEFORE rows / columns in front of the
// tile; K12 and K20: pad 9 on every side, (TILE+18)^2 -- into `xs`: LDS row stride TILE + 32, window column wc at wc + 16 - BEFORE, so that a
// tile well inside the image is copied as 16-byte row segments (vec_in: rows and base 16-byte aligned); every other tile reads through the
// fold.  The caller's barrier follows.
template <int TILE, int BEFORE = 9, int X = TILE + 18> __device__ __forceinline__ void hill_stage_window(const uint8_t* __restrict__ img, uint8_t* xs,
                                                                                                       int r0, int c0, int h, int w, int vec_in, int tid) {
    constexpr int XS = TILE + 32, SEGS = XS / 16, OFF = 16 - BEFORE;
    static_assert(BEFORE <= 16 && X - BEFORE <= TILE + 16, "the window must lie inside the 16-byte segments around the tile");
    if (vec_in && r0 - BEFORE >= 0 && r0 - BEFORE + X <= h && c0 - 16 >= 0 && c0 + TILE + 16 <= w) {
        for (int i = tid; i < X * SEGS; i += 256) {
            const int wr = i / SEGS, seg = i % SEGS;
            const u32x4 v = *reinterpret_cast<const u32x4*>(img + (size_t)(r0 - BEFORE + wr) * w + (c0 - 16 + seg * 16));
            *reinterpret_cast<u32x4*>(xs + wr * XS + seg * 16) = v;
        }
    } else {
        for (int i = tid; i < X * X; i += 256) {
            const int wr = i / X, wc = i % X;
            xs[wr * XS + wc + OFF] = img[(size_t)sym_fold(r0 - BEFORE + wr, h) * w + sym_fold(c0 - BEFORE + wc, w)];
        }
    }
}

// ---- fixed-order block sum -----------------------------------------------------------------------------------------------------------
// Every thread has stored its terms in rows[k][tid] (each row THREADS long, double or long long); afterwards rows[k][0] holds row k's sum,
// paired (tid, tid + st) with st halving from THREADS/2, so a sum's bits depend on neither the schedule nor the launch.  One barrier per
// level serves all rows.
template <int THREADS, typename... T> __device__ __forceinline__ void block_sum(int tid, T*... rows) {
    __syncthreads();
    for (int st = THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) ((rows[tid] += rows[tid + st]), ...);
        __syncthreads();
    }
}

// ---- the +-1 sender's exponentials (K37, K38, K45) -------------------------------------------------------------------------------------------
// e = exp(-a) for the two directions of a pixel of value x: 0 for a wet direction and for a = +inf (or NaN)
__device__ __forceinline__ void ternary_exp(uint8_t x, double a, double& ep, double& em) {
    const double e = a < __builtin_inf() ? exp(-a) : 0.0;
    ep = x == 255 ? 0.0 : e;
    em = x == 0 ? 0.0 : e;
}

// ---- exact radix select over float32 bit patterns (K13, K18) -----------------------------------------------------------------------
// Three digit levels of 11 / 11 / 10 bits; `mask` selects the bits the earlier levels fixed.
struct RadixDigit { int shift, bins; uint32_t mask; };
__device__ __forceinline__ RadixDigit radix_digit(int level) {
    return level == 0 ? RadixDigit{21, 2048, 0u} : level == 1 ? RadixDigit{10, 2048, 0xFFE00000u} : RadixDigit{0, 1024, 0xFFFFFC00u};
}
// One 256-thread workgroup: the bin of `hist` (this level's counts of the keys under the prefix st[0]) that holds rank kk, by a
// fixed-order scan; st[0] gains the bin's digit, st[1] becomes the rank within the bin.  C = uint32_t or unsigned long long counts.
template <typename C> __device__ __forceinline__ void radix_pick(const C* __restrict__ hist, C* __restrict__ st, C kk, int level,
                                                                 C* part, int tid) {
    const RadixDigit dg = radix_digit(level);
    const int per = dg.bins / 256;
    C mine = 0;
    for (int j = 0; j < per; ++j) mine += hist[tid * per + j];
    part[tid] = mine;
    __syncthreads();
    C before = 0;                                            // exclusive prefix of this thread's bin range (256 adds: negligible)
    for (int t = 0; t < tid; ++t) before += part[t];
    if (kk < before || kk >= before + mine) return;
    for (int j = 0; j < per; ++j) {
        const C cnt = hist[tid * per + j];
        if (kk < before + cnt) {
            const uint32_t prefix = level == 0 ? 0u : (uint32_t)st[0];
            st[0] = prefix | ((uint32_t)(tid * per + j) << dg.shift);
            st[1] = kk - before;
            return;
        }
        before += cnt;
    }
}
// b = c_(k+1) beside a = c_(k) among `size` keys: a again when k is the last rank or count(c <= a) already covers rank k+1, else
// min(c > a), which the "next" passes keep as the maximum of the complemented bits
__device__ __forceinline__ uint32_t radix_next_bits(uint32_t a, long long k, long long size, long long count_le, uint32_t not_min_gt) {
    return (k + 1 < size && count_le < k + 2) ? ~not_min_gt : a;
}
