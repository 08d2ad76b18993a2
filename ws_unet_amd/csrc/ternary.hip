// K37-K39: the +-1 embedding simulators, LSB matching (LSBM; Sharp, IH 2001) and the payload-limited sender (Filler & Fridrich, IEEE TIFS 5(4), 2010)
// over a cost map, with K20's float64 HILL cost: the embedder the literature calls HILL.  Not part of the reference.
//
//   per pixel, for a multiplier lambda > 0 and a cost rho > 0 (+inf: a wet pixel):
//     a   = lambda * rho                      a+ = +inf where x == 255 (the +1 change is wet), else a;   a- = +inf where x == 0, else a
//     e+- = exp(-a+-)   (exp(-inf) = 0)       Z  = (1 + e+) + e-          p+- = e+- / Z
//   K37  h = log2(Z) + (t+ + t-) / (Z ln 2),  t+- = a e+- where e+- > 0, else 0 (inf * 0 is never formed);  entropy[image][l] = sum of h, bits
//   K38  T+- = floor(p+- * 2^32) in float64;  u = word i % 4 of Philox4x32-10 on counter (i / 4, 0, 0, 0) under the image's seed (K23's word);
//        u < T+ : x + 1;   T+ <= u < T+ + T- : x - 1;   else x.   T+ + T- <= 2/3 * 2^32: the sum fits 32 bits.
//   K39  the same draw with constant thresholds: T+ = T- = T inside the range, (2T, 0) at x == 0, (0, 2T) at x == 255, T = floor(alpha / 4 * 2^32).
//
// A wet direction has threshold 0, so no byte leaves 0..255 and the changes are added to four packed bytes at once without a carry between
// them; nothing is clamped.  float64 operations are plain operators in the order above (contract(off): lambda * rho is a multiply of its own
// that feeds exp).  K37 sums in a fixed order: pixel i of an image belongs to workgroup (i / 256) % TE_PARTS, thread i % 256; a thread adds
// its pixels in ascending order, block_sum pairs the 256 threads, the finish kernel adds the TE_PARTS partials in workgroup order.  So the bits
// depend on (x, rho, lambda, H*W) alone: not on the run, the batch size or the image's place in the batch.
#pragma clang fp contract(off)
#include "wsu_metric.h"
#include "wsu_philox.h"

namespace {

constexpr int TE_PARTS = 64;           // K37 workgroups per image
constexpr int TE_MAXL = 16;            // K37 multipliers per launch, at most
constexpr int PM_MAX_BLOCKS = 64;      // K38 / K39 workgroups per image, at most
constexpr double LN2 = 0.693147180559945309417232121458;
constexpr double TWO32 = 4294967296.0;

// (ternary_exp: wsu_metric.h, shared with the layer kernels K45-K47.)

// ---- K37 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ternary_entropy_partial_kernel(const uint8_t* __restrict__ x, const double* __restrict__ rho,
                                                                      const double* __restrict__ lambdas, double* __restrict__ partial,
                                                                      long long hw, int nl) {
    __shared__ double red[TE_MAXL][256];
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const uint8_t* img = x + (size_t)nn * hw;
    const double* cimg = rho + (size_t)nn * hw;
    double lam[TE_MAXL], acc[TE_MAXL];
#pragma unroll
    for (int l = 0; l < TE_MAXL; ++l) {
        lam[l] = l < nl ? lambdas[(size_t)nn * nl + l] : 0.0;
        acc[l] = 0.0;
    }
    for (long long i = (long long)part * 256 + tid; i < hw; i += (long long)TE_PARTS * 256) {
        const uint8_t px = img[i];
        const double c = cimg[i];
#pragma unroll
        for (int l = 0; l < TE_MAXL; ++l) {
            if (l < nl) {                                                    // (uniform over the launch)
                const double a = lam[l] * c;
                double ep, em;
                ternary_exp(px, a, ep, em);
                const double z = (1.0 + ep) + em;
                const double tp = ep > 0.0 ? a * ep : 0.0;
                const double tm = em > 0.0 ? a * em : 0.0;
                const double t = tp + tm;
                const double den = z * LN2;
                acc[l] += log2(z) + t / den;
            }
        }
    }
#pragma unroll
    for (int l = 0; l < TE_MAXL; ++l) red[l][tid] = acc[l];
    block_sum<256>(tid, red[0], red[1], red[2], red[3], red[4], red[5], red[6], red[7], red[8], red[9], red[10], red[11], red[12], red[13],
                   red[14], red[15]);
    if (tid < nl) partial[((size_t)nn * TE_PARTS + part) * TE_MAXL + tid] = red[tid][0];
}

// thread l of workgroup nn: the TE_PARTS partials of multiplier l, added in workgroup order
__global__ __launch_bounds__(64) void ternary_entropy_finish_kernel(const double* __restrict__ partial, double* __restrict__ entropy, int nl) {
    const int nn = blockIdx.x, l = threadIdx.x;
    if (l >= nl) return;
    double s = 0.0;
    for (int p = 0; p < TE_PARTS; ++p) s += partial[((size_t)nn * TE_PARTS + p) * TE_MAXL + l];
    entropy[(size_t)nn * nl + l] = s;
}

// ---- K38 / K39 ------------------------------------------------------------------------------------------------------------
// (image_span, span_byte_index, add_changes: wsu_metric.h, as K22 / K23 use them.)
// the two thresholds of a pixel of value x.  LSBM: thr = T, `c` unused; else lam * c is the pixel's a.
template <bool LSBM> __device__ __forceinline__ void pm1_thresholds(uint8_t x, double lam, double c, uint32_t thr, uint32_t& tp, uint32_t& tm) {
    if (LSBM) {
        tp = x == 255 ? 0u : x == 0 ? 2u * thr : thr;
        tm = x == 0 ? 0u : x == 255 ? 2u * thr : thr;
    } else {
        const double a = lam * c;
        double ep, em;
        ternary_exp(x, a, ep, em);
        const double z = (1.0 + ep) + em;
        const double pp = ep / z, pm = em / z;
        tp = (uint32_t)(pp * TWO32);                                         // floor: not negative, at most 2^31
        tm = (uint32_t)(pm * TWO32);
    }
}
// +1 / -1 / 0 for the draw u
__device__ __forceinline__ int pm1_draw(uint32_t u, uint32_t tp, uint32_t tm) { return u < tp ? 1 : u - tp < tm ? -1 : 0; }

template <bool LSBM>
__global__ __launch_bounds__(256) void embed_pm1_kernel(const uint8_t* __restrict__ cover, const double* __restrict__ rho,
                                                        const double* __restrict__ lambdas, const uint32_t* __restrict__ thresholds,
                                                        const uint64_t* __restrict__ seeds, uint8_t* __restrict__ stego,
                                                        long long* __restrict__ changes, long long hw) {
    const int nn = blockIdx.y, tid = threadIdx.x;
    const uint8_t* cin = cover + (size_t)nn * hw;
    uint8_t* cout = stego + (size_t)nn * hw;
    const double* rin = LSBM ? nullptr : rho + (size_t)nn * hw;
    const double lam = LSBM ? 0.0 : lambdas[nn];
    const uint32_t thr = LSBM ? thresholds[nn] : 0u;
    const uint32_t k0 = (uint32_t)seeds[nn], k1 = (uint32_t)(seeds[nn] >> 32);
    const Span sp = image_span(cin, cout, hw, true);
    int cnt = 0;
    for (long long g = (long long)blockIdx.x * 256 + tid; g < sp.groups; g += (long long)gridDim.x * 256) {
        const long long p = sp.head + 16 * g;                               // a multiple of 4
        u32x4 v = *reinterpret_cast<const u32x4*>(cin + p);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const Words4 wd = philox4x32_10((uint32_t)(p / 4 + q), k0, k1);
            uint32_t up = 0, dn = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t tp, tm;
                pm1_thresholds<LSBM>((uint8_t)(v[q] >> (8 * e)), lam, LSBM ? 0.0 : rin[p + 4 * q + e], thr, tp, tm);
                const int d = pm1_draw(wd.v[e], tp, tm);
                up |= (d > 0 ? 1u : 0u) << (8 * e);
                dn |= (d < 0 ? 1u : 0u) << (8 * e);
            }
            v[q] = v[q] + up - dn;                                          // no byte carries: a wet direction is never drawn
            cnt += __popc(up | dn);
        }
        *reinterpret_cast<u32x4*>(cout + p) = v;
    }
    for (long long j = (long long)blockIdx.x * 256 + tid; j < sp.bytes; j += (long long)gridDim.x * 256) {
        const long long i = span_byte_index(sp, j);
        const uint8_t xv = cin[i];
        uint32_t tp, tm;
        pm1_thresholds<LSBM>(xv, lam, LSBM ? 0.0 : rin[i], thr, tp, tm);
        const int d = pm1_draw(word_of(philox4x32_10((uint32_t)(i / 4), k0, k1), (int)(i & 3)), tp, tm);
        cout[i] = (uint8_t)((int)xv + d);
        cnt += d != 0 ? 1 : 0;
    }
    add_changes(cnt, changes + nn, tid);
}

int pm1_blocks(long long hw) {
    const long long b = (hw / 16 + 255) / 256;
    return (int)(b < 1 ? 1 : b > PM_MAX_BLOCKS ? PM_MAX_BLOCKS : b);
}

}  // namespace

// a frame's pixel count must fit Philox's 32-bit counter word (4 pixels each), as in embed.hip
#define PM1_REQUIRE_SHAPE(what)                                                                                       \
    WSU_REQUIRE(n > 0 && n <= 65535 && h >= 1 && w >= 1, what ": bad shape n=%d h=%d w=%d", n, h, w);                 \
    WSU_REQUIRE((long long)h * w < (1LL << 32), what ": %lld pixels per image exceed the 32-bit counters", (long long)h * w)

extern "C" {

size_t wsu_ternary_entropy_workspace_bytes(int n) { return n > 0 ? (size_t)n * TE_PARTS * TE_MAXL * sizeof(double) : 0; }

int wsu_ternary_entropy(const uint8_t* x_u8, const double* rho, const double* lambdas, int l, double* entropy, void* workspace,
                        size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && rho && lambdas && entropy && workspace, "ternary_entropy: null pointer");
    PM1_REQUIRE_SHAPE("ternary_entropy");
    WSU_REQUIRE(l >= 1 && l <= TE_MAXL, "ternary_entropy: l=%d multipliers outside 1..%d", l, TE_MAXL);
    WSU_REQUIRE(workspace_bytes >= wsu_ternary_entropy_workspace_bytes(n), "ternary_entropy: workspace too small");
    WSU_REQUIRE((uintptr_t)workspace % 8 == 0, "ternary_entropy: workspace must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(ternary_entropy_partial_kernel, dim3(TE_PARTS, n), dim3(256), 0, s, x_u8, rho, lambdas, partial, (long long)h * w, l);
    int rc = wsu_check_launch("ternary_entropy_partial_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(ternary_entropy_finish_kernel, dim3(n), dim3(64), 0, s, partial, entropy, l);
    return wsu_check_launch("ternary_entropy_finish_kernel");
}

int wsu_embed_ternary(const uint8_t* cover, const double* rho, const double* lambdas, const uint64_t* seeds, uint8_t* stego,
                      long long* changes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(cover && rho && lambdas && seeds && stego && changes, "embed_ternary: null pointer");
    PM1_REQUIRE_SHAPE("embed_ternary");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long hw = (long long)h * w;
    if (hipMemsetAsync(changes, 0, (size_t)n * sizeof(long long), s) != hipSuccess) return wsu_check_launch("embed_ternary memset");
    hipLaunchKernelGGL(embed_pm1_kernel<false>, dim3(pm1_blocks(hw), n), dim3(256), 0, s, cover, rho, lambdas,
                       static_cast<const uint32_t*>(nullptr), seeds, stego, changes, hw);
    return wsu_check_launch("embed_pm1_kernel");
}

int wsu_lsbm_threshold(double alpha, uint32_t* threshold) {
    WSU_REQUIRE(threshold, "lsbm_threshold: null pointer");
    WSU_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "lsbm_threshold: alpha=%g outside [0, 1]", alpha);
    *threshold = (uint32_t)(alpha / 4.0 * TWO32);                       // floor: the product is not negative; at most 2^30
    return 0;
}

int wsu_embed_lsbm(const uint8_t* cover, const uint64_t* seeds, const uint32_t* thresholds, uint8_t* stego, long long* changes,
                   int n, int h, int w, void* stream) {
    WSU_REQUIRE(cover && seeds && thresholds && stego && changes, "embed_lsbm: null pointer");
    PM1_REQUIRE_SHAPE("embed_lsbm");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long hw = (long long)h * w;
    if (hipMemsetAsync(changes, 0, (size_t)n * sizeof(long long), s) != hipSuccess) return wsu_check_launch("embed_lsbm memset");
    hipLaunchKernelGGL(embed_pm1_kernel<true>, dim3(pm1_blocks(hw), n), dim3(256), 0, s, cover, static_cast<const double*>(nullptr),
                       static_cast<const double*>(nullptr), thresholds, seeds, stego, changes, hw);
    return wsu_check_launch("embed_pm1_kernel");
}

}  // extern "C"
