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
// K38 and K39 are one rule (Pm1Rule) of the simulators' pixel loop, embed_span of wsu_embed.h, which also owns the launch set-up.
// A wet direction has threshold 0, so no byte leaves 0..255 and the changes are added to four packed bytes at once without a carry between
// them; nothing is clamped.  float64 operations are plain operators in the order above (contract(off): lambda * rho is a multiply of its own
// that feeds exp).  K37 sums in a fixed order: pixel i of an image belongs to workgroup (i / 256) % TE_PARTS, thread i % 256; a thread adds
// its pixels in ascending order, block_sum pairs the 256 threads, the finish kernel adds the TE_PARTS partials in workgroup order.  So the bits
// depend on (x, rho, lambda, H*W) alone: not on the run, the batch size or the image's place in the batch.
#pragma clang fp contract(off)
#include "wsu_metric.h"
#include "wsu_embed.h"
#include "wsu_philox.h"

namespace {

constexpr int TE_PARTS = 64;           // K37 workgroups per image
constexpr int TE_MAXL = 16;            // K37 multipliers per launch, at most
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

// ---- K38 / K39: a rule of embed_span ------------------------------------------------------------------------------------------------------
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

// The image's state: seed halves, lambda with the cost row (K38) or the constant threshold (K39, no cost is read).
template <bool LSBM> struct Pm1Rule {
    SeedKey k;
    uint32_t thr;
    double lam;
    const double* rin;
    // +1 / -1 / 0 for pixel i of value x under the draw u
    __device__ __forceinline__ int draw(long long i, uint8_t x, uint32_t u) const {
        uint32_t tp, tm;
        pm1_thresholds<LSBM>(x, lam, LSBM ? 0.0 : rin[i], thr, tp, tm);
        return u < tp ? 1 : u - tp < tm ? -1 : 0;
    }
    __device__ __forceinline__ uint32_t quad(long long i0, uint32_t x, int& cnt) const {
        const Words4 wd = philox_quad(i0, k);
        uint32_t up = 0, dn = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int d = draw(i0 + e, (uint8_t)(x >> (8 * e)), wd.v[e]);
            up |= (d > 0 ? 1u : 0u) << (8 * e);
            dn |= (d < 0 ? 1u : 0u) << (8 * e);
        }
        cnt += __popc(up | dn);
        return x + up - dn;                                                  // no byte carries: a wet direction is never drawn
    }
    __device__ __forceinline__ uint8_t byte(long long i, uint8_t x, int& cnt) const {
        const int d = draw(i, x, philox_byte(i, k));
        cnt += d != 0 ? 1 : 0;
        return (uint8_t)((int)x + d);
    }
};

// (At most 100 SGPRs: beyond them a SIMD holds 7 waves instead of 8, and 32 planes of 512 x 512 are 8 waves per SIMD.  K39 took 106 without
// the limit and was 1.2 % slower for it, profiles/r33.  The attribute is on the template, so K38 has it too and does not need it: it
// takes 84.  The limit does not fail a build: a change that needs more spills SGPRs to VGPR lanes in silence.  If K39 slows down, look at
// `make isa` for v_writelane / v_readlane in its loop and at the kernel's VGPRs in -Rpass-analysis=kernel-resource-usage: above 64 a SIMD
// holds 7 waves again, and then the limit is better raised or dropped.)
template <bool LSBM>
__global__ __attribute__((amdgpu_num_sgpr(100))) __launch_bounds__(256) void embed_pm1_kernel(const uint8_t* __restrict__ cover, const double* __restrict__ rho,
                                                        const double* __restrict__ lambdas, const uint32_t* __restrict__ thresholds,
                                                        const uint64_t* __restrict__ seeds, uint8_t* __restrict__ stego,
                                                        long long* __restrict__ changes, long long hw) {
    const int nn = blockIdx.y;
    const Pm1Rule<LSBM> rule{SeedKey(seeds[nn]), LSBM ? thresholds[nn] : 0u, LSBM ? 0.0 : lambdas[nn], LSBM ? nullptr : rho + (size_t)nn * hw};
    embed_span(rule, cover + (size_t)nn * hw, stego + (size_t)nn * hw, hw, changes + nn);
}

// ---- K51: the sender's change probability as a 16-bit weight ---------------------------------------------------------------------------------
// q = floor((e+ + e-) / Z * 2^16) with K38's a, e+-, Z: beta <= 2/3, so q <= 43 690.  A thread takes four pixels and stores them with one
// 8-byte store where the plane allows it (pixel index and address both multiples of 4), else pixel by pixel.
__device__ __forceinline__ uint32_t change_weight(uint8_t x, double lam, double c) {
    const double a = lam * c;
    double ep, em;
    ternary_exp(x, a, ep, em);
    const double z = (1.0 + ep) + em;
    const double beta = (ep + em) / z;
    return (uint32_t)(beta * 65536.0);                                       // floor: not negative
}

__global__ __launch_bounds__(256) void change_weights_kernel(const uint8_t* __restrict__ x, const double* __restrict__ rho,
                                                             const double* __restrict__ lambdas, uint16_t* __restrict__ weights, long long hw) {
    const int nn = blockIdx.y;
    const double lam = lambdas[nn];
    const uint8_t* img = x + (size_t)nn * hw;
    const double* cimg = rho + (size_t)nn * hw;
    uint16_t* out = weights + (size_t)nn * hw;
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 + 4 <= hw && (reinterpret_cast<uintptr_t>(out + i0) & 7) == 0) {
        uint32_t q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = change_weight(img[i0 + e], lam, cimg[i0 + e]);
        *reinterpret_cast<uint2*>(out + i0) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
    } else {
        for (long long i = i0; i < min(i0 + 4, hw); ++i) out[i] = (uint16_t)change_weight(img[i], lam, cimg[i]);
    }
}

}  // namespace

extern "C" {

int wsu_change_weights(const uint8_t* x_u8, const double* rho, const double* lambdas, uint16_t* weights_u16, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && rho && lambdas && weights_u16, "change_weights: null pointer");
    WSU_REQUIRE_SHAPE("change_weights", WSU_COUNTER_PIXELS, "counters");
    const long long hw = (long long)h * w;
    hipLaunchKernelGGL(change_weights_kernel, dim3((unsigned)((hw + 1023) / 1024), n), dim3(256), 0, static_cast<hipStream_t>(stream), x_u8,
                       rho, lambdas, weights_u16, hw);
    return wsu_check_launch("change_weights_kernel");
}

size_t wsu_ternary_entropy_workspace_bytes(int n) { return n > 0 ? (size_t)n * TE_PARTS * TE_MAXL * sizeof(double) : 0; }

int wsu_ternary_entropy(const uint8_t* x_u8, const double* rho, const double* lambdas, int l, double* entropy, void* workspace,
                        size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && rho && lambdas && entropy && workspace, "ternary_entropy: null pointer");
    WSU_REQUIRE_SHAPE("ternary_entropy", WSU_COUNTER_PIXELS, "counters");
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
    WSU_REQUIRE_SHAPE("embed_ternary", WSU_COUNTER_PIXELS, "counters");
    return embed_launch("embed_ternary memset", "embed_pm1_kernel", embed_pm1_kernel<false>, changes, n, h, w, stream, cover, rho, lambdas,
                        static_cast<const uint32_t*>(nullptr), seeds, stego, changes, (long long)h * w);
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
    WSU_REQUIRE_SHAPE("embed_lsbm", WSU_COUNTER_PIXELS, "counters");
    return embed_launch("embed_lsbm memset", "embed_pm1_kernel", embed_pm1_kernel<true>, changes, n, h, w, stream, cover,
                        static_cast<const double*>(nullptr), static_cast<const double*>(nullptr), thresholds, seeds, stego, changes,
                        (long long)h * w);
}

}  // extern "C"
