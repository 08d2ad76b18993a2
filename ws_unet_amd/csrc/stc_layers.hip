// K45-K47: the plane kernels of the ternary two-layer syndrome-trellis embedder (Filler, Judas, Fridrich, IEEE TIFS 6(3), 2011, sections V-VI,
// for +-1 changes): two binary codes (K43), first over bit 1 of the pixels, then over bit 0.  Not part of the reference.
//
//   per pixel x with cost rho >= 0 (+inf: wet) and the image's multiplier lambda, K37's text:
//     a = lambda * rho;   a+ = +inf where x == 255, else a;   a- = +inf where x == 0, else a;   e+- = exp(-a+-);   Z = (1 + e+) + e-
//   d = the direction that changes bit 1 of x: +1 for odd x, -1 for even x;  o = the other direction (x + o only changes bit 0)
//   K45  u1 = (x >> 1) & 1;   rho1 = a_d + log1p(e_o)  ( = ln((1 - q1) / q1), q1 = e_d / Z; +inf where a_d is );
//        h1 = (r log1p(t)) / ln 2 - q1 log2(q1) where e_d > 0, else 0, with r = (1 + e_o) / Z and t = e_d / (1 + e_o): the binary entropy of
//        q1 in bits, every term positive;   H1[image] = the sum of h1
//   K46  decided = k1 > 0 and (y1 & 1) != u1:  u0 = 1 - (x & 1), rho0 = +inf;   else u0 = x & 1, rho0 = a_o
//   K47  good = ok1 and ok0;   x + d where good and decided (never at the end of the range d points to);   x + o where good, not decided and
//        (y0 & 1) != (x & 1);   else x.   changes = the number of changed pixels, distortion = the sum of rho over them, ok = good
//
// contract(off): lambda * rho is a multiply of its own, as in K37.  K45 and K47 sum in K37's fixed order: pixel i belongs to workgroup
// (i / 256) % SL_PARTS, thread i % 256; a thread adds its pixels in ascending order, block_sum pairs the 256 threads, the finish kernel adds
// the SL_PARTS partials in workgroup order.  So the bits depend on the image alone, not on the batch.  Every access is one element per lane
// at consecutive addresses: a wave reads 512 contiguous bytes of rho and 64 of x per step (K38 gives each thread 128 contiguous bytes of
// rho instead, which splits a wave's load over 64 cache lines).
#pragma clang fp contract(off)
#include "wsu_metric.h"

namespace {

constexpr int SL_PARTS = 64;           // workgroups per image
constexpr double LN2 = 0.693147180559945309417232121458;

// a and e of the two directions of a pixel, named by what they do to bit 1
struct LayerTerms { double ad, ao, ed, eo, z; };
__device__ __forceinline__ LayerTerms layer_terms(uint8_t x, double lam, double c) {
    const double inf = __builtin_inf();
    const double a = lam * c;
    double ep, em;
    ternary_exp(x, a, ep, em);
    const double ap = x == 255 ? inf : a, am = x == 0 ? inf : a;
    const bool odd = (x & 1) != 0;
    return LayerTerms{odd ? ap : am, odd ? am : ap, odd ? ep : em, odd ? em : ep, (1.0 + ep) + em};
}

// ---- K45 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stc_layer_high_kernel(const uint8_t* __restrict__ x, const double* __restrict__ rho,
                                                             const double* __restrict__ lambdas, uint8_t* __restrict__ u1,
                                                             double* __restrict__ rho1, double* __restrict__ partial, long long hw) {
    __shared__ double red[256];
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const uint8_t* img = x + (size_t)nn * hw;
    const double* cimg = rho + (size_t)nn * hw;
    uint8_t* uimg = u1 + (size_t)nn * hw;
    double* rimg = rho1 + (size_t)nn * hw;
    const double lam = lambdas[nn];
    double acc = 0.0;
    for (long long i = (long long)part * 256 + tid; i < hw; i += (long long)SL_PARTS * 256) {
        const uint8_t px = img[i];
        const LayerTerms t = layer_terms(px, lam, cimg[i]);
        const double one_o = 1.0 + t.eo;
        double hb = 0.0;
        if (t.ed > 0.0) {
            const double q = t.ed / t.z, r = one_o / t.z, s = t.ed / one_o;
            hb = (r * log1p(s)) / LN2 - q * log2(q);
        }
        acc += hb;
        uimg[i] = (px >> 1) & 1;
        rimg[i] = t.ad + log1p(t.eo);
    }
    red[tid] = acc;
    block_sum<256>(tid, red);
    if (tid == 0) partial[(size_t)nn * SL_PARTS + part] = red[0];
}

// thread = image: its SL_PARTS partials, added in workgroup order
__global__ __launch_bounds__(64) void stc_layer_high_finish_kernel(const double* __restrict__ partial, double* __restrict__ entropy, int n) {
    const int nn = blockIdx.x * 64 + threadIdx.x;
    if (nn >= n) return;
    double s = 0.0;
    for (int p = 0; p < SL_PARTS; ++p) s += partial[(size_t)nn * SL_PARTS + p];
    entropy[nn] = s;
}

// ---- K46 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stc_layer_low_kernel(const uint8_t* __restrict__ x, const double* __restrict__ rho,
                                                            const double* __restrict__ lambdas, const uint8_t* __restrict__ y1,
                                                            const int32_t* __restrict__ k1, uint8_t* __restrict__ u0,
                                                            double* __restrict__ rho0, long long hw) {
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const uint8_t* img = x + (size_t)nn * hw;
    const double* cimg = rho + (size_t)nn * hw;
    const uint8_t* yimg = y1 + (size_t)nn * hw;
    uint8_t* uimg = u0 + (size_t)nn * hw;
    double* rimg = rho0 + (size_t)nn * hw;
    const double lam = lambdas[nn], inf = __builtin_inf();
    const bool high = k1[nn] > 0;                                               // else y1 is not read
    for (long long i = (long long)part * 256 + tid; i < hw; i += (long long)SL_PARTS * 256) {
        const uint8_t px = img[i];
        const double a = lam * cimg[i];
        const bool odd = (px & 1) != 0;
        const double ao = odd ? (px == 0 ? inf : a) : (px == 255 ? inf : a);    // (neither end is reached: an odd pixel is not 0)
        const bool decided = high && (yimg[i] & 1) != ((px >> 1) & 1);
        uimg[i] = decided ? 1 - (px & 1) : px & 1;
        rimg[i] = decided ? inf : ao;
    }
}

// ---- K47 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stc_layer_compose_kernel(const uint8_t* cover, const double* __restrict__ rho,
                                                                const uint8_t* __restrict__ y1, const uint8_t* __restrict__ y0,
                                                                const int32_t* __restrict__ k1, const uint8_t* __restrict__ ok1,
                                                                const uint8_t* __restrict__ ok0, uint8_t* stego,
                                                                double* __restrict__ partial_d, long long* __restrict__ partial_c,
                                                                long long hw) {
    __shared__ double red[256];
    __shared__ long long cred[256];
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const uint8_t* cimg = cover + (size_t)nn * hw;                             // (stego may be cover: a pixel is read, then written, by one thread)
    const double* rimg = rho + (size_t)nn * hw;
    const uint8_t* y1img = y1 + (size_t)nn * hw;
    const uint8_t* y0img = y0 + (size_t)nn * hw;
    uint8_t* simg = stego + (size_t)nn * hw;
    const bool good = ok1[nn] != 0 && ok0[nn] != 0;
    const bool high = good && k1[nn] > 0;
    double acc = 0.0;
    long long cnt = 0;
    for (long long i = (long long)part * 256 + tid; i < hw; i += (long long)SL_PARTS * 256) {
        const uint8_t px = cimg[i];
        const bool odd = (px & 1) != 0;
        const int d = odd ? 1 : -1;
        const bool decided = high && (y1img[i] & 1) != ((px >> 1) & 1) && px != (odd ? 255 : 0);
        const bool low = good && !decided && (y0img[i] & 1) != (px & 1);
        if (decided || low) {
            acc += rimg[i];
            ++cnt;
        }
        simg[i] = (uint8_t)(decided ? px + d : low ? px - d : px);
    }
    red[tid] = acc;
    cred[tid] = cnt;
    block_sum<256>(tid, red, cred);
    if (tid == 0) {
        partial_d[(size_t)nn * SL_PARTS + part] = red[0];
        partial_c[(size_t)nn * SL_PARTS + part] = cred[0];
    }
}

__global__ __launch_bounds__(64) void stc_layer_compose_finish_kernel(const double* __restrict__ partial_d, const long long* __restrict__ partial_c,
                                                                      const uint8_t* __restrict__ ok1, const uint8_t* __restrict__ ok0,
                                                                      long long* __restrict__ changes, double* __restrict__ distortion,
                                                                      uint8_t* __restrict__ ok, int n) {
    const int nn = blockIdx.x * 64 + threadIdx.x;
    if (nn >= n) return;
    double s = 0.0;
    long long c = 0;
    for (int p = 0; p < SL_PARTS; ++p) {
        s += partial_d[(size_t)nn * SL_PARTS + p];
        c += partial_c[(size_t)nn * SL_PARTS + p];
    }
    distortion[nn] = s;
    changes[nn] = c;
    ok[nn] = ok1[nn] != 0 && ok0[nn] != 0 ? 1 : 0;
}

}  // namespace

extern "C" {

size_t wsu_stc_layer_workspace_bytes(int n) { return n > 0 ? (size_t)n * SL_PARTS * (sizeof(double) + sizeof(long long)) : 0; }

int wsu_stc_layer_high(const uint8_t* x_u8, const double* rho, const double* lambdas, uint8_t* u1, double* rho1, double* entropy,
                       void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && rho && lambdas && u1 && rho1 && entropy && workspace, "stc_layer_high: null pointer");
    WSU_REQUIRE_SHAPE("stc_layer_high", WSU_PATH_PIXELS, "path");       // (the planes feed K43, whose paths are int32)
    WSU_REQUIRE(workspace_bytes >= wsu_stc_layer_workspace_bytes(n), "stc_layer_high: workspace too small");
    WSU_REQUIRE((uintptr_t)workspace % 8 == 0, "stc_layer_high: workspace must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(stc_layer_high_kernel, dim3(SL_PARTS, n), dim3(256), 0, s, x_u8, rho, lambdas, u1, rho1, partial, (long long)h * w);
    const int rc = wsu_check_launch("stc_layer_high_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(stc_layer_high_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, s, partial, entropy, n);
    return wsu_check_launch("stc_layer_high_finish_kernel");
}

int wsu_stc_layer_low(const uint8_t* x_u8, const double* rho, const double* lambdas, const uint8_t* y1, const int32_t* k1, uint8_t* u0,
                      double* rho0, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && rho && lambdas && y1 && k1 && u0 && rho0, "stc_layer_low: null pointer");
    WSU_REQUIRE_SHAPE("stc_layer_low", WSU_PATH_PIXELS, "path");
    hipLaunchKernelGGL(stc_layer_low_kernel, dim3(SL_PARTS, n), dim3(256), 0, static_cast<hipStream_t>(stream), x_u8, rho, lambdas, y1, k1, u0,
                       rho0, (long long)h * w);
    return wsu_check_launch("stc_layer_low_kernel");
}

int wsu_stc_layer_compose(const uint8_t* cover, const double* rho, const uint8_t* y1, const uint8_t* y0, const int32_t* k1,
                          const uint8_t* ok1, const uint8_t* ok0, uint8_t* stego, long long* changes, double* distortion, uint8_t* ok,
                          void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(cover && rho && y1 && y0 && k1 && ok1 && ok0 && stego && changes && distortion && ok && workspace,
                "stc_layer_compose: null pointer");
    WSU_REQUIRE_SHAPE("stc_layer_compose", WSU_PATH_PIXELS, "path");
    WSU_REQUIRE(workspace_bytes >= wsu_stc_layer_workspace_bytes(n), "stc_layer_compose: workspace too small");
    WSU_REQUIRE((uintptr_t)workspace % 8 == 0, "stc_layer_compose: workspace must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* partial_d = static_cast<double*>(workspace);
    long long* partial_c = reinterpret_cast<long long*>(partial_d + (size_t)n * SL_PARTS);
    hipLaunchKernelGGL(stc_layer_compose_kernel, dim3(SL_PARTS, n), dim3(256), 0, s, cover, rho, y1, y0, k1, ok1, ok0, stego, partial_d, partial_c,
                       (long long)h * w);
    const int rc = wsu_check_launch("stc_layer_compose_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(stc_layer_compose_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, s, partial_d, partial_c, ok1, ok0, changes, distortion, ok,
                       n);
    return wsu_check_launch("stc_layer_compose_finish_kernel");
}

}  // extern "C"
