// K7p: the pieces of the PLANAR training path (mode F16F8P activations, gradients in the same three-plane layout with the gradient's
// residual scaling) that are not the matrix kernels themselves -- autograd of src/unet/model/unet.py:137-189 (loop pattern
// src/detector/train.py:55-95; oracle: oracle/unet_ref.py under torch.autograd):
//   * reflect-padding adjoint of the 3x3 data gradient: gather of the gradient's border rows / columns into strips, and the fold of the
//     strips' 1x3 convolutions (computed by conv3x3_pl_kernel<GRAD> with the ring weight sets) back onto rows 1, H-2 / columns 1, W-2
//   * max-pool backward (+ skip add + ReLU mask), head backward, per-channel sums, first-layer weight gradient
// Planar layout (include/wsu.h): [n][C/16][3 planes][H][W][16 B], planes = f16 ch 0-7 | f16 ch 8-15 | e4m3 residuals ch 0-15; activations
// scale the residual by 2^12, gradients by 2^14 (wsu_device.h).  Everything is deterministic (fixed-order reductions, no float atomics).
#include "wsu_device.h"

namespace {

__device__ __forceinline__ size_t pl_off(int n, int nch, int ch, int plane, size_t hw, size_t pix) {
    return ((((size_t)n * nch + ch) * 3 + plane) * hw + pix) * 16;
}

// 3 stored granules of one pixel -> 16 fp32 values (f16 part + e4m3 residual * lo_mul)
__device__ __forceinline__ void pl_decode16(const u32x4& h0, const u32x4& h1, const u32x4& lo, float lo_mul, float (&v)[16]) {
    const f16x8 a = __builtin_bit_cast(f16x8, h0), b = __builtin_bit_cast(f16x8, h1);
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] = (float)a[e]; v[8 + e] = (float)b[e]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int wd = (int)lo[k];
        v[4 * k + 0] += __builtin_amdgcn_cvt_f32_fp8(wd, 0) * lo_mul;
        v[4 * k + 1] += __builtin_amdgcn_cvt_f32_fp8(wd, 1) * lo_mul;
        v[4 * k + 2] += __builtin_amdgcn_cvt_f32_fp8(wd, 2) * lo_mul;
        v[4 * k + 3] += __builtin_amdgcn_cvt_f32_fp8(wd, 3) * lo_mul;
    }
}
__device__ __forceinline__ void pl_encode16(const float (&v)[16], float div_lo, u32x4& h0, u32x4& h1, u32x4& lo) {
    uint32_t h[8], l[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wsu_split4_f16r8(mk_f4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]), div_lo, h[2 * k], h[2 * k + 1], l[k]);
    h0 = mk_u4(h[0], h[1], h[2], h[3]); h1 = mk_u4(h[4], h[5], h[6], h[7]); lo = mk_u4(l[0], l[1], l[2], l[3]);
}
// 8 mask bits (stored f16 > 0) of one granule
__device__ __forceinline__ unsigned pl_pos_bits(const u32x4& g) {
    unsigned bits = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int wd = (int)g[e];
        bits |= ((short)(wd & 0xFFFF) > 0 ? 1u : 0u) << (2 * e);
        bits |= (wd >= 0x10000 ? 1u : 0u) << (2 * e + 1);
    }
    return bits;
}

// ---- ring strips: [4 sets: top, bottom, left, right][nch][3][n rows][L + 2][16 B]; data at columns 1..W (1..H), zeros elsewhere ----------
__global__ __launch_bounds__(256) void ring_gather_pl_kernel(const char* __restrict__ g, char* __restrict__ strips,
                                                             int n, int h, int w, int nch, int L) {
    const size_t hw = (size_t)h * w;
    const long long total = (long long)4 * nch * 3 * n * (L + 2);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long t = i;
        const int j = (int)(t % (L + 2)); t /= (L + 2);
        const int r = (int)(t % n); t /= n;
        const int plane = (int)(t % 3); t /= 3;
        const int ch = (int)(t % nch); const int set = (int)(t / nch);
        u32x4 v = mk_u4(0, 0, 0, 0);
        const int len = set < 2 ? w : h;
        if (j >= 1 && j <= len) {
            const int yy = set == 0 ? 0 : set == 1 ? h - 1 : j - 1;
            const int xx = set == 2 ? 0 : set == 3 ? w - 1 : j - 1;
            v = *reinterpret_cast<const u32x4*>(g + pl_off(r, nch, ch, plane, hw, (size_t)yy * w + xx));
        }
        *reinterpret_cast<u32x4*>(strips + (size_t)i * 16) = v;
    }
}

// so: the strips' conv outputs [4][nci][3][n][L + 2][16 B] (gradient encoding).  One thread per (image, ring pixel, 16-channel chunk).
__global__ __launch_bounds__(256) void ring_fold_pl_kernel(const char* __restrict__ so, char* __restrict__ dx1, char* __restrict__ dx2,
                                                           const char* __restrict__ mask1, const char* __restrict__ mask2,
                                                           int n, int h, int w, int nci, int nco1, int L, int gres) {
    // gres = 0 (products F16): gradient tensors carry no residual plane -- dx's is neither read nor written.  The strips' conv outputs are scratch of
    // this entry, not gradient tensors: they keep their residual plane in either case (a ring pixel is rounded to f16 by the main result and by the sum
    // stored here, not a third time in between)
    const u32x4 zres = mk_u4(0, 0, 0, 0);
    const int nrows = (h - 2 != 1) ? 2 : 1, ncols = (w - 2 != 1) ? 2 : 1;
    const int rlo = min(1, h - 2), rhi = max(1, h - 2);
    const int per_img = nrows * w + ncols * (h - nrows);
    const size_t hw = (size_t)h * w, shw = (size_t)n * (L + 2);
    const long long total = (long long)n * per_img * nci;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long t = i;
        int b = (int)(t % per_img); t /= per_img;
        const int ch = (int)(t % nci); const int img = (int)(t / nci);
        int y, x;
        if (b < nrows * w) { y = (b / w == 0) ? 1 : h - 2; x = b % w; }
        else {
            b -= nrows * w;
            int row = b / ncols;
            if (row >= rlo) ++row;
            if (nrows == 2 && row >= rhi) ++row;
            y = row; x = (b % ncols == 0) ? 1 : w - 2;
        }
        const bool d1 = ch < nco1;
        char* dx = d1 ? dx1 : dx2;
        const char* mk = d1 ? mask1 : mask2;
        const int ncd = d1 ? nco1 : nci - nco1, chd = d1 ? ch : ch - nco1;
        const size_t pix = (size_t)y * w + x;
        float v[16];
        pl_decode16(*reinterpret_cast<const u32x4*>(dx + pl_off(img, ncd, chd, 0, hw, pix)), *reinterpret_cast<const u32x4*>(dx + pl_off(img, ncd, chd, 1, hw, pix)),
                    gres ? *reinterpret_cast<const u32x4*>(dx + pl_off(img, ncd, chd, 2, hw, pix)) : zres, WSU_F8_GLO_DIV, v);
        float add[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) add[e] = 0.f;
        auto take = [&](int set, int col) {                                  // strips image `set`, row `img`, column `col`
            const size_t p = (size_t)img * (L + 2) + col;
            float s[16];
            pl_decode16(*reinterpret_cast<const u32x4*>(so + pl_off(set, nci, ch, 0, shw, p)), *reinterpret_cast<const u32x4*>(so + pl_off(set, nci, ch, 1, shw, p)),
                        *reinterpret_cast<const u32x4*>(so + pl_off(set, nci, ch, 2, shw, p)), WSU_F8_GLO_DIV, s);
#pragma unroll
            for (int e = 0; e < 16; ++e) add[e] += s[e];
        };
        // fixed order: top (centre, left corner, right corner), bottom (same), left, right
        if (y == 1)     { take(0, x + 1); if (x == 1) take(0, 0); if (x == w - 2) take(0, w + 1); }
        if (y == h - 2) { take(1, x + 1); if (x == 1) take(1, 0); if (x == w - 2) take(1, w + 1); }
        if (x == 1) take(2, y + 1);
        if (x == w - 2) take(3, y + 1);
        unsigned m0 = 0xFFu, m1 = 0xFFu;
        if (mk) {
            m0 = pl_pos_bits(*reinterpret_cast<const u32x4*>(mk + pl_off(img, ncd, chd, 0, hw, pix)));
            m1 = pl_pos_bits(*reinterpret_cast<const u32x4*>(mk + pl_off(img, ncd, chd, 1, hw, pix)));
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[e] += ((m0 >> e) & 1u) ? add[e] : 0.f;
            v[8 + e] += ((m1 >> e) & 1u) ? add[8 + e] : 0.f;
        }
        u32x4 h0, h1, lo;
        pl_encode16(v, WSU_F8_GLO_DIV, h0, h1, lo);
        *reinterpret_cast<u32x4*>(dx + pl_off(img, ncd, chd, 0, hw, pix)) = h0;
        *reinterpret_cast<u32x4*>(dx + pl_off(img, ncd, chd, 1, hw, pix)) = h1;
        if (gres) *reinterpret_cast<u32x4*>(dx + pl_off(img, ncd, chd, 2, hw, pix)) = lo;
    }
}

// 8 channels of one pixel: f16 granule + its 8 residual bytes -> fp32; and back
__device__ __forceinline__ void pl_decode8(const u32x4& h, const u32x2& r, float lo_mul, float (&v)[8]) {
    const int r0 = (int)r.x, r1 = (int)r.y;                  // value = residual * lo_mul + f16 part: one v_cvt_f32_fp8 + one v_fma_mix_f32 per value
    v[0] = wsu_fma_f16_lo(__builtin_amdgcn_cvt_f32_fp8(r0, 0), lo_mul, h.x); v[1] = wsu_fma_f16_hi(__builtin_amdgcn_cvt_f32_fp8(r0, 1), lo_mul, h.x);
    v[2] = wsu_fma_f16_lo(__builtin_amdgcn_cvt_f32_fp8(r0, 2), lo_mul, h.y); v[3] = wsu_fma_f16_hi(__builtin_amdgcn_cvt_f32_fp8(r0, 3), lo_mul, h.y);
    v[4] = wsu_fma_f16_lo(__builtin_amdgcn_cvt_f32_fp8(r1, 0), lo_mul, h.z); v[5] = wsu_fma_f16_hi(__builtin_amdgcn_cvt_f32_fp8(r1, 1), lo_mul, h.z);
    v[6] = wsu_fma_f16_lo(__builtin_amdgcn_cvt_f32_fp8(r1, 2), lo_mul, h.w); v[7] = wsu_fma_f16_hi(__builtin_amdgcn_cvt_f32_fp8(r1, 3), lo_mul, h.w);
}
__device__ __forceinline__ void pl_encode8(const float (&v)[8], float div_lo, u32x4& h, u32x2& r) {
    uint32_t h0, h1, h2, h3, l0, l1;
    wsu_split4_f16r8(mk_f4(v[0], v[1], v[2], v[3]), div_lo, h0, h1, l0);
    wsu_split4_f16r8(mk_f4(v[4], v[5], v[6], v[7]), div_lo, h2, h3, l1);
    h = mk_u4(h0, h1, h2, h3); r = mk_u2(l0, l1);
}
// addresses of the f16 granule / residual half of 8-channel group cg (of c channels) at pixel pix of image n
__device__ __forceinline__ const char* pl_h(const char* t, int n, int c, int cg, size_t hw, size_t pix) { return t + pl_off(n, c >> 4, cg >> 1, cg & 1, hw, pix); }
__device__ __forceinline__ const char* pl_r(const char* t, int n, int c, int cg, size_t hw, size_t pix) { return t + pl_off(n, c >> 4, cg >> 1, 2, hw, pix) + (cg & 1) * 8; }

// ---- 2x2 max-pool backward + skip add + ReLU mask (autograd of unet.py:143-149 with the skip connection of :178,184) -------------------------
// g[n, c, y, x] = (skip_g[n, c, y, x] + [ (y, x) is the first maximum of its window ] * dyp[n, c, y/2, x/2]) * (a[n, c, y, x] > 0), a = the
// stored activation the pool consumed.  One thread per (pooled pixel, 8-channel group); the argmax is recomputed from the stored values in the
// window order (0,0) (0,1) (1,0) (1,1) of nn.MaxPool2d.
__global__ __launch_bounds__(256) void pool_bwd_pl_kernel(const char* __restrict__ skip_g, const char* __restrict__ dyp, const char* __restrict__ act,
                                                          char* __restrict__ g, int n, int h, int w, int c, int gres) {
    // gres = 0 (products F16): the gradients' residual planes (skip_g, dyp, g) are neither read nor written; the activation is read whole
    const u32x2 zres = mk_u2(0, 0);
    const int hp = h >> 1, wp = w >> 1, ncg = c >> 3;
    const size_t hw = (size_t)h * w, hwp = (size_t)hp * wp;
    const long long total = (long long)n * ncg * hwp;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        // lane pairs = the two 8-channel groups of one 16-channel chunk at the same pixel: together they read / write whole 16-byte residual
        // granules (round 2 gave consecutive lanes consecutive pixels of ONE group: every residual access used 8 of 16 bytes, the other half
        // went to a workgroup far away in the grid)
        long long t = i;
        const int cgl = (int)(t & 1); t >>= 1;
        const int xp = (int)(t % wp); t /= wp;
        const int yp = (int)(t % hp); t /= hp;
        const int cg = (int)(t % (ncg >> 1)) * 2 + cgl; const int img = (int)(t / (ncg >> 1));
        float d[8];
        pl_decode8(*reinterpret_cast<const u32x4*>(pl_h(dyp, img, c, cg, hwp, (size_t)yp * wp + xp)),
                   gres ? *reinterpret_cast<const u32x2*>(pl_r(dyp, img, c, cg, hwp, (size_t)yp * wp + xp)) : zres, WSU_F8_GLO_DIV, d);
        float av[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t pix = (size_t)(2 * yp + (k >> 1)) * w + 2 * xp + (k & 1);
            pl_decode8(*reinterpret_cast<const u32x4*>(pl_h(act, img, c, cg, hw, pix)), *reinterpret_cast<const u32x2*>(pl_r(act, img, c, cg, hw, pix)), WSU_F8_XLO_DIV, av[k]);
        }
        int best[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int bi = 0; float bv = av[0][e];
#pragma unroll
            for (int k = 1; k < 4; ++k) if (av[k][e] > bv) { bv = av[k][e]; bi = k; }
            best[e] = bi;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t pix = (size_t)(2 * yp + (k >> 1)) * w + 2 * xp + (k & 1);
            float v[8];
            if (skip_g) pl_decode8(*reinterpret_cast<const u32x4*>(pl_h(skip_g, img, c, cg, hw, pix)), gres ? *reinterpret_cast<const u32x2*>(pl_r(skip_g, img, c, cg, hw, pix)) : zres, WSU_F8_GLO_DIV, v);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = 0.f;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (best[e] == k) v[e] += d[e];
                if (!(av[k][e] > 0.f)) v[e] = 0.f;
            }
            u32x4 hq; u32x2 rq;
            pl_encode8(v, WSU_F8_GLO_DIV, hq, rq);
            *reinterpret_cast<u32x4*>(const_cast<char*>(pl_h(g, img, c, cg, hw, pix))) = hq;
            if (gres) *reinterpret_cast<u32x2*>(const_cast<char*>(pl_r(g, img, c, cg, hw, pix))) = rq;
        }
    }
}

// ---- 1x1 head + sigmoid backward (autograd of unet.py:186-188): dz = dout * out * (1 - out);  g[c] = (sum_o w[o][c] dz[o]) * (x[c] > 0);
// dW[o][c] = sum_px dz[o] x[c];  db[o] = sum_px dz[o].  Thread = (pixel lane, 8-channel group); per-block partials, fixed-order reduction. --------
constexpr int HEADP_MAXCO = 4;
// NCO = output planes compiled in (1: the reference's single plane -- 48 registers of weights / weight-gradient sums fewer than the 4-plane
// form, which sat at 144 registers = 3 waves per SIMD for a streaming kernel; 4: 2..4 planes)
template <int NCO>
__global__ __launch_bounds__(256) void head_bwd_pl_kernel(const char* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ out,
                                                          const float* __restrict__ dout, char* __restrict__ g, float* __restrict__ part,
                                                          int n, int hw_, int wrow, int c, int cout, int gres) {
    const int ncg = c >> 3;                                   // 8 for the reference's 64 channels
    const int ppb = 256 / ncg;                                // pixels per block pass
    const int cg = threadIdx.x / ppb, pl = threadIdx.x % ppb;
    const size_t hw = (size_t)hw_;
    float wv[NCO][8], aw[NCO][8], ab[NCO];
#pragma unroll
    for (int o = 0; o < NCO; ++o) {
        ab[o] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { wv[o][e] = o < cout ? wgt[(size_t)o * c + cg * 8 + e] : 0.f; aw[o][e] = 0.f; }
    }
    // (a block walks rows of `wrow` pixels -- wrow divides the plane, the launcher passes the image width -- so that image and pixel come from one
    // 32-bit division per row instead of two 64-bit ones per pixel)
    const int rows_per_img = (int)(hw / wrow), rows = n * rows_per_img;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
      const int img = row / rows_per_img;
      const size_t rowpix = (size_t)(row - img * rows_per_img) * wrow;
      for (int col = pl; col < wrow; col += ppb) {
        const size_t pix = rowpix + col;
        float xv[8], gv[8];
        pl_decode8(*reinterpret_cast<const u32x4*>(pl_h(x, img, c, cg, hw, pix)), *reinterpret_cast<const u32x2*>(pl_r(x, img, c, cg, hw, pix)), WSU_F8_XLO_DIV, xv);
#pragma unroll
        for (int e = 0; e < 8; ++e) gv[e] = 0.f;
#pragma unroll
        for (int o = 0; o < NCO; ++o)
            if (o < cout) {
                const size_t oi = ((size_t)img * cout + o) * hw + pix;
                const float ov = out[oi];
                const float dz = dout[oi] * ov * (1.f - ov);
                ab[o] += dz;
#pragma unroll
                for (int e = 0; e < 8; ++e) { gv[e] = fmaf(wv[o][e], dz, gv[e]); aw[o][e] = fmaf(xv[e], dz, aw[o][e]); }
            }
#pragma unroll
        for (int e = 0; e < 8; ++e) if (!(xv[e] > 0.f)) gv[e] = 0.f;
        u32x4 hq; u32x2 rq;
        pl_encode8(gv, WSU_F8_GLO_DIV, hq, rq);
        *reinterpret_cast<u32x4*>(const_cast<char*>(pl_h(g, img, c, cg, hw, pix))) = hq;
        if (gres) *reinterpret_cast<u32x2*>(const_cast<char*>(pl_r(g, img, c, cg, hw, pix))) = rq;      // (products F16: no residual plane)
      }
    }
    // block partial: part[block][o][c + 1]
    __shared__ float red[256 * 9];
    for (int o = 0; o < cout; ++o) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) red[threadIdx.x * 9 + e] = aw[o][e];
        red[threadIdx.x * 9 + 8] = ab[o];
        __syncthreads();
        if (pl == 0) {
            float sacc[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) sacc[e] = 0.f;
            for (int k = 0; k < ppb; ++k)
#pragma unroll
                for (int e = 0; e < 9; ++e) sacc[e] += red[(cg * ppb + k) * 9 + e];
            float* dst = part + ((size_t)blockIdx.x * cout + o) * (c + 1);
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[cg * 8 + e] = sacc[e];
            if (cg == 0) dst[c] = sacc[8];
        }
    }
}
// one WAVE per output: lane-strided partial sums + a butterfly -- a fixed order (deterministic); one thread per output walked the block
// partials serially: 0.28 ms for 65 sums at batch 64
__global__ __launch_bounds__(256) void head_bwd_pl_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int nblocks, int c, int cout) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= cout * (c + 1)) return;                           // wave-uniform
    float s = 0.f;
    for (int b = lane; b < nblocks; b += 64) s += part[(size_t)b * cout * (c + 1) + i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    const int o = i / (c + 1), k = i % (c + 1);
    if (lane == 0) { if (k < c) dw[(size_t)o * c + k] = s; else db[o] = s; }
}

// ---- per-channel sums of a planar gradient (bias gradient of the transposed conv) and the first layer's weight gradient (single input plane:
// dW[co][tap] = sum_px g[co][px] * img[reflect(px + tap)], db[co] = sum_px g[co][px]; unet.py:82,141).  Thread = (pixel lane, 8-channel group);
// block partials [block][c][NV], reduced in block order. ----------------------------------------------------------------------------------------
template <bool FIRST>
__global__ __launch_bounds__(256) void chansum_pl_kernel(const char* __restrict__ g, const float* __restrict__ img, float* __restrict__ part,
                                                         int n, int h, int w, int c, int gres) {
    constexpr int NV = FIRST ? 10 : 1;                        // 9 taps + bias | the plain sum
    const int ncg = c >> 3, ppb = 256 / ncg;
    const int cg = threadIdx.x / ppb, pl = threadIdx.x % ppb;
    const size_t hw = (size_t)h * w;
    float acc[NV][8];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
    // a block walks image ROWS (one 32-bit division per row; the pixel loop adds): as a flat pixel loop the four 64-bit divisions per pixel (image, pixel,
    // row, column) made this streaming kernel VALU-bound -- 1.03 ms for the first layer's 2.1 GB gradient at batch 64 (2.1 TB/s)
    const int rows = n * h;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int im = row / h, y = row - im * h;
        const size_t rowpix = (size_t)y * w;
        [[maybe_unused]] const float* src = FIRST ? img + (size_t)im * hw : nullptr;
        [[maybe_unused]] const int ro[3] = {wsu_reflect(y - 1, h) * w, y * w, wsu_reflect(y + 1, h) * w};
        for (int x = pl; x < w; x += ppb) {
            float gv[8];
            pl_decode8(*reinterpret_cast<const u32x4*>(pl_h(g, im, c, cg, hw, rowpix + x)), gres ? *reinterpret_cast<const u32x2*>(pl_r(g, im, c, cg, hw, rowpix + x)) : mk_u2(0, 0), WSU_F8_GLO_DIV, gv);
            if constexpr (FIRST) {
                const int co[3] = {wsu_reflect(x - 1, w), x, wsu_reflect(x + 1, w)};
#pragma unroll
                for (int tp = 0; tp < 9; ++tp) {
                    const float iv = src[ro[tp / 3] + co[tp % 3]];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[tp][e] = fmaf(gv[e], iv, acc[tp][e]);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[9][e] += gv[e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[0][e] += gv[e];
            }
        }
    }
    __shared__ float red[256 * 8];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) red[threadIdx.x * 8 + e] = acc[k][e];
        __syncthreads();
        if (pl == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float sacc = 0.f;
                for (int j = 0; j < ppb; ++j) sacc += red[(cg * ppb + j) * 8 + e];
                part[((size_t)blockIdx.x * c + cg * 8 + e) * NV + k] = sacc;
            }
        }
    }
}
// out[i] = sum over blocks of part[b][i], i < count: one wave per output, lane-strided partial sums + a butterfly (a fixed order: deterministic)
__global__ __launch_bounds__(256) void block_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int nblocks, int count) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= count) return;                                   // wave-uniform
    float sacc = 0.f;
    for (int b = lane; b < nblocks; b += 64) sacc += part[(size_t)b * count + i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sacc += __shfl_xor(sacc, m);
    if (lane == 0) out[i] = sacc;
}
// first layer: [c][10] sums -> dw (c, 1, 3, 3), db (c)
// K7p (round 4): data gradient of the first layer from a PLANAR gradient -- the input gradient of the planar training path (saliency,
// src/saliency.py:159-174; VERDICT r03 missing #4: a default-mode model used to switch to the fp32-storage kernels for this call).
// dx[n,ci,y,x] = sum over the padded positions that reflect onto (y,x) of sum_{u,v,co} W[co,ci,u,v] * g[n, yp-u+1, xp-v+1, co] (g zero outside the
// image): one thread per input element, consecutive lanes = consecutive pixels of a row (16 contiguous bytes per lane and plane), weights as
// [tap][co] in LDS, fp32 accumulation in a fixed order.  `gres` = 0: the gradient carries no residual plane (products F16).
__global__ __launch_bounds__(256) void first_dgrad_pl_kernel(const char* __restrict__ g, const float* __restrict__ w, float* __restrict__ dx,
                                                             int n, int h, int wd, int cin, int c, int gres) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* wl = reinterpret_cast<float*>(smem);                 // [ci][tap][co]
    for (int i = threadIdx.x; i < cin * 9 * c; i += blockDim.x) {
        const int co = i % c, tap = (i / c) % 9, ci = i / (9 * c);
        wl[i] = w[((size_t)co * cin + ci) * 9 + tap];
    }
    __syncthreads();
    const size_t hw = (size_t)h * wd;
    const int nch = c >> 4;
    const long long total = (long long)n * cin * hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % wd); long long t = i / wd;
        const int y = (int)(t % h); t /= h;
        const int ci = (int)(t % cin); const int img = (int)(t / cin);
        int ys[3], xs[3]; int ny = 0, nx = 0;
        ys[ny++] = y; if (y == 1) ys[ny++] = -1; if (y == h - 2) ys[ny++] = h;
        xs[nx++] = x; if (x == 1) xs[nx++] = -1; if (x == wd - 2) xs[nx++] = wd;
        float acc = 0.f;
        for (int iy = 0; iy < ny; ++iy)
            for (int ix = 0; ix < nx; ++ix)
                for (int u = 0; u < 3; ++u) {
                    const int sy = ys[iy] - u + 1;
                    if (sy < 0 || sy >= h) continue;
                    for (int v = 0; v < 3; ++v) {
                        const int sx = xs[ix] - v + 1;
                        if (sx < 0 || sx >= wd) continue;
                        const size_t pix = (size_t)sy * wd + sx;
                        const float* wp = wl + (ci * 9 + u * 3 + v) * c;
                        float s_ = 0.f;
                        for (int ch = 0; ch < nch; ++ch) {
                            float gv[16];
                            pl_decode16(*reinterpret_cast<const u32x4*>(g + pl_off(img, nch, ch, 0, hw, pix)), *reinterpret_cast<const u32x4*>(g + pl_off(img, nch, ch, 1, hw, pix)),
                                        gres ? *reinterpret_cast<const u32x4*>(g + pl_off(img, nch, ch, 2, hw, pix)) : mk_u4(0, 0, 0, 0), WSU_F8_GLO_DIV, gv);
#pragma unroll
                            for (int e = 0; e < 16; ++e) s_ = fmaf(gv[e], wp[ch * 16 + e], s_);
                        }
                        acc += s_;
                    }
                }
        dx[i] = acc;
    }
}

__global__ void first_split_kernel(const float* __restrict__ sums, float* __restrict__ dw, float* __restrict__ db, int c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c * 10) return;
    const int co = i / 10, k = i % 10;
    if (k < 9) dw[co * 9 + k] = sums[i]; else if (db) db[co] = sums[i];
}

// The first layer's weight gradient for cin <= 8 input planes (side-information planes behind the image, data/pairs.py): chansum_pl_kernel<true>'s
// scheme with 9 sums per plane.  One launch takes NP <= 4 planes from p0 on (and the bias sum if BIAS): 9 * NP + 1 accumulators per channel, 8
// channels per thread -- 296 registers for NP = 4.  All 8 planes in one launch would need 584, beyond the 512 a wave can hold (the build reports
// scratch for it), so cin > 4 takes a second launch and reads g twice.  Block partials [block][c][9 * cin + 1], column ci * 9 + tap, bias last.
template <int NP, bool BIAS>
__global__ __launch_bounds__(256) void first_planes_wgrad_kernel(const char* __restrict__ g, const float* __restrict__ x, float* __restrict__ part,
                                                                 int n, int h, int w, int cin, int p0, int c, int gres) {
    constexpr int NV = 9 * NP + (BIAS ? 1 : 0);
    const int nvt = 9 * cin + 1;
    const int ncg = c >> 3, ppb = 256 / ncg;
    const int cg = threadIdx.x / ppb, pl = threadIdx.x % ppb;
    const size_t hw = (size_t)h * w;
    float acc[NV][8];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
    const int rows = n * h;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int im = row / h, y = row - im * h;
        const size_t rowpix = (size_t)y * w;
        const float* src = x + ((size_t)im * cin + p0) * hw;
        const int ro[3] = {wsu_reflect(y - 1, h) * w, y * w, wsu_reflect(y + 1, h) * w};
        for (int xx = pl; xx < w; xx += ppb) {
            float gv[8];
            pl_decode8(*reinterpret_cast<const u32x4*>(pl_h(g, im, c, cg, hw, rowpix + xx)), gres ? *reinterpret_cast<const u32x2*>(pl_r(g, im, c, cg, hw, rowpix + xx)) : mk_u2(0, 0), WSU_F8_GLO_DIV, gv);
            const int co[3] = {wsu_reflect(xx - 1, w), xx, wsu_reflect(xx + 1, w)};
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int tp = 0; tp < 9; ++tp) {
                    const float iv = src[p * hw + ro[tp / 3] + co[tp % 3]];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[p * 9 + tp][e] = fmaf(gv[e], iv, acc[p * 9 + tp][e]);
                }
            if constexpr (BIAS) {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[9 * NP][e] += gv[e];
            }
        }
    }
    __shared__ float red[256 * 8];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) red[threadIdx.x * 8 + e] = acc[k][e];
        __syncthreads();
        if (pl == 0) {
            const int col = k < 9 * NP ? p0 * 9 + k : 9 * cin;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float sacc = 0.f;
                for (int j = 0; j < ppb; ++j) sacc += red[(cg * ppb + j) * 8 + e];
                part[((size_t)blockIdx.x * c + cg * 8 + e) * nvt + col] = sacc;
            }
        }
    }
}
// [c][9 * cin + 1] sums -> dw (c, cin, 3, 3), db (c)
__global__ void first_planes_split_kernel(const float* __restrict__ sums, float* __restrict__ dw, float* __restrict__ db, int c, int cin) {
    const int nvt = 9 * cin + 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c * nvt) return;
    const int co = i / nvt, k = i % nvt;
    if (k < 9 * cin) dw[co * 9 * cin + k] = sums[i]; else if (db) db[co] = sums[i];
}

constexpr int SUM_BLOCKS = 2048;                             // ~8 workgroups per CU: these kernels stream (2 - 3 loads in flight per thread), occupancy is their memory parallelism

inline unsigned grid_for(long long total) { return (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192); }

}  // namespace

// internal (conv3x3_pl.hip): the two thin kernels around the strips' conv
WSU_INTERNAL int wsu_ring_gather_pl(const void* g, void* strips, int n, int h, int w, int c, int L, void* stream) {
    const long long total = (long long)4 * (c / 16) * 3 * n * (L + 2);
    hipLaunchKernelGGL(ring_gather_pl_kernel, dim3(grid_for(total)), dim3(256), 0, static_cast<hipStream_t>(stream), (const char*)g, (char*)strips, n, h, w, c / 16, L);
    return wsu_check_launch("ring_gather_pl_kernel");
}
WSU_INTERNAL int wsu_ring_fold_pl(const void* strips_out, void* dx1, void* dx2, const void* mask1, const void* mask2,
                                int n, int h, int w, int cin, int csplit, int L, int gres, void* stream) {
    const int nrows = (h - 2 != 1) ? 2 : 1, ncols = (w - 2 != 1) ? 2 : 1;
    const long long total = (long long)n * (nrows * w + ncols * (h - nrows)) * (cin / 16);
    hipLaunchKernelGGL(ring_fold_pl_kernel, dim3(grid_for(total)), dim3(256), 0, static_cast<hipStream_t>(stream), (const char*)strips_out, (char*)dx1, (char*)dx2,
                       (const char*)mask1, (const char*)mask2, n, h, w, cin / 16, csplit / 16, L, gres);
    return wsu_check_launch("ring_fold_pl_kernel");
}

extern "C" {

// K7p: g = (skip_g + max-pool routing of dy_pool) * (act > 0) on planar tensors (layout: wsu.h): skip_g (optional), g at (h, w); dy_pool at (h/2, w/2);
// act = the stored activation the pool consumed (c channels, multiple of 16; h, w even).  g may alias skip_g.
int wsu_maxpool2x2_pl_bwd(const void* skip_g, const void* dy_pool, const void* act, void* g, int n, int h, int w, int c, int products, void* stream) {
    WSU_REQUIRE(dy_pool && act && g, "maxpool2x2_pl_bwd: null pointer");
    WSU_REQUIRE(products == WSU_PRODUCTS_F16F8 || products == WSU_PRODUCTS_F16, "maxpool2x2_pl_bwd: products must be WSU_PRODUCTS_F16F8 or WSU_PRODUCTS_F16");
    WSU_REQUIRE(n > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0 && c > 0 && c % 16 == 0, "maxpool2x2_pl_bwd: bad shape");
    const long long total = (long long)n * (c / 8) * (h / 2) * (w / 2);
    hipLaunchKernelGGL(pool_bwd_pl_kernel, dim3(grid_for(total)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       (const char*)skip_g, (const char*)dy_pool, (const char*)act, (char*)g, n, h, w, c, products == WSU_PRODUCTS_F16 ? 0 : 1);
    return wsu_check_launch("pool_bwd_pl_kernel");
}

size_t wsu_head_pl_bwd_workspace_bytes(int c, int cout) { return (size_t)SUM_BLOCKS * cout * (c + 1) * sizeof(float); }

// K7p: backward of the 1x1 head + sigmoid: x (planar activation, c channels = the head's input, c in {16, 32, 64, 128}), w (cout, c), out / dout
// (N, cout, H, W) fp32 (dout pre-scaled like every planar gradient), cout <= 4 -> g (planar gradient w.r.t. the PRE-activation of the layer that produced x:
// its ReLU mask is applied), dw (cout, c), db (cout).
int wsu_conv1x1_sigmoid_pl_bwd(const void* x, const float* w, const float* out, const float* dout, void* g, float* dw, float* db,
                               float* workspace, size_t workspace_bytes, int n, int h, int wd, int c, int cout, int products, void* stream) {
    WSU_REQUIRE(x && w && out && dout && g && dw && db && workspace, "conv1x1_sigmoid_pl_bwd: null pointer");
    WSU_REQUIRE(products == WSU_PRODUCTS_F16F8 || products == WSU_PRODUCTS_F16, "conv1x1_sigmoid_pl_bwd: products must be WSU_PRODUCTS_F16F8 or WSU_PRODUCTS_F16");
    const int gres = products == WSU_PRODUCTS_F16 ? 0 : 1;
    WSU_REQUIRE(n > 0 && h > 0 && wd > 0 && c >= 16 && c <= 128 && (c & (c - 1)) == 0 && cout >= 1 && cout <= HEADP_MAXCO, "conv1x1_sigmoid_pl_bwd: bad shape c=%d cout=%d", c, cout);
    WSU_REQUIRE(workspace_bytes >= wsu_head_pl_bwd_workspace_bytes(c, cout), "conv1x1_sigmoid_pl_bwd: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = (long long)n * h < SUM_BLOCKS ? n * h : SUM_BLOCKS;      // a block walks image rows
    if (cout == 1) hipLaunchKernelGGL(head_bwd_pl_kernel<1>, dim3(nblk), dim3(256), 0, s, (const char*)x, w, out, dout, (char*)g, workspace, n, h * wd, wd, c, cout, gres);
    else hipLaunchKernelGGL(head_bwd_pl_kernel<HEADP_MAXCO>, dim3(nblk), dim3(256), 0, s, (const char*)x, w, out, dout, (char*)g, workspace, n, h * wd, wd, c, cout, gres);
    int rc = wsu_check_launch("head_bwd_pl_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(head_bwd_pl_reduce_kernel, dim3((cout * (c + 1) + 3) / 4), dim3(256), 0, s, workspace, dw, db, nblk, c, cout);
    return wsu_check_launch("head_bwd_pl_reduce_kernel");
}

size_t wsu_chansum_pl_workspace_bytes(int c) { return (size_t)(SUM_BLOCKS + 1) * c * 10 * sizeof(float); }

// K7p: db[c] = per-channel sum of a planar gradient (bias gradient of the transposed conv), c in {16, 32, 64, ..., 2048}
int wsu_colsum_pl(const void* g, float* db, float* workspace, size_t workspace_bytes, int n, int h, int w, int c, int products, void* stream) {
    WSU_REQUIRE(g && db && workspace, "colsum_pl: null pointer");
    WSU_REQUIRE(products == WSU_PRODUCTS_F16F8 || products == WSU_PRODUCTS_F16, "colsum_pl: products must be WSU_PRODUCTS_F16F8 or WSU_PRODUCTS_F16");
    WSU_REQUIRE(n > 0 && h > 0 && w > 0 && c >= 16 && c <= 2048 && c % 16 == 0 && 256 % (c / 8) == 0, "colsum_pl: bad shape (c=%d must be 16..2048 with 256 %% (c / 8) == 0)", c);
    WSU_REQUIRE(workspace_bytes >= wsu_chansum_pl_workspace_bytes(c), "colsum_pl: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = (long long)n * h < SUM_BLOCKS ? n * h : SUM_BLOCKS;      // a block walks image rows
    hipLaunchKernelGGL(chansum_pl_kernel<false>, dim3(nblk), dim3(256), 0, s, (const char*)g, (const float*)nullptr, workspace, n, h, w, c, products == WSU_PRODUCTS_F16 ? 0 : 1);
    int rc = wsu_check_launch("chansum_pl_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(block_sum_kernel, dim3((c + 3) / 4), dim3(256), 0, s, workspace, db, nblk, c);
    return wsu_check_launch("block_sum_kernel");
}

// K7p: weight / bias gradient of the first layer for a single input plane: g (planar gradient, c channels), img (N, 1, H, W) fp32 -> dw (c, 1, 3, 3), db (c) or NULL
int wsu_conv3x3_first_pl_bwd_weight(const void* g, const float* img, float* dw, float* db, float* workspace, size_t workspace_bytes,
                                    int n, int h, int w, int c, int products, void* stream) {
    WSU_REQUIRE(g && img && dw && workspace, "conv3x3_first_pl_bwd_weight: null pointer");
    WSU_REQUIRE(products == WSU_PRODUCTS_F16F8 || products == WSU_PRODUCTS_F16, "conv3x3_first_pl_bwd_weight: products must be WSU_PRODUCTS_F16F8 or WSU_PRODUCTS_F16");
    WSU_REQUIRE(n > 0 && h >= 2 && w >= 2 && c >= 16 && c <= 256 && c % 16 == 0 && 256 % (c / 8) == 0, "conv3x3_first_pl_bwd_weight: bad shape c=%d", c);
    WSU_REQUIRE(workspace_bytes >= wsu_chansum_pl_workspace_bytes(c), "conv3x3_first_pl_bwd_weight: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = (long long)n * h < SUM_BLOCKS ? n * h : SUM_BLOCKS;      // a block walks image rows
    float* sums = workspace + (size_t)SUM_BLOCKS * c * 10;
    hipLaunchKernelGGL(chansum_pl_kernel<true>, dim3(nblk), dim3(256), 0, s, (const char*)g, img, workspace, n, h, w, c, products == WSU_PRODUCTS_F16 ? 0 : 1);
    int rc = wsu_check_launch("chansum_pl_kernel<first>");
    if (rc) return rc;
    hipLaunchKernelGGL(block_sum_kernel, dim3((c * 10 + 3) / 4), dim3(256), 0, s, workspace, sums, nblk, c * 10);
    rc = wsu_check_launch("block_sum_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(first_split_kernel, dim3((c * 10 + 63) / 64), dim3(64), 0, s, (const float*)sums, dw, db, c);
    return wsu_check_launch("first_split_kernel");
}

size_t wsu_conv3x3_first_pl_bwd_weight_planes_workspace_bytes(int cin, int c) {
    if (cin < 1 || c < 1) return 0;
    return (size_t)(SUM_BLOCKS + 1) * c * (9 * cin + 1) * sizeof(float);
}

// K7p: weight / bias gradient of the first layer for cin <= 8 input planes: g (planar gradient, c channels), x_nchw (N, cin, H, W) fp32 ->
// dw (c, cin, 3, 3), db (c) or NULL.  Planes 0-3 (and the bias sum) in one launch, planes 4-7 in a second; block partials summed in block order.
int wsu_conv3x3_first_pl_bwd_weight_planes(const void* g, const float* x_nchw, float* dw, float* db, float* workspace, size_t workspace_bytes,
                                           int n, int h, int w, int cin, int c, int products, void* stream) {
    WSU_REQUIRE(g && x_nchw && dw && workspace, "conv3x3_first_pl_bwd_weight_planes: null pointer");
    WSU_REQUIRE(products == WSU_PRODUCTS_F16F8 || products == WSU_PRODUCTS_F16, "conv3x3_first_pl_bwd_weight_planes: products must be WSU_PRODUCTS_F16F8 or WSU_PRODUCTS_F16");
    WSU_REQUIRE(n > 0 && h >= 2 && w >= 2 && cin >= 1 && cin <= 8 && c >= 16 && c <= 256 && c % 16 == 0 && 256 % (c / 8) == 0,
                "conv3x3_first_pl_bwd_weight_planes: bad shape cin=%d c=%d", cin, c);
    WSU_REQUIRE((long long)n * h <= 0x7FFFFFFFll, "conv3x3_first_pl_bwd_weight_planes: %lld rows exceed the row index", (long long)n * h);
    WSU_REQUIRE(workspace_bytes >= wsu_conv3x3_first_pl_bwd_weight_planes_workspace_bytes(cin, c), "conv3x3_first_pl_bwd_weight_planes: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = (long long)n * h < SUM_BLOCKS ? n * h : SUM_BLOCKS;      // a block walks image rows
    const int nvt = 9 * cin + 1, gres = products == WSU_PRODUCTS_F16 ? 0 : 1;
    float* sums = workspace + (size_t)SUM_BLOCKS * c * nvt;
    for (int p0 = 0; p0 < cin; p0 += 4) {
        const int np = cin - p0 < 4 ? cin - p0 : 4;
#define WSU_FIRST_PLANES(NP, BIAS) hipLaunchKernelGGL((first_planes_wgrad_kernel<NP, BIAS>), dim3(nblk), dim3(256), 0, s, (const char*)g, x_nchw, workspace, n, h, w, cin, p0, c, gres)
        if (p0 == 0) { if (np == 1) WSU_FIRST_PLANES(1, true); else if (np == 2) WSU_FIRST_PLANES(2, true); else if (np == 3) WSU_FIRST_PLANES(3, true); else WSU_FIRST_PLANES(4, true); }
        else { if (np == 1) WSU_FIRST_PLANES(1, false); else if (np == 2) WSU_FIRST_PLANES(2, false); else if (np == 3) WSU_FIRST_PLANES(3, false); else WSU_FIRST_PLANES(4, false); }
#undef WSU_FIRST_PLANES
        const int rc = wsu_check_launch("first_planes_wgrad_kernel");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(block_sum_kernel, dim3((c * nvt + 3) / 4), dim3(256), 0, s, workspace, sums, nblk, c * nvt);
    int rc = wsu_check_launch("block_sum_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(first_planes_split_kernel, dim3((c * nvt + 63) / 64), dim3(64), 0, s, (const float*)sums, dw, db, c, cin);
    return wsu_check_launch("first_planes_split_kernel");
}

// K7p: data gradient of the first layer: g (planar gradient, c channels at h x w), w_oihw (c, cin, 3, 3) fp32 -> dx (N, cin, H, W) fp32 (in g's scale).
int wsu_conv3x3_first_pl_bwd_data(const void* g, const float* w_oihw, float* dx_nchw, int n, int h, int w, int cin, int c, int products, void* stream) {
    WSU_REQUIRE(g && w_oihw && dx_nchw, "conv3x3_first_pl_bwd_data: null pointer");
    WSU_REQUIRE(products == WSU_PRODUCTS_F16F8 || products == WSU_PRODUCTS_F16, "conv3x3_first_pl_bwd_data: products must be WSU_PRODUCTS_F16F8 or WSU_PRODUCTS_F16");
    WSU_REQUIRE(n > 0 && h >= 2 && w >= 2 && cin >= 1 && cin <= 8 && c >= 16 && c <= 256 && c % 16 == 0, "conv3x3_first_pl_bwd_data: bad shape cin=%d c=%d", cin, c);
    const long long total = (long long)n * cin * h * w;
    const unsigned nblk = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    static bool attr_done = false;                            // cin = 8, c = 256: 73 728 B of weights, above the 64 KB a kernel gets unasked
    if (!attr_done) {
        if (int rc = wsu_raise_lds(first_dgrad_pl_kernel, 8 * 9 * 256 * (int)sizeof(float), "first_dgrad_pl")) return rc;
        attr_done = true;
    }
    hipLaunchKernelGGL(first_dgrad_pl_kernel, dim3(nblk), dim3(256), (size_t)cin * 9 * c * sizeof(float), static_cast<hipStream_t>(stream),
                       (const char*)g, w_oihw, dx_nchw, n, h, w, cin, c, products == WSU_PRODUCTS_F16 ? 0 : 1);
    return wsu_check_launch("first_dgrad_pl_kernel");
}

}  // extern "C"
