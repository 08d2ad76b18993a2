// K31 / K32: the JPEG history of a bitmap (R. Boehme, "Weighted stego-image steganalysis for JPEG covers", IH 2008): the residual energy of
// an image against a set of quantisation tables, and the image after a round trip through one table -- the WS predictor for covers that
// were a JPEG once.  Not part of the reference.  DESIGN.md 4-jpeg has the arithmetic; tests/jpeg_np.py restates it in numpy int64.
//
//   C[k][n] = rint(2^13 c_k cos((2n+1) k pi / 16)) (JH_C);  blocks of 8 x 8 on the grid at the plane's origin;  X = pixels - 128
//   Y  = C X C^T                       exact integers at scale 2^26, |Y| < 2^37; the first product fits 32 bits
//   k  = sign(Y) ((|Y| + D/2) // D)    D = Q 2^26, Q in 1..255: rounds half away from zero
//   K31  r = Y - k D;  r' = (r + 2^15) >> 16 (arithmetic);  E[image][table] = sum r'^2 over the image's coefficients (int64)
//   K32  Z = C^T (k Q) C + 128 2^26;  x_hat = float32(clamp(Z, 0, 255 2^26) / 2^26);  u8 = clamp((Z + 2^25) >> 26, 0, 255)
//
// One workgroup owns JH_SLOTS consecutive blocks of one image.  Thread (slot, r) transforms row r of its block (32-bit sums, C as
// immediates) into LDS; thread (slot, u) then forms the eight coefficients Y[u][0..7] of its block with 64-bit multiply-adds and keeps them
// in registers while the tables pass.
//
// K31 per coefficient and table, in 32 bits.  With a = |Y| = ah 2^26 + al, hb = al >> 25 and t = (2 ah + hb + Q) >> 1:
//     (a + D/2) // D = ((a + Q 2^25) >> 26) // Q = t // Q                  (a floor of a floor), t < 2^12
//     r' = S (ah - k Q) + lo,  S = +-1024 with Y's sign,  lo = (al + 2^15) >> 16 for Y >= 0, (2^15 - al) >> 16 for Y < 0
//          (the part of r above bit 26 is a multiple of 2^16, so the shift splits)
//   t // Q is int(float(t) * (1.f / Q) + 0.002f): float(t) is exact, the product is within 2^-10 of t / Q, and the fractional part of
//   t / Q is 0 or lies in [1/255, 254/255], so the truncation is the quotient (tests/test_jpeg_host.py walks every t and Q).  A thread
//   keeps (2 ah + hb, S ah + lo, S) per coefficient, JH_B blocks deep, so that a table's Q and 1 / Q are read from LDS once per JH_B
//   blocks; a table's sum leaves through the wave fold and the flush of the count kernels (wsu_count.h), in 64 bits.  The tables travel
//   as a kernel argument, JH_TCH at a launch (a launch per JH_TCH tables, each repeating the transform: 64 multiply-adds per thread
//   against ~300 operations per table).
// K32 quantises with the image's own table, transforms back through LDS (32-bit first pass) and writes a row of eight pixels per
//   thread.  An image with use = 0 gets the KB prediction in K11's float32 operation sequence (ws_pixel_terms: conv of u / 255.f, summed
//   K00 .. K22, times 255.f) on its interior and the pixel itself on its border, so that the statistic of such an image has the bits of
//   the KB filter's row.
#pragma clang fp contract(off)
#include "wsu_count.h"
#include "wsu_metric.h"

namespace {

constexpr int JH_THREADS = 256, JH_B = 4, JH_SLOTS = JH_THREADS / 8 * JH_B, JH_TS = 68, JH_TCH = 32, JH_WAVES = JH_THREADS / 64;
// C: immediates where the index is a constant, a table in memory where it is not
__device__ constexpr int JH_C[8][8] = {
    {2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},
    {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
    {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},
    {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
    {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},
    {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
    {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},
    {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// up to JH_TCH tables (K31: of one launch; K32: of the launch's images, with their `use` bits), a kernel argument
struct JhTables {
    uint8_t q[JH_TCH][64];
    uint32_t use;
};

// eight pixels from an 8-byte aligned address
__device__ __forceinline__ void jh_load8(const uint8_t* __restrict__ p, int (&px)[8]) {
    const u32x2 v = *reinterpret_cast<const u32x2*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) px[i] = (int)((v[i >> 2] >> (8 * (i & 3))) & 255u);
}

// where block b of a plane with bw blocks per row begins
__device__ __forceinline__ size_t jh_block_origin(long long b, int bw, int w) { return (size_t)(b / bw) * 8 * w + (size_t)(b % bw) * 8; }

// The forward transform of the workgroup's blocks b0 .. b0 + JH_SLOTS - 1 (those below `blocks`; the others transform as zeros, whose
// coefficients add nothing to any sum): afterwards thread (slot j * 32 + tid / 8, u = tid % 8) holds y[j][v] = Y[u][v] of its block.
// tl: JH_SLOTS * JH_TS ints; cm: C, 64 ints.  Leaves no barrier behind: the caller syncs before it writes tl again.
__device__ __forceinline__ void jh_forward(const uint8_t* __restrict__ img, int w, int bw, long long blocks, long long b0, int* tl,
                                           int* cm, long long (&y)[JH_B][8]) {
    const int tid = threadIdx.x, sub = tid & 7;
    if (tid < 64) cm[tid] = JH_C[tid >> 3][tid & 7];
#pragma unroll
    for (int j = 0; j < JH_B; ++j) {
        const int slot = j * (JH_THREADS / 8) + (tid >> 3);
        const long long b = b0 + slot;
        int px[8] = {128, 128, 128, 128, 128, 128, 128, 128};
        if (b < blocks) jh_load8(img + jh_block_origin(b, bw, w) + (size_t)sub * w, px);
        int t[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            int s = 0;
#pragma unroll
            for (int n = 0; n < 8; ++n) s += (px[n] - 128) * JH_C[v][n];
            t[v] = s;
        }
        int* row = tl + slot * JH_TS + sub * 8;
        *reinterpret_cast<u32x4*>(row) = mk_u4((uint32_t)t[0], (uint32_t)t[1], (uint32_t)t[2], (uint32_t)t[3]);
        *reinterpret_cast<u32x4*>(row + 4) = mk_u4((uint32_t)t[4], (uint32_t)t[5], (uint32_t)t[6], (uint32_t)t[7]);
    }
    __syncthreads();
    int c[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) c[r] = cm[sub * 8 + r];
#pragma unroll
    for (int j = 0; j < JH_B; ++j) {
        const int* blk = tl + (j * (JH_THREADS / 8) + (tid >> 3)) * JH_TS;
#pragma unroll
        for (int v = 0; v < 8; ++v) y[j][v] = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const u32x4 lo = *reinterpret_cast<const u32x4*>(blk + r * 8), hi = *reinterpret_cast<const u32x4*>(blk + r * 8 + 4);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                y[j][v] += (long long)c[r] * (int)lo[v];
                y[j][v + 4] += (long long)c[r] * (int)hi[v];
            }
        }
    }
}

__global__ __launch_bounds__(JH_THREADS) void jpeg_energies_kernel(const uint8_t* __restrict__ xu8, const JhTables tabs, int mt,
                                                                  unsigned long long* __restrict__ energies, int m_total, int h, int w,
                                                                  long long blocks) {
    __shared__ __attribute__((aligned(16))) int tl[JH_SLOTS * JH_TS];
    __shared__ __attribute__((aligned(16))) int qi[JH_TCH * 64];
    __shared__ __attribute__((aligned(16))) float qr[JH_TCH * 64];
    __shared__ int cm[64];
    __shared__ unsigned long long part[JH_WAVES * JH_TCH];         // [JH_WAVES][mt]
    const int tid = threadIdx.x, nn = blockIdx.y, u = tid & 7;
    for (int i = tid; i < mt * 64; i += JH_THREADS) {
        const int q = tabs.q[i >> 6][i & 63];
        qi[i] = q;
        qr[i] = 1.0f / (float)q;
    }
    long long y[JH_B][8];
    jh_forward(xu8 + (size_t)nn * h * w, w, w >> 3, blocks, (long long)blockIdx.x * JH_SLOTS, tl, cm, y);
    int a2[JH_B][8], p[JH_B][8], sg[JH_B][8];
#pragma unroll
    for (int j = 0; j < JH_B; ++j)
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const bool neg = y[j][v] < 0;
            const unsigned long long a = (unsigned long long)(neg ? -y[j][v] : y[j][v]);
            const int ah = (int)(a >> 26), al = (int)(a & 0x3FFFFFFull);
            const int lo = neg ? (32768 - al) >> 16 : (al + 32768) >> 16;
            sg[j][v] = neg ? -1024 : 1024;
            a2[j][v] = 2 * ah + (al >> 25);
            p[j][v] = sg[j][v] * ah + lo;
        }
#pragma unroll 1                                         // (qi / qr were staged before jh_forward's barrier)
    for (int mm = 0; mm < mt; ++mm) {
        int q[8];
        float rq[8];
        {
            const u32x4 q0 = *reinterpret_cast<const u32x4*>(qi + mm * 64 + u * 8), q1 = *reinterpret_cast<const u32x4*>(qi + mm * 64 + u * 8 + 4);
            const f32x4 r0 = *reinterpret_cast<const f32x4*>(qr + mm * 64 + u * 8), r1 = *reinterpret_cast<const f32x4*>(qr + mm * 64 + u * 8 + 4);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                q[v] = (int)q0[v]; q[v + 4] = (int)q1[v];
                rq[v] = r0[v]; rq[v + 4] = r1[v];
            }
        }
        unsigned long long e = 0;
#pragma unroll
        for (int j = 0; j < JH_B; ++j)
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const int t = (a2[j][v] + q[v]) >> 1;
                const int k = (int)((float)t * rq[v] + 0.002f);
                const int rp = p[j][v] - __mul24(sg[j][v], __mul24(k, q[v]));
                e += (unsigned long long)((long long)rp * rp);
            }
        e = wave_sum(e);
        if ((tid & 63) == 0) part[(tid >> 6) * mt + mm] = e;
    }
    count_flush<JH_WAVES>(part, mt, energies, (size_t)nn * m_total);
}

__global__ __launch_bounds__(JH_THREADS) void jpeg_predict_kernel(const uint8_t* __restrict__ xu8, const JhTables tabs, float* __restrict__ xhat,
                                                                 uint8_t* __restrict__ xout, int h, int w, long long blocks) {
    __shared__ __attribute__((aligned(16))) int tl[JH_SLOTS * JH_TS];
    __shared__ int cm[64];
    __shared__ int tq[64];
    __shared__ float unit[256];
    const int tid = threadIdx.x, nn = blockIdx.y, sub = tid & 7, bw = w >> 3;
    const long long b0 = (long long)blockIdx.x * JH_SLOTS;
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    float* hat = xhat ? xhat + (size_t)nn * h * w : nullptr;
    uint8_t* out = xout ? xout + (size_t)nn * h * w : nullptr;
    if (!((tabs.use >> nn) & 1u)) {                      // (uniform over the workgroup) no JPEG history: KB's prediction, the input as the twin
        unit[tid] = (float)tid / 255.0f;
        __syncthreads();
        const Taps3x3<float> kb = kb_taps_f32();
#pragma unroll 1
        for (int j = 0; j < JH_B; ++j) {
            const long long b = b0 + j * (JH_THREADS / 8) + (tid >> 3);
            if (b >= blocks) continue;
            const int r = (int)(b / bw) * 8 + sub, c0 = (int)(b % bw) * 8;
            int px[3][10];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint8_t* row = img + (size_t)min(max(r - 1 + i, 0), h - 1) * w;
                int mid[8];
                jh_load8(row + c0, mid);
                px[i][0] = row[max(c0 - 1, 0)];
                px[i][9] = row[min(c0 + 8, w - 1)];
#pragma unroll
                for (int n = 0; n < 8; ++n) px[i][n + 1] = mid[n];
            }
            float o[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                float q[3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) q[a][bb] = unit[px[a][n + bb]];
                const float pred = conv9_f32<true>(kb, q) * 255.0f;
                const bool border = r == 0 || r == h - 1 || c0 + n == 0 || c0 + n == w - 1;
                o[n] = border ? (float)px[1][n + 1] : pred;
            }
            const size_t at = (size_t)r * w + c0;
            if (hat) {
                *reinterpret_cast<f32x4*>(hat + at) = mk_f4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<f32x4*>(hat + at + 4) = mk_f4(o[4], o[5], o[6], o[7]);
            }
            if (out) *reinterpret_cast<u32x2*>(out + at) = *reinterpret_cast<const u32x2*>(img + at);
        }
        return;
    }
    if (tid < 64) tq[tid] = tabs.q[nn][tid];
    long long y[JH_B][8];
    jh_forward(img, w, bw, blocks, b0, tl, cm, y);
    __syncthreads();                                     // every thread has formed its coefficients: tl is free for the way back
    int q[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) q[v] = tq[sub * 8 + v];
#pragma unroll
    for (int j = 0; j < JH_B; ++j) {
        int kq[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const bool neg = y[j][v] < 0;
            const unsigned long long a = (unsigned long long)(neg ? -y[j][v] : y[j][v]);
            const unsigned t = (unsigned)((a + ((unsigned long long)q[v] << 25)) >> 26);
            const int m = (int)(t / (unsigned)q[v]) * q[v];
            kq[v] = neg ? -m : m;
        }
        int pr[8];                                       // P[u][n] = sum_v (k Q)[u][v] C[v][n], |P| < 2^27
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            int s = 0;
#pragma unroll
            for (int v = 0; v < 8; ++v) s += kq[v] * JH_C[v][n];
            pr[n] = s;
        }
        int* row = tl + (j * (JH_THREADS / 8) + (tid >> 3)) * JH_TS + sub * 8;
        *reinterpret_cast<u32x4*>(row) = mk_u4((uint32_t)pr[0], (uint32_t)pr[1], (uint32_t)pr[2], (uint32_t)pr[3]);
        *reinterpret_cast<u32x4*>(row + 4) = mk_u4((uint32_t)pr[4], (uint32_t)pr[5], (uint32_t)pr[6], (uint32_t)pr[7]);
    }
    __syncthreads();
    int c[8];                                            // column r = sub of C
#pragma unroll
    for (int uu = 0; uu < 8; ++uu) c[uu] = cm[uu * 8 + sub];
#pragma unroll 1
    for (int j = 0; j < JH_B; ++j) {
        const long long b = b0 + j * (JH_THREADS / 8) + (tid >> 3);
        if (b >= blocks) continue;
        const int* blk = tl + (j * (JH_THREADS / 8) + (tid >> 3)) * JH_TS;
        long long z[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) z[n] = 128ll << 26;
#pragma unroll
        for (int uu = 0; uu < 8; ++uu) {
            const u32x4 lo = *reinterpret_cast<const u32x4*>(blk + uu * 8), hi = *reinterpret_cast<const u32x4*>(blk + uu * 8 + 4);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                z[n] += (long long)c[uu] * (int)lo[n];
                z[n + 4] += (long long)c[uu] * (int)hi[n];
            }
        }
        const size_t at = jh_block_origin(b, bw, w) + (size_t)sub * w;
        if (hat) {
            float o[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const long long zc = z[n] < 0 ? 0 : z[n] > (255ll << 26) ? (255ll << 26) : z[n];
                o[n] = (float)((double)zc * (1.0 / 67108864.0));
            }
            *reinterpret_cast<f32x4*>(hat + at) = mk_f4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<f32x4*>(hat + at + 4) = mk_f4(o[4], o[5], o[6], o[7]);
        }
        if (out) {
            uint32_t wd[2] = {0u, 0u};
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const long long v = (z[n] + (1ll << 25)) >> 26;
                wd[n >> 2] |= (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v) << (8 * (n & 3));
            }
            *reinterpret_cast<u32x2*>(out + at) = mk_u2(wd[0], wd[1]);
        }
    }
}

// the checks both entry points share (`entries` table entries, the first of table number `first`); the number of blocks of a plane, 0 after
// the argument error has been set
long long jh_blocks(const char* who, const int* tables, long long entries, long long first, int n, int h, int w) {
    if (n < 1 || n > 65535 || h < 8 || w < 8 || h % 8 || w % 8) {
        wsu_set_error("%s: bad shape n=%d h=%d w=%d (1 <= n <= 65535; h and w positive multiples of 8)", who, n, h, w);
        return 0;
    }
    if ((long long)h * w > (1ll << 24)) { wsu_set_error("%s: h=%d w=%d: planes of more than 2^24 pixels are not supported", who, h, w); return 0; }
    for (long long i = 0; i < entries; ++i)
        if (tables[i] < 1 || tables[i] > 255) {
            wsu_set_error("%s: table %lld entry %lld is %d, outside 1..255", who, first + i / 64, i % 64, tables[i]);
            return 0;
        }
    return (long long)(h / 8) * (w / 8);
}

}  // namespace

extern "C" {

int wsu_jpeg_energies(const uint8_t* x_u8, const int* tables, int m, long long* energies, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && tables && energies, "jpeg_energies: null pointer");
    WSU_REQUIRE(m >= 1 && m <= 65536, "jpeg_energies: m=%d tables outside 1..65536", m);
    WSU_REQUIRE((uintptr_t)x_u8 % 8 == 0 && (uintptr_t)energies % 8 == 0, "jpeg_energies: x_u8 and energies must be 8-byte aligned");
    const long long blocks = jh_blocks("jpeg_energies", tables, (long long)m * 64, 0, n, h, w);
    if (!blocks) return WSU_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(energies, 0, (size_t)n * m * sizeof(long long), s) != hipSuccess) return wsu_check_launch("jpeg_energies memset");
    const unsigned tiles = (unsigned)((blocks + JH_SLOTS - 1) / JH_SLOTS);
    for (int m0 = 0; m0 < m; m0 += JH_TCH) {
        JhTables t{};
        const int mt = m - m0 < JH_TCH ? m - m0 : JH_TCH;
        for (int i = 0; i < mt * 64; ++i) t.q[i >> 6][i & 63] = (uint8_t)tables[(size_t)m0 * 64 + i];
        hipLaunchKernelGGL(jpeg_energies_kernel, dim3(tiles, n), dim3(JH_THREADS), 0, s, x_u8, t, mt,
                           reinterpret_cast<unsigned long long*>(energies) + m0, m, h, w, blocks);
        const int rc = wsu_check_launch("jpeg_energies_kernel");
        if (rc) return rc;
    }
    return 0;
}

int wsu_jpeg_predict(const uint8_t* x_u8, const int* tables, const uint8_t* use, float* x_hat, uint8_t* x_u8_out, int n, int h, int w,
                     void* stream) {
    WSU_REQUIRE(x_u8 && tables && use, "jpeg_predict: null pointer");
    WSU_REQUIRE(x_hat || x_u8_out, "jpeg_predict: null pointer: give x_hat, x_u8_out or both");
    WSU_REQUIRE((uintptr_t)x_u8 % 8 == 0 && (uintptr_t)x_u8_out % 8 == 0 && (uintptr_t)x_hat % 16 == 0,
                "jpeg_predict: x_u8 and x_u8_out must be 8-byte aligned, x_hat 16-byte aligned");
    if (n < 1 || n > 65535) { wsu_set_error("jpeg_predict: bad shape n=%d h=%d w=%d (1 <= n <= 65535)", n, h, w); return WSU_ERR_ARG; }
    for (int i = 0; i < n; ++i) {                        // the table of an image that does not use it is not read
        if (use[i] && !jh_blocks("jpeg_predict", tables + (size_t)i * 64, 64, i, n, h, w)) return WSU_ERR_ARG;
    }
    const long long blocks = jh_blocks("jpeg_predict", tables, 0, 0, n, h, w);
    if (!blocks) return WSU_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned tiles = (unsigned)((blocks + JH_SLOTS - 1) / JH_SLOTS);
    const size_t plane = (size_t)h * w;
    for (int n0 = 0; n0 < n; n0 += JH_TCH) {
        JhTables t{};
        const int nt = n - n0 < JH_TCH ? n - n0 : JH_TCH;
        for (int i = 0; i < nt; ++i) {
            if (!use[n0 + i]) continue;
            t.use |= 1u << i;
            for (int k = 0; k < 64; ++k) t.q[i][k] = (uint8_t)tables[(size_t)(n0 + i) * 64 + k];
        }
        hipLaunchKernelGGL(jpeg_predict_kernel, dim3(tiles, nt), dim3(JH_THREADS), 0, s, x_u8 + n0 * plane, t,
                           x_hat ? x_hat + n0 * plane : nullptr, x_u8_out ? x_u8_out + n0 * plane : nullptr, h, w, blocks);
        const int rc = wsu_check_launch("jpeg_predict_kernel");
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
