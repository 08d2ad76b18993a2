// K20-K23, K28, K30, K34: the stego simulators HILLR, LSBR, LSBRS, LSBRK and HILLRM (the reference ships ready-made twins of its five covers, made by a library outside its
// tree; tests/golden/stego_HILLR_* pins HILLR to those files bit for bit, LSBR's realisation is this package's own):
//
//   HILLR   key = HILL cost in float64 (the operation order of tests/hill_np.hill_cost), full frame
//           k   = floor((H*W - 1) * alpha / 2)             c_(k) = the key of rank k (0-based, ascending)
//           stego = cover ^ (key <= c_(k))                 (k + 1 changes when c_(k) is held by one pixel; ties are all flipped)
//   LSBR    stego = cover ^ (word < T),  T = floor(alpha / 2 * 2^32),  word = Philox4x32-10 word (i % 4) of counter (i / 4, 0, 0, 0)
//           under the image's 64-bit seed as key (low, high), i = the pixel's linear index in its image
//   LSBRS   stego = cover ^ (path position of i < m  and  word < 2^31),  m = floor(alpha * H * W): LSBR at alpha = 1 on the first m pixels
//           of the path over the whole plane, row by row from the top or from the bottom (K28)
//   LSBRK   stego = cover ^ (key word < T  and  word < 2^31),  T = floor(alpha * 2^32) compared in 64 bits, key word = the same Philox word
//           under the 64-bit stego key shared by all images: LSBR at alpha = 1 on the pixels the key selects (K30)
//   HILLRM  stego = cover ^ (key <= c_(k)  and  word < 2^31),  k = floor((H*W - 1) * alpha): LSBR at alpha = 1 on the pixels HILLR's
//           criterion selects, i.e. a real message instead of HILLR's flip of every selected pixel (K34)
//
// K23 is a rule of the pixel loop embed_span of wsu_embed.h (as K38 / K39 of ternary.hip are), which also holds the span, the change
// count and the launch set-up that K22, K28, K30 and K34 share; the shape check is WSU_REQUIRE_SHAPE of wsu_device.h.
// K20 is K12 in float64 on a 32 x 32 tile (the float64 arrays of a 64 x 64 tile would need 97 KB of LDS; a 32 x 32 tile needs 36 KB
// and stays static): every sum is a direct sum in numpy's order, the two divisions are IEEE divisions, nothing is contracted.  K21 is an
// exact radix select over the keys' uint64 patterns (positive and finite after the clamp, so monotone): six histogram passes of
// 11/11/11/11/11/9 bits.  All cross-workgroup traffic is integer atomics, results pass between kernels only at kernel boundaries, the
// workspace and the change counters are zeroed on the stream: two calls give the same bits.
#pragma clang fp contract(off)
#include "wsu_metric.h"
#include "wsu_embed.h"
#include "wsu_philox.h"

namespace {

typedef __attribute__((ext_vector_type(2))) double f64x2;

constexpr int ET = 32;                 // K20 output tile (ET x ET pixels per workgroup, 256 threads)
constexpr int EX = ET + 18;            // staged u8 window (pad 9 on each side)
constexpr int EXS = ET + 32;           // its LDS row stride (hill_stage_window)
constexpr int ER = ET + 16;            // |R| extent
constexpr int ES = ET + 14;            // S / rho0 extent

constexpr int SEL_LEVELS = 6;          // K21 radix: 11 / 11 / 11 / 11 / 11 / 9 bits
constexpr int SEL_BINS = 2048;
constexpr int SEL_PARTS = 64;          // K21 workgroups per image

// ---- K20 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hill_cost_f64_kernel(const uint8_t* __restrict__ x, double* __restrict__ cost, int h, int w,
                                                            int vec_in, int vec_out, double clamp) {
    __shared__ __attribute__((aligned(16))) uint8_t xs[EX * EXS];
    __shared__ short ar[ER * ER];
    __shared__ double rho[ES * ES];
    __shared__ __attribute__((aligned(16))) double hbuf[ES * ET];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * ET, r0 = blockIdx.y * ET, nn = blockIdx.z;
    const uint8_t* img = x + (size_t)nn * h * w;

    hill_stage_window<ET>(img, xs, r0, c0, h, w, vec_in, tid);
    __syncthreads();
    // ---- |R| (exact integers, |R| <= 16 * 255)
    for (int i = tid; i < ER * ER; i += 256) {
        const int a = i / ER, b = i % ER;
        const uint8_t* p = xs + a * EXS + b + 7;
        const int r = -(int)p[0] + 2 * (int)p[1] - (int)p[2]
                    + 2 * (int)p[EXS] - 4 * (int)p[EXS + 1] + 2 * (int)p[EXS + 2]
                    - (int)p[2 * EXS] + 2 * (int)p[2 * EXS + 1] - (int)p[2 * EXS + 2];
        ar[i] = (short)(r < 0 ? -r : r);
    }
    __syncthreads();
    // ---- S = box3x3(|R|) (exact), rho0 = 1 / (S / 9): two IEEE divisions, as numpy's `1.0 / (s / 9.0)`
    for (int i = tid; i < ES * ES; i += 256) {
        const int a = i / ES, b = i % ES;
        int s = 0;
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) s += ar[(a + u) * ER + b + v];
        const double m = (double)s / 9.0;
        rho[i] = s > 0 ? 1.0 / m : __builtin_inf();
    }
    __syncthreads();
    // ---- horizontal 15-tap direct sums, left to right from 0
    for (int i = tid; i < ES * ET; i += 256) {
        const int a = i / ET, b = i % ET;
        const double* p = rho + a * ES + b;
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < 15; ++t) s += p[t];
        hbuf[i] = s;
    }
    __syncthreads();
    // ---- vertical 15-tap direct sums, top to bottom from 0, / 225, clamp; two consecutive columns per thread -> one 16-byte store
    for (int i = tid; i < ET * (ET / 2); i += 256) {
        const int a = i / (ET / 2), b = (i % (ET / 2)) * 2;
        f64x2 s = {0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 15; ++t) s += *reinterpret_cast<const f64x2*>(hbuf + (a + t) * ET + b);
        s.x = s.x / 225.0;
        s.y = s.y / 225.0;
        s.x = s.x <= clamp ? s.x : clamp;          // inf / nan / > clamp -> clamp
        s.y = s.y <= clamp ? s.y : clamp;
        const int r = r0 + a, c = c0 + b;
        if (r >= h) continue;
        double* o = cost + ((size_t)nn * h + r) * w + c;
        if (vec_out && c + 2 <= w) {
            *reinterpret_cast<f64x2*>(o) = s;
        } else {
            if (c < w) o[0] = s.x;
            if (c + 1 < w) o[1] = s.y;
        }
    }
}

// ---- K21 ------------------------------------------------------------------------------------------------------------------
// Level l fixes the bits from sel_shift(l) upwards; the bits above sel_shift(l - 1) are the prefix the earlier levels found.
__device__ __forceinline__ int sel_shift(int level) { return level < SEL_LEVELS - 1 ? 53 - 11 * level : 0; }
__device__ __forceinline__ int sel_bins(int level) { return level < SEL_LEVELS - 1 ? SEL_BINS : 512; }
__device__ __forceinline__ uint64_t sel_mask(int level) { return level == 0 ? 0ull : ~0ull << sel_shift(level - 1); }

// Workspace: state[n][2] (uint64) = {prefix bits, remaining rank}, then hist[SEL_LEVELS][n][SEL_BINS] (uint32).
__device__ __forceinline__ uint32_t* sel_hist(void* ws, int level, int n, int nn) {
    return reinterpret_cast<uint32_t*>(static_cast<uint64_t*>(ws) + (size_t)2 * n) + ((size_t)level * n + nn) * SEL_BINS;
}

__global__ __launch_bounds__(256) void rank_select_hist_kernel(const uint64_t* __restrict__ keys, void* __restrict__ ws, int level,
                                                               int n, long long hw) {
    __shared__ uint32_t lh[SEL_BINS];
    const int nn = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const int shift = sel_shift(level), bins = sel_bins(level);
    const uint64_t mask = sel_mask(level);
    const uint64_t prefix = level == 0 ? 0ull : static_cast<const uint64_t*>(ws)[(size_t)2 * nn];
    for (int b = tid; b < SEL_BINS; b += 256) lh[b] = 0u;
    __syncthreads();
    const uint64_t* img = keys + (size_t)nn * hw;
    for (long long i = (long long)part * 256 + tid; i < hw; i += (long long)SEL_PARTS * 256) {
        const uint64_t u = img[i];
        if ((u & mask) == prefix) atomicAdd(&lh[(uint32_t)(u >> shift) & (uint32_t)(bins - 1)], 1u);
    }
    __syncthreads();
    uint32_t* hist = sel_hist(ws, level, n, nn);
    for (int b = tid; b < bins; b += 256)
        if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

// one workgroup per image: the bin that holds the remaining rank, by a fixed-order scan of the histogram; the last level writes the
// whole pattern.  A negative rank selects nothing: pattern 0, below every key.  A rank past the last is the last.
__global__ __launch_bounds__(256) void rank_select_pick_kernel(void* __restrict__ ws, const long long* __restrict__ k, int level,
                                                               uint64_t* __restrict__ bits, int n, long long hw) {
    __shared__ uint64_t part[256];
    const int nn = blockIdx.x, tid = threadIdx.x;
    const bool last = level == SEL_LEVELS - 1;
    const long long k0 = k[nn];
    if (k0 < 0) {                                            // (uniform over the workgroup)
        if (last && tid == 0) bits[nn] = 0ull;
        return;
    }
    uint64_t* st = static_cast<uint64_t*>(ws) + (size_t)2 * nn;
    const uint64_t prefix = level == 0 ? 0ull : st[0];
    const uint64_t kk = level == 0 ? (uint64_t)(k0 < hw ? k0 : hw - 1) : st[1];
    const uint32_t* hist = sel_hist(ws, level, n, nn);
    const int per = sel_bins(level) / 256;
    uint64_t mine = 0;
    for (int j = 0; j < per; ++j) mine += hist[tid * per + j];
    part[tid] = mine;
    __syncthreads();                                         // (also: every thread has read st[] before the finder writes it)
    uint64_t before = 0;
    for (int t = 0; t < tid; ++t) before += part[t];
    if (kk < before || kk >= before + mine) return;
    for (int j = 0; j < per; ++j) {
        const uint64_t cnt = hist[tid * per + j];
        if (kk < before + cnt) {
            const uint64_t found = prefix | ((uint64_t)(tid * per + j) << sel_shift(level));
            st[0] = found;
            st[1] = kk - before;
            if (last) bits[nn] = found;
            return;
        }
        before += cnt;
    }
}

// ---- K22: a pixel loop of its own (wsu_embed.h says why) ------------------------------------------------------------------------------
// A wave takes 1024 consecutive pixels at a time: lane l owns pixels 16 l .. 16 l + 15 (one 16-byte load and store), the keys are
// read 64 consecutive ones per step (lane l: key 64 j + l) and a ballot hands every lane the 16 decisions of its pixels.
__global__ __launch_bounds__(256) void embed_threshold_kernel(const uint8_t* __restrict__ cover, const uint64_t* __restrict__ keys,
                                                              const uint64_t* __restrict__ bits, uint8_t* __restrict__ stego,
                                                              long long* __restrict__ changes, long long hw) {
    const int nn = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const uint8_t* cin = cover + (size_t)nn * hw;
    uint8_t* cout = stego + (size_t)nn * hw;
    const uint64_t* kin = keys + (size_t)nn * hw;
    const uint64_t thr = bits[nn];
    const Span sp = image_span(cin, cout, hw, false);
    int cnt = 0;
    const long long nwaves = (long long)gridDim.x * 4;
    for (long long ch = (long long)blockIdx.x * 4 + (tid >> 6); ch * 64 < sp.groups; ch += nwaves) {       // (uniform over the wave)
        const long long base = sp.head + ch * 1024, end = sp.head + 16 * sp.groups;
        uint32_t my = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long long i = base + j * 64 + lane;
            const bool flip = i < end && kin[i] <= thr;
            const unsigned long long m = __ballot(flip);
            if ((lane >> 2) == j) my = (uint32_t)(m >> (16 * (lane & 3))) & 0xFFFFu;
        }
        const long long g = ch * 64 + lane;
        if (g < sp.groups) {
            u32x4 v = *reinterpret_cast<const u32x4*>(cin + sp.head + 16 * g);
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e >> 2] ^= ((my >> e) & 1u) << (8 * (e & 3));
            *reinterpret_cast<u32x4*>(cout + sp.head + 16 * g) = v;
            cnt += __popc(my);
        }
    }
    for (long long j = (long long)blockIdx.x * 256 + tid; j < sp.bytes; j += (long long)gridDim.x * 256) {
        const long long i = span_byte_index(sp, j);
        const uint8_t flip = kin[i] <= thr ? 1 : 0;
        cout[i] = cin[i] ^ flip;
        cnt += flip;
    }
    add_changes(cnt, changes + nn, tid);
}

// ---- K23: a rule of embed_span; K28 and K30: the same loop written out (why: at K30) ---------------------------------------------------
// Pixel i draws the Philox word philox_byte(i, seed) (philox_quad: the four of a quad, wsu_philox.h); a rule says what the draw does to
// the pixel.

// K23.  LSBR: a pixel flips iff its word is below the image's threshold.
struct LsbrRule {
    SeedKey k;
    uint32_t thr;
    __device__ __forceinline__ uint32_t quad(long long i0, uint32_t x, int& cnt) const {
        const uint32_t flips = below_bytes(philox_quad(i0, k), thr);
        cnt += __popc(flips);
        return x ^ flips;
    }
    __device__ __forceinline__ uint8_t byte(long long i, uint8_t x, int& cnt) const {
        const uint8_t flip = philox_byte(i, k) < thr ? 1 : 0;
        cnt += flip;
        return x ^ flip;
    }
};
__global__ __launch_bounds__(256) void embed_lsbr_kernel(const uint8_t* __restrict__ cover, const uint64_t* __restrict__ seeds,
                                                         const uint32_t* __restrict__ thresholds, uint8_t* __restrict__ stego,
                                                         long long* __restrict__ changes, long long hw) {
    const int nn = blockIdx.y;
    embed_span(LsbrRule{SeedKey(seeds[nn]), thresholds[nn]}, cover + (size_t)nn * hw, stego + (size_t)nn * hw, hw, changes + nn);
}

// K28.  LSBRS: the message occupies the first m pixels of the path over the whole plane (row by row, left to right; rows from the top,
// order 0, or from the bottom, order 1); a pixel on it flips as under K23 at alpha = 1 (word < 2^31).  The first m path positions are at
// most two runs of linear indices: order 0: [0, m); order 1: the m / w full rows at the bottom, [(h - m / w) w, h w), and the first m % w
// pixels of the row above them.  A quad of pixels outside both runs costs no generator call.
struct Runs { long long a0, a1, b0, b1; };
__device__ __forceinline__ bool in_runs(const Runs& u, long long i) { return (i >= u.a0 && i < u.a1) || (i >= u.b0 && i < u.b1); }

__global__ __launch_bounds__(256) void embed_lsbr_seq_kernel(const uint8_t* __restrict__ cover, const uint64_t* __restrict__ seeds,
                                                             const long long* __restrict__ counts, int order, uint8_t* __restrict__ stego,
                                                             long long* __restrict__ changes, long long hw, int w) {
    const int nn = blockIdx.y, tid = threadIdx.x;
    const uint8_t* cin = cover + (size_t)nn * hw;
    uint8_t* cout = stego + (size_t)nn * hw;
    const uint32_t k0 = (uint32_t)seeds[nn], k1 = (uint32_t)(seeds[nn] >> 32), thr = 0x80000000u;
    long long m = counts[nn];
    m = m < 0 ? 0 : m > hw ? hw : m;
    Runs u{0, m, 0, 0};
    if (order) {
        const long long full = hw - m / w * w;                              // the first pixel of the full rows
        u = Runs{full, hw, full - w, full - w + m % w};                     // (m % w == 0: the second run is empty, also where full == 0)
    }
    const Span sp = image_span(cin, cout, hw, true);
    int cnt = 0;
    for (long long g = (long long)blockIdx.x * 256 + tid; g < sp.groups; g += (long long)gridDim.x * 256) {
        const long long p = sp.head + 16 * g;                               // a multiple of 4
        u32x4 v = *reinterpret_cast<const u32x4*>(cin + p);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t on = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) on |= (in_runs(u, p + 4 * q + e) ? 1u : 0u) << (8 * e);
            if (on) {
                const Words4 wd = philox4x32_10((uint32_t)(p / 4 + q), k0, k1);
                uint32_t flips = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) flips |= (wd.v[e] < thr ? 1u : 0u) << (8 * e);
                flips &= on;
                v[q] ^= flips;
                cnt += __popc(flips);
            }
        }
        *reinterpret_cast<u32x4*>(cout + p) = v;
    }
    for (long long j = (long long)blockIdx.x * 256 + tid; j < sp.bytes; j += (long long)gridDim.x * 256) {
        const long long i = span_byte_index(sp, j);
        uint8_t flip = 0;
        if (in_runs(u, i)) {
            const Words4 wd = philox4x32_10((uint32_t)(i / 4), k0, k1);
            const int e = (int)(i & 3);
            const uint32_t word = e == 0 ? wd.v[0] : e == 1 ? wd.v[1] : e == 2 ? wd.v[2] : wd.v[3];
            flip = word < thr ? 1 : 0;
        }
        cout[i] = cin[i] ^ flip;
        cnt += flip;
    }
    add_changes(cnt, changes + nn, tid);
}

// K30.  LSBRK: the message occupies the pixels a stego key selects, the same in every image: pixel i is used iff word i % 4 of counter
// (i / 4, 0, 0, 0) under the key is below `thr` (floor(alpha * 2^32), up to 2^32: 64-bit comparison); a used pixel flips as under K23 at
// alpha = 1 with the image's own seed.  A quad without a used pixel costs one generator call, not two.  MASK: the used positions
// themselves (1 / 0), one plane, no cover, no change count.  Written as rules of embed_span, K28 and this kernel compiled to all but the
// same instructions and yet measured slower than before (K28 3.4 % on average, K30 up to 4.7 % in single runs, profiles/r33), so both
// keep their own loops over image_span.
template <bool MASK>
__global__ __launch_bounds__(256) void embed_lsbr_keyed_kernel(const uint8_t* __restrict__ cover, const uint64_t* __restrict__ seeds,
                                                               uint64_t key, uint64_t thr, uint8_t* __restrict__ stego,
                                                               long long* __restrict__ changes, long long hw) {
    const int nn = blockIdx.y, tid = threadIdx.x;
    uint8_t* cout = stego + (size_t)nn * hw;
    const uint8_t* cin = MASK ? cout : cover + (size_t)nn * hw;
    const uint32_t kk0 = (uint32_t)key, kk1 = (uint32_t)(key >> 32);
    uint32_t k0 = 0, k1 = 0;
    if (!MASK) { k0 = (uint32_t)seeds[nn]; k1 = (uint32_t)(seeds[nn] >> 32); }
    const Span sp = image_span(cin, cout, hw, true);
    int cnt = 0;
    for (long long g = (long long)blockIdx.x * 256 + tid; g < sp.groups; g += (long long)gridDim.x * 256) {
        const long long p = sp.head + 16 * g;                               // a multiple of 4
        u32x4 v = {0u, 0u, 0u, 0u};
        if (!MASK) v = *reinterpret_cast<const u32x4*>(cin + p);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t on = below_bytes(philox4x32_10((uint32_t)(p / 4 + q), kk0, kk1), thr);
            if (MASK) {
                v[q] = on;
            } else if (on) {
                const uint32_t flips = below_bytes(philox4x32_10((uint32_t)(p / 4 + q), k0, k1), 0x80000000ull) & on;
                v[q] ^= flips;
                cnt += __popc(flips);
            }
        }
        *reinterpret_cast<u32x4*>(cout + p) = v;
    }
    for (long long j = (long long)blockIdx.x * 256 + tid; j < sp.bytes; j += (long long)gridDim.x * 256) {
        const long long i = span_byte_index(sp, j);
        const int e = (int)(i & 3);
        const bool on = (uint64_t)word_of(philox4x32_10((uint32_t)(i / 4), kk0, kk1), e) < thr;
        if (MASK) {
            cout[i] = on ? 1 : 0;
        } else {
            const uint8_t flip = on && word_of(philox4x32_10((uint32_t)(i / 4), k0, k1), e) < 0x80000000u ? 1 : 0;
            cout[i] = cin[i] ^ flip;
            cnt += flip;
        }
    }
    if (!MASK) add_changes(cnt, changes + nn, tid);
}

// K34.  HILLRM: HILLR's pixel selection with a real message: a pixel whose key is at most the threshold pattern is USED, and a used pixel
// flips as under K23 at alpha = 1 with the image's seed (word < 2^31).  One thread per quad of pixels (one generator call, none where no
// pixel of the quad is used); bytes in and out, so any alignment and in-place use are fine.
__global__ __launch_bounds__(256) void embed_threshold_lsbr_kernel(const uint8_t* __restrict__ cover, const uint64_t* __restrict__ keys,
                                                                   const uint64_t* __restrict__ bits, const uint64_t* __restrict__ seeds,
                                                                   uint8_t* __restrict__ stego, long long* __restrict__ changes, long long hw) {
    const int nn = blockIdx.y, tid = threadIdx.x;
    const uint8_t* cin = cover + (size_t)nn * hw;
    uint8_t* cout = stego + (size_t)nn * hw;
    const uint64_t* kin = keys + (size_t)nn * hw;
    const uint64_t thr = bits[nn];
    const uint32_t k0 = (uint32_t)seeds[nn], k1 = (uint32_t)(seeds[nn] >> 32);
    int cnt = 0;
    for (long long g = (long long)blockIdx.x * 256 + tid; 4 * g < hw; g += (long long)gridDim.x * 256) {
        bool used[4];
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            used[e] = 4 * g + e < hw && kin[4 * g + e] <= thr;
            any = any || used[e];
        }
        Words4 wd{{~0u, ~0u, ~0u, ~0u}};
        if (any) wd = philox4x32_10((uint32_t)g, k0, k1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * g + e < hw) {
                const uint8_t flip = used[e] && wd.v[e] < 0x80000000u ? 1 : 0;
                cout[4 * g + e] = cin[4 * g + e] ^ flip;
                cnt += flip;
            }
        }
    }
    add_changes(cnt, changes + nn, tid);
}

}  // namespace

extern "C" {

int wsu_hill_cost_f64(const uint8_t* x_u8, double* key, double clamp, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && key, "hill_cost_f64: null pointer");
    WSU_REQUIRE_SHAPE("hill_cost_f64", WSU_COUNTER_PIXELS, "counters");
    WSU_REQUIRE(clamp > 0.0 && clamp < __builtin_inf(), "hill_cost_f64: clamp=%g must be positive and finite", clamp);
    const int vec_in = (w % 16 == 0) && ((uintptr_t)x_u8 % 16 == 0);
    const int vec_out = (w % 2 == 0) && ((uintptr_t)key % 16 == 0);
    hipLaunchKernelGGL(hill_cost_f64_kernel, dim3((w + ET - 1) / ET, (h + ET - 1) / ET, n), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x_u8, key, h, w, vec_in, vec_out, clamp);
    return wsu_check_launch("hill_cost_f64_kernel");
}

size_t wsu_rank_select_f64_workspace_bytes(int n) {
    return n > 0 ? (size_t)n * (2 * sizeof(uint64_t) + (size_t)SEL_LEVELS * SEL_BINS * sizeof(uint32_t)) : 0;
}

int wsu_rank_select_f64(const double* key, const long long* k, uint64_t* bits, void* workspace, size_t workspace_bytes,
                        int n, int h, int w, void* stream) {
    WSU_REQUIRE(key && k && bits && workspace, "rank_select_f64: null pointer");
    WSU_REQUIRE_SHAPE("rank_select_f64", WSU_COUNTER_PIXELS, "counters");
    WSU_REQUIRE(workspace_bytes >= wsu_rank_select_f64_workspace_bytes(n), "rank_select_f64: workspace too small");
    WSU_REQUIRE((uintptr_t)workspace % 8 == 0, "rank_select_f64: workspace must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long hw = (long long)h * w;
    if (hipMemsetAsync(workspace, 0, wsu_rank_select_f64_workspace_bytes(n), s) != hipSuccess) return wsu_check_launch("rank_select_f64 memset");
    for (int level = 0; level < SEL_LEVELS; ++level) {
        hipLaunchKernelGGL(rank_select_hist_kernel, dim3(SEL_PARTS, n), dim3(256), 0, s, reinterpret_cast<const uint64_t*>(key), workspace,
                           level, n, hw);
        int rc = wsu_check_launch("rank_select_hist_kernel");
        if (rc) return rc;
        hipLaunchKernelGGL(rank_select_pick_kernel, dim3(n), dim3(256), 0, s, workspace, k, level, bits, n, hw);
        rc = wsu_check_launch("rank_select_pick_kernel");
        if (rc) return rc;
    }
    return 0;
}

int wsu_embed_threshold(const uint8_t* cover, const double* key, const uint64_t* bits, uint8_t* stego, long long* changes,
                        int n, int h, int w, void* stream) {
    WSU_REQUIRE(cover && key && bits && stego && changes, "embed_threshold: null pointer");
    WSU_REQUIRE_SHAPE("embed_threshold", WSU_COUNTER_PIXELS, "counters");
    return embed_launch("embed_threshold memset", "embed_threshold_kernel", embed_threshold_kernel, changes, n, h, w, stream, cover,
                        reinterpret_cast<const uint64_t*>(key), bits, stego, changes, (long long)h * w);
}

int wsu_lsbr_threshold(double alpha, uint32_t* threshold) {
    WSU_REQUIRE(threshold, "lsbr_threshold: null pointer");
    WSU_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "lsbr_threshold: alpha=%g outside [0, 1]", alpha);
    *threshold = (uint32_t)(alpha / 2.0 * 4294967296.0);               // floor: the product is not negative
    return 0;
}

int wsu_embed_lsbr(const uint8_t* cover, const uint64_t* seeds, const uint32_t* thresholds, uint8_t* stego, long long* changes,
                   int n, int h, int w, void* stream) {
    WSU_REQUIRE(cover && seeds && thresholds && stego && changes, "embed_lsbr: null pointer");
    WSU_REQUIRE_SHAPE("embed_lsbr", WSU_COUNTER_PIXELS, "counters");
    return embed_launch("embed_lsbr memset", "embed_lsbr_kernel", embed_lsbr_kernel, changes, n, h, w, stream, cover, seeds, thresholds, stego,
                        changes, (long long)h * w);
}

int wsu_embed_lsbr_seq(const uint8_t* cover, const uint64_t* seeds, const long long* counts, int order, uint8_t* stego, long long* changes,
                       int n, int h, int w, void* stream) {
    WSU_REQUIRE(cover && seeds && counts && stego && changes, "embed_lsbr_seq: null pointer");
    WSU_REQUIRE(order == 0 || order == 1, "embed_lsbr_seq: order=%d outside {0 = rows from the top, 1 = rows from the bottom}", order);
    WSU_REQUIRE_SHAPE("embed_lsbr_seq", WSU_COUNTER_PIXELS, "counters");
    return embed_launch("embed_lsbr_seq memset", "embed_lsbr_seq_kernel", embed_lsbr_seq_kernel, changes, n, h, w, stream, cover, seeds, counts,
                        order, stego, changes, (long long)h * w, w);
}

int wsu_embed_lsbr_keyed(const uint8_t* cover, const uint64_t* seeds, uint64_t key_seed, uint64_t alpha_threshold, uint8_t* stego,
                         long long* changes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(cover && seeds && stego && changes, "embed_lsbr_keyed: null pointer");
    WSU_REQUIRE(alpha_threshold <= (1ull << 32), "embed_lsbr_keyed: alpha_threshold=%llu above 2^32", (unsigned long long)alpha_threshold);
    WSU_REQUIRE_SHAPE("embed_lsbr_keyed", WSU_COUNTER_PIXELS, "counters");
    return embed_launch("embed_lsbr_keyed memset", "embed_lsbr_keyed_kernel", embed_lsbr_keyed_kernel<false>, changes, n, h, w, stream, cover,
                        seeds, key_seed, alpha_threshold, stego, changes, (long long)h * w);
}

int wsu_embed_threshold_lsbr(const uint8_t* cover, const double* key, const uint64_t* bits, const uint64_t* seeds, uint8_t* stego,
                             long long* changes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(cover && key && bits && seeds && stego && changes, "embed_threshold_lsbr: null pointer");
    WSU_REQUIRE_SHAPE("embed_threshold_lsbr", WSU_COUNTER_PIXELS, "counters");
    return embed_launch("embed_threshold_lsbr memset", "embed_threshold_lsbr_kernel", embed_threshold_lsbr_kernel, changes, n, h, w, stream,
                        cover, reinterpret_cast<const uint64_t*>(key), bits, seeds, stego, changes, (long long)h * w);
}

// (no change counters to zero: the launch is written out)
int wsu_lsbr_key_mask(uint64_t key_seed, uint64_t alpha_threshold, uint8_t* mask, int h, int w, void* stream) {
    const int n = 1;
    WSU_REQUIRE(mask, "lsbr_key_mask: null pointer");
    WSU_REQUIRE(alpha_threshold <= (1ull << 32), "lsbr_key_mask: alpha_threshold=%llu above 2^32", (unsigned long long)alpha_threshold);
    WSU_REQUIRE_SHAPE("lsbr_key_mask", WSU_COUNTER_PIXELS, "counters");
    const long long hw = (long long)h * w;
    hipLaunchKernelGGL(embed_lsbr_keyed_kernel<true>, dim3(embed_blocks(hw), 1), dim3(256), 0, static_cast<hipStream_t>(stream), nullptr, nullptr,
                       key_seed, alpha_threshold, mask, nullptr, hw);
    return wsu_check_launch("embed_lsbr_keyed_kernel");
}

}  // extern "C"
