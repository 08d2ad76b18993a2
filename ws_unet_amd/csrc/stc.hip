// K40-K44: binary syndrome-trellis codes (Filler, Judas, Fridrich, "Minimizing additive distortion in steganography using syndrome-trellis
// codes", IEEE TIFS 6(3), 2011): a real message embedded with near-minimal cost and read back.  Not part of the reference.
//
//   the code, per image, over the LSBs x[0..n) along a pixel path, costs rho[0..n) >= 0 (+inf: wet), message m[0..k), constraint height
//   h in 1..10, S = 2^h states and a column table cols[0..ceil(n / k)):
//     block i owns the path positions [floor(i n / k), floor((i + 1) n / k)); position t of it has column cols[t] & ((1 << min(h, k - i)) - 1)
//     forward   W[0] = 0, W[s > 0] = +inf;  per position j with column c:  a = W[s] + (x_j ? rho_j : 0),  b = W[s ^ c] + (x_j ? 0 : rho_j),
//               take[j][s] = b < a (a tie keeps y = 0),  W[s] = take ? b : a;  after block i:  W[s] = W[2 s + m_i] for s < S / 2, +inf above
//               cost = W[0] after the last block;  ok = cost < +inf
//     backward  s = 0;  for i = k - 1 .. 0:  s = 2 s + m_i, then over the block's positions downwards  y_j = take[j][s],  s ^= c_j where y_j
//     extract   m_b = XOR of y_j over the blocks i in (b - h, b] and their positions t whose column has bit b - i set
//   K40  the generator word of every pixel: word p % 4 of Philox4x32-10 on counter (p / 4, 0, 0, 0) under the image's seed (K23's word)
//   K41  forward and backward; where y_j != x_j the pixel flips its LSB (change 0) or moves by d = +1 / -1 as bit 0 of its generator word
//        is 1 / 0, inwards at 0 and 255 (change 1)
//   K42  extract
//   K43  K41 with a message length, a row stride and a first bit per image (ks, first: DEVICE int32 [N]); ks[i] == 0: no block exists, y = x,
//        cost 0, ok 1.  An image whose (ks, first) is out of range (k < 0, k > n, first < 0, first + k > max_bits, ceil(n / k) > cols_len) is
//        clamped to k = 0 and reported with cost +inf and ok 0: nothing is read or written out of bounds on its account.
//   K44  K42 with the same per-image arguments and the code's bit within the stego byte; an image with k == 0 or out of range writes nothing
//
// K41 / K43 and K42 / K44 are the same kernels: a workgroup reads its image's (k, message row) once at entry (StcImage), uniform or ragged.
//
// Only float64 additions and comparisons touch a cost, so the bits are those of the numpy restatement whatever the schedule.
//
// Organisation: one workgroup per image, one thread per state.  h <= 6 is one wave: W lives in a register, W[s ^ c]
// and the end-of-block shift are lane permutes, there is no barrier.  Above that W is double-buffered in LDS with ONE barrier per
// position; the end-of-block shift costs none, because the position that ends a block writes its results to their shifted places.  A
// position's x, rho, path and column are staged by the whole workgroup 1024 positions at a time; a wave then holds 64 positions in
// registers and hands one to all its lanes per step as scalars.  take[j] is one ballot word per wave; lane p keeps position p's and the
// wave stores its 64 words together.  The backward walk is a chain of dependent reads: the workgroup copies 256 positions' take words into LDS, thread 0 walks them there, then
// 256 threads apply the changes.  Every loop's trip count is known when the workgroup starts (it has read its image's k by then); nothing waits on a flag.
#pragma clang fp contract(off)
#include "wsu_metric.h"
#include "wsu_philox.h"

namespace {

constexpr int STC_MAX_H = 10;
constexpr int STC_STAGE = 1024;        // forward: positions staged at a time
constexpr int STC_BACK = 256;          // backward: positions per LDS chunk
constexpr uint32_t STC_LAST = 0x10000u;  // the position ends its block; bit 17 then holds the block's message bit
constexpr uint32_t STC_XBIT = 0x40000u;  // forward staging: the cover's LSB at the position

// position j of the path -> its column (low 16 bits) | STC_LAST | message bit << 17
__device__ __forceinline__ uint32_t stc_position(long long j, long long n, int k, int height, const uint32_t* __restrict__ cols,
                                                 const uint8_t* __restrict__ msg) {
    const long long i = ((j + 1) * k - 1) / n;                                 // the block that owns j
    const long long start = i * n / k, end = (i + 1) * n / k;
    const int rows = k - i < height ? (int)(k - i) : height;
    uint32_t cf = cols[j - start] & ((1u << rows) - 1u);
    if (j + 1 == end) cf |= STC_LAST | ((uint32_t)(msg[i] & 1) << 17);
    return cf;
}
// the pixel of path position j, or -1 where a path entry lies outside the image (never dereferenced)
__device__ __forceinline__ long long stc_pixel(const int32_t* __restrict__ path, long long j, long long n) {
    const long long p = path ? (long long)path[j] : j;
    return p >= 0 && p < n ? p : -1;
}
__device__ __forceinline__ double lane_double(double v, int lane) {            // lane `lane`'s v, as a scalar
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// what a workgroup knows of its image's code: the message length, the row its bits start at, and whether ragged arguments were out of range
struct StcImage { int k; bool bad; size_t at; };                               // at: the first message byte, from `message`
struct StcRagged { const int32_t* ks; const int32_t* first; long long stride; int max_bits, cols_len; };     // ks == nullptr: uniform k
__device__ __forceinline__ StcImage stc_image(const StcRagged& rg, long long n, int k, int nn) {
    if (!rg.ks) return StcImage{k, false, (size_t)nn * k};
    const int ki = rg.ks[nn], f = rg.first[nn];
    const bool bad = ki < 0 || ki > n || f < 0 || (long long)f + ki > rg.max_bits || (ki > 0 && (n + ki - 1) / ki > rg.cols_len);
    return StcImage{bad ? 0 : ki, bad, (size_t)nn * rg.stride + (bad ? 0 : f)};
}

// ---- K40 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void philox_words_kernel(const uint64_t* __restrict__ seeds, uint32_t* __restrict__ words, long long hw) {
    const int nn = blockIdx.y;
    const uint32_t k0 = (uint32_t)seeds[nn], k1 = (uint32_t)(seeds[nn] >> 32);
    uint32_t* out = words + (size_t)nn * hw;
    const long long quads = (hw + 3) / 4;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < quads; g += (long long)gridDim.x * 256) {
        const Words4 wd = philox4x32_10((uint32_t)g, k0, k1);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * g + e < hw) out[4 * g + e] = wd.v[e];
    }
}

// ---- K41, forward ---------------------------------------------------------------------------------------------------------
template <bool ONE_WAVE>
__global__ __launch_bounds__(1024) void stc_forward_kernel(const uint8_t* __restrict__ cover, const double* __restrict__ rho,
                                                           const uint8_t* __restrict__ message, const uint32_t* __restrict__ cols,
                                                           const int32_t* __restrict__ path, unsigned long long* __restrict__ take,
                                                           double* __restrict__ cost, uint8_t* __restrict__ ok, long long n, int k_uniform,
                                                           int height, StcRagged rg) {
    __shared__ double wb[ONE_WAVE ? 1 : 2][ONE_WAVE ? 1 : 1 << STC_MAX_H];
    __shared__ double rs[STC_STAGE];
    __shared__ uint32_t cfs[STC_STAGE];
    const int nn = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthreads = blockDim.x, wpp = nthreads >> 6, half = (1 << height) >> 1;
    const double inf = __builtin_inf();
    const uint8_t* cimg = cover + (size_t)nn * n;
    const double* rimg = rho + (size_t)nn * n;
    const StcImage im = stc_image(rg, n, k_uniform, nn);
    const int k = im.k;
    const uint8_t* msg = message + im.at;
    const long long nrun = k > 0 ? n : 0;                                      // k == 0: no block, W stays (0, +inf ..)
    const int32_t* pimg = path ? path + (size_t)nn * n : nullptr;
    unsigned long long* timg = take + (size_t)nn * n * wpp;
    double wreg = tid == 0 ? 0.0 : inf;                                        // ONE_WAVE: W[lane]
    int cur = 0;
    if (!ONE_WAVE) wb[0][tid] = wreg;                                          // (the staging barrier below publishes it)
    for (long long base = 0; base < nrun; base += STC_STAGE) {
        const int cnt = n - base < STC_STAGE ? (int)(n - base) : STC_STAGE;
        __syncthreads();                                                       // the previous stage has been read
        for (int q = tid; q < cnt; q += nthreads) {
            const long long j = base + q, pix = stc_pixel(pimg, j, n);
            const double r = pix >= 0 ? rimg[pix] : inf;
            const uint32_t xb = pix >= 0 ? cimg[pix] & 1u : 0u;
            rs[q] = r;
            cfs[q] = stc_position(j, n, k, height, cols, msg) | (xb ? STC_XBIT : 0u);
        }
        __syncthreads();
        for (int g = 0; g < cnt; g += 64) {
            const int q = g + lane < cnt ? g + lane : cnt - 1;
            const double rl = rs[q];
            const int cfl = (int)cfs[q];
            const int m = cnt - g < 64 ? cnt - g : 64;
            int tlo = 0, thi = 0;                                              // lane p: position g + p's ballot word
            for (int p = 0; p < m; ++p) {
                const uint32_t cf = (uint32_t)__builtin_amdgcn_readlane(cfl, p);
                const double r = lane_double(rl, p);
                const double c0 = (cf & STC_XBIT) ? r : 0.0, c1 = (cf & STC_XBIT) ? 0.0 : r;   // (scalars)
                const int c = (int)(cf & 0xFFFFu);
                double a, b;
                if (ONE_WAVE) {
                    a = wreg + c0;
                    b = __shfl(wreg, lane ^ c, 64) + c1;
                } else {
                    a = wb[cur][tid] + c0;
                    b = wb[cur][tid ^ c] + c1;
                }
                const bool tk = b < a;
                const double wv = tk ? b : a;
                const unsigned long long word = __ballot(tk);
                tlo = lane == p ? (int)(uint32_t)word : tlo;
                thi = lane == p ? (int)(uint32_t)(word >> 32) : thi;
                if (cf & STC_LAST) {                                           // (uniform) W'[s] = W[2 s + m_i], +inf above S / 2
                    const int mi = (int)((cf >> 17) & 1u);
                    if (ONE_WAVE) {
                        const double v = __shfl(wv, (2 * lane + mi) & 63, 64);
                        wreg = lane < half ? v : inf;
                    } else {
                        const bool keep = (tid & 1) == mi;
                        wb[cur ^ 1][keep ? tid >> 1 : half + (tid >> 1)] = keep ? wv : inf;
                    }
                } else {
                    if (ONE_WAVE) wreg = wv;
                    else wb[cur ^ 1][tid] = wv;
                }
                if (!ONE_WAVE) {
                    __syncthreads();
                    cur ^= 1;
                }
            }
            if (lane < m) timg[(base + g + lane) * wpp + wave] = ((unsigned long long)(uint32_t)thi << 32) | (uint32_t)tlo;
        }
    }
    if (tid == 0) {
        const double total = im.bad ? inf : ONE_WAVE ? wreg : wb[cur][0];
        cost[nn] = total;
        ok[nn] = total < inf ? 1 : 0;
    }
}

// ---- K41, backward --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void stc_backward_kernel(const uint8_t* __restrict__ cover, const uint8_t* __restrict__ message,
                                                            const uint32_t* __restrict__ cols, const int32_t* __restrict__ path,
                                                            const uint64_t* __restrict__ seeds, const unsigned long long* __restrict__ take,
                                                            const double* __restrict__ cost, uint8_t* __restrict__ stego,
                                                            long long* __restrict__ changes, long long n, int k_uniform, int height, int change,
                                                            StcRagged rg) {
    __shared__ unsigned long long tks[STC_BACK << (STC_MAX_H - 6)];            // 32 KiB
    __shared__ uint32_t cfs[STC_BACK];
    __shared__ uint8_t ys[STC_BACK];
    __shared__ int total;
    const int nn = blockIdx.x, tid = threadIdx.x;
    const int nthreads = blockDim.x, wpp = nthreads >> 6;
    const uint32_t smask = (1u << height) - 1u;
    const uint8_t* cimg = cover + (size_t)nn * n;
    uint8_t* simg = stego + (size_t)nn * n;
    const StcImage im = stc_image(rg, n, k_uniform, nn);
    const int k = im.k;
    const uint8_t* msg = message + im.at;
    const int32_t* pimg = path ? path + (size_t)nn * n : nullptr;
    const unsigned long long* timg = take + (size_t)nn * n * wpp;
    const uint32_t k0 = (uint32_t)seeds[nn], k1 = (uint32_t)(seeds[nn] >> 32);
    const bool good = k > 0 && cost[nn] < __builtin_inf();                     // else the stego is the cover
    uint32_t s = 0;                                                            // thread 0's state
    int cnt = 0;
    if (tid == 0) total = 0;
    for (long long hi = n; hi > 0; hi -= STC_BACK) {
        const long long lo = hi > STC_BACK ? hi - STC_BACK : 0;
        const int m = (int)(hi - lo);
        __syncthreads();                                                       // the previous chunk has been applied
        if (good) {
            for (int q = tid; q < m * wpp; q += nthreads) tks[q] = timg[lo * wpp + q];
            for (int q = tid; q < m; q += nthreads) cfs[q] = stc_position(lo + q, n, k, height, cols, msg);
            __syncthreads();
            if (tid == 0) {
                for (int q = m - 1; q >= 0; --q) {
                    const uint32_t cf = cfs[q];
                    if (cf & STC_LAST) s = (2u * s + ((cf >> 17) & 1u)) & smask;
                    const uint32_t y = (uint32_t)(tks[q * wpp + (int)(s >> 6)] >> (s & 63u)) & 1u;
                    ys[q] = (uint8_t)y;
                    if (y) s ^= cf & 0xFFFFu;
                }
            }
            __syncthreads();
        }
        for (int q = tid; q < m; q += nthreads) {
            const long long pix = stc_pixel(pimg, lo + q, n);
            if (pix < 0) continue;
            const uint8_t xv = cimg[pix];
            uint8_t out = xv;
            if (good && ys[q] != (xv & 1)) {
                if (change == 0) {
                    out = xv ^ 1;
                } else {
                    const uint32_t u = word_of(philox4x32_10((uint32_t)(pix / 4), k0, k1), (int)(pix & 3));
                    const int d = xv == 0 ? 1 : xv == 255 ? -1 : (u & 1u) ? 1 : -1;
                    out = (uint8_t)((int)xv + d);
                }
                ++cnt;
            }
            simg[pix] = out;
        }
    }
    if (cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0) changes[nn] = total;
}

// ---- K42 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stc_extract_kernel(const uint8_t* __restrict__ stego, const uint32_t* __restrict__ cols,
                                                          const int32_t* __restrict__ path, uint8_t* __restrict__ message, long long n,
                                                          int k_uniform, int height, int plane, StcRagged rg) {
    const int nn = blockIdx.y;
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    const StcImage im = stc_image(rg, n, k_uniform, nn);
    const int k = im.k;
    if (b >= k) return;
    const uint8_t* simg = stego + (size_t)nn * n;
    const int32_t* pimg = path ? path + (size_t)nn * n : nullptr;
    uint32_t bit = 0;
    for (int r = 0; r < height && r <= b; ++r) {
        const long long i = b - r, start = i * n / k, end = (i + 1) * n / k;
        for (long long j = start; j < end; ++j) {
            if ((cols[j - start] >> r) & 1u) {
                const long long pix = stc_pixel(pimg, j, n);
                if (pix >= 0) bit ^= (simg[pix] >> plane) & 1u;
            }
        }
    }
    message[im.at + b] = (uint8_t)bit;
}

int stc_threads(int height) { return height <= 6 ? 64 : 1 << height; }

// K41 / K43 after their argument checks: the forward and the backward kernel of `phases`, with the uniform k or the ragged arguments
int stc_embed_launch(const uint8_t* cover, const double* rho, const uint8_t* message, const uint32_t* cols, const int32_t* path,
                     const uint64_t* seeds, int change, int height, int k, const StcRagged& rg, int phases, uint8_t* stego, double* cost,
                     long long* changes, uint8_t* ok, void* workspace, int n, long long hw, hipStream_t s) {
    unsigned long long* take = static_cast<unsigned long long*>(workspace);
    const int threads = stc_threads(height);
    if (phases & 1) {
        if (height <= 6)
            hipLaunchKernelGGL(stc_forward_kernel<true>, dim3(n), dim3(threads), 0, s, cover, rho, message, cols, path, take, cost, ok, hw, k, height, rg);
        else
            hipLaunchKernelGGL(stc_forward_kernel<false>, dim3(n), dim3(threads), 0, s, cover, rho, message, cols, path, take, cost, ok, hw, k, height, rg);
        const int rc = wsu_check_launch("stc_forward_kernel");
        if (rc) return rc;
    }
    if (phases & 2) {
        hipLaunchKernelGGL(stc_backward_kernel, dim3(n), dim3(threads), 0, s, cover, message, cols, path, seeds, take, cost, stego, changes, hw, k,
                           height, change, rg);
        return wsu_check_launch("stc_backward_kernel");
    }
    return 0;
}

}  // namespace

// (shapes: WSU_PATH_PIXELS, so path entries are int32 and the products (j + 1) * k stay below 2^62)
#define STC_REQUIRE_HEIGHT(what)                                                                                      \
    WSU_REQUIRE(height >= 1 && height <= STC_MAX_H, what ": constraint height %d outside 1..%d", height, STC_MAX_H)
#define STC_REQUIRE_CODE(what)                                                                                        \
    STC_REQUIRE_HEIGHT(what);                                                                                         \
    WSU_REQUIRE(k >= 1, what ": k=%d message bits, at least 1 expected", k);                                          \
    WSU_REQUIRE((long long)k <= (long long)h * w, what ": k=%d message bits exceed the %lld pixels", k, (long long)h * w)
// the host's part of the ragged arguments; what ks and first hold is checked by every workgroup (stc_image)
#define STC_REQUIRE_RAGGED(what)                                                                                      \
    WSU_REQUIRE(ks && first, what ": null ks or first");                                                              \
    WSU_REQUIRE(max_bits >= 1 && (long long)max_bits <= message_stride,                                               \
                what ": max_bits=%d outside 1..message_stride=%lld", max_bits, message_stride);                       \
    WSU_REQUIRE(cols_len >= 1, what ": cols_len=%d, at least 1 expected", cols_len)

extern "C" {

int wsu_philox_words(const uint64_t* seeds, uint32_t* words, int n, int h, int w, void* stream) {
    WSU_REQUIRE(seeds && words, "philox_words: null pointer");
    WSU_REQUIRE_SHAPE("philox_words", WSU_COUNTER_PIXELS, "counters");
    const long long hw = (long long)h * w, blocks = (hw / 4 + 255) / 256;
    hipLaunchKernelGGL(philox_words_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 256 ? 256 : blocks), n), dim3(256), 0,
                       static_cast<hipStream_t>(stream), seeds, words, hw);
    return wsu_check_launch("philox_words_kernel");
}

size_t wsu_stc_workspace_bytes(long long pixels, int height) {
    if (pixels <= 0 || height < 1 || height > STC_MAX_H) return 0;
    return (size_t)pixels * (size_t)(stc_threads(height) / 8);                 // one ballot word per wave and position
}

int wsu_stc_embed(const uint8_t* cover, const double* rho, const uint8_t* message, const uint32_t* cols, const int32_t* path,
                  const uint64_t* seeds, int change, int height, int k, int phases, uint8_t* stego, double* cost, long long* changes,
                  uint8_t* ok, void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(cover && rho && message && cols && seeds && stego && cost && changes && ok && workspace, "stc_embed: null pointer");
    WSU_REQUIRE_SHAPE("stc_embed", WSU_PATH_PIXELS, "path");
    STC_REQUIRE_CODE("stc_embed");
    WSU_REQUIRE(change == 0 || change == 1, "stc_embed: change=%d is neither 0 (flip) nor 1 (pm1)", change);
    WSU_REQUIRE(phases >= 1 && phases <= 3, "stc_embed: phases=%d outside 1..3 (1 forward, 2 backward, 3 both)", phases);
    const long long hw = (long long)h * w;
    WSU_REQUIRE(workspace_bytes >= (size_t)n * wsu_stc_workspace_bytes(hw, height), "stc_embed: workspace too small");
    WSU_REQUIRE((uintptr_t)workspace % 8 == 0, "stc_embed: workspace must be 8-byte aligned");
    return stc_embed_launch(cover, rho, message, cols, path, seeds, change, height, k, StcRagged{nullptr, nullptr, 0, 0, 0}, phases, stego, cost,
                            changes, ok, workspace, n, hw, static_cast<hipStream_t>(stream));
}

int wsu_stc_extract(const uint8_t* stego, const uint32_t* cols, const int32_t* path, int height, int k, uint8_t* message, int n, int h,
                    int w, void* stream) {
    WSU_REQUIRE(stego && cols && message, "stc_extract: null pointer");
    WSU_REQUIRE_SHAPE("stc_extract", WSU_PATH_PIXELS, "path");
    STC_REQUIRE_CODE("stc_extract");
    hipLaunchKernelGGL(stc_extract_kernel, dim3((unsigned)((k + 255) / 256), n), dim3(256), 0, static_cast<hipStream_t>(stream), stego, cols,
                       path, message, (long long)h * w, k, height, 0, StcRagged{nullptr, nullptr, 0, 0, 0});
    return wsu_check_launch("stc_extract_kernel");
}

int wsu_stc_embed_ragged(const uint8_t* cover, const double* rho, const uint8_t* message, long long message_stride, const int32_t* ks,
                         const int32_t* first, int max_bits, const uint32_t* cols, int cols_len, const int32_t* path, const uint64_t* seeds,
                         int change, int height, uint8_t* stego, double* cost, long long* changes, uint8_t* ok, void* workspace,
                         size_t workspace_bytes, int n, int h, int w, void* stream) {
    WSU_REQUIRE(cover && rho && message && cols && seeds && stego && cost && changes && ok && workspace, "stc_embed_ragged: null pointer");
    WSU_REQUIRE_SHAPE("stc_embed_ragged", WSU_PATH_PIXELS, "path");
    STC_REQUIRE_HEIGHT("stc_embed_ragged");
    STC_REQUIRE_RAGGED("stc_embed_ragged");
    WSU_REQUIRE(change == 0 || change == 1, "stc_embed_ragged: change=%d is neither 0 (flip) nor 1 (pm1)", change);
    const long long hw = (long long)h * w;
    WSU_REQUIRE(workspace_bytes >= (size_t)n * wsu_stc_workspace_bytes(hw, height), "stc_embed_ragged: workspace too small");
    WSU_REQUIRE((uintptr_t)workspace % 8 == 0, "stc_embed_ragged: workspace must be 8-byte aligned");
    return stc_embed_launch(cover, rho, message, cols, path, seeds, change, height, 0, StcRagged{ks, first, message_stride, max_bits, cols_len}, 3,
                            stego, cost, changes, ok, workspace, n, hw, static_cast<hipStream_t>(stream));
}

int wsu_stc_extract_ragged(const uint8_t* stego, const uint32_t* cols, int cols_len, const int32_t* path, int height, int bit,
                           const int32_t* ks, const int32_t* first, int max_bits, uint8_t* message, long long message_stride, int n, int h,
                           int w, void* stream) {
    WSU_REQUIRE(stego && cols && message, "stc_extract_ragged: null pointer");
    WSU_REQUIRE_SHAPE("stc_extract_ragged", WSU_PATH_PIXELS, "path");
    STC_REQUIRE_HEIGHT("stc_extract_ragged");
    STC_REQUIRE_RAGGED("stc_extract_ragged");
    WSU_REQUIRE(bit >= 0 && bit <= 7, "stc_extract_ragged: bit=%d outside 0..7", bit);
    const long long hw = (long long)h * w;
    const long long most = max_bits < hw ? max_bits : hw;                        // no image has more bits than pixels
    hipLaunchKernelGGL(stc_extract_kernel, dim3((unsigned)((most + 255) / 256), n), dim3(256), 0, static_cast<hipStream_t>(stream), stego, cols,
                       path, message, hw, 0, height, bit, StcRagged{ks, first, message_stride, max_bits, cols_len});
    return wsu_check_launch("stc_extract_kernel");
}

}  // extern "C"
