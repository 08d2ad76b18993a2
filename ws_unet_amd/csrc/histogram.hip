// K58 - K60: the counting halves of the histogram attacks (ws_unet_amd/histogram.py): the chi-square attack on the pairs of values
// (Westfeld, Pfitzmann, IH 1999) and the histogram characteristic function centre of mass (Harmsen, Pearlman 2003) with Ker's calibrated
// and adjacency variants (IEEE SPL 12(6), 2005).  Not part of the reference.
//
//   K58  table[n][s][v] = #{(r,c): x[r][c] = v, floor(t S / (H W)) = s},  t = r W + c (order 0, 'rows') or (H-1-r) W + c (order 1, 'rows_up'):
//        the histogram of each of S consecutive segments of the path; S = 1 is the plain histogram.
//   K59  A[n][u][v] = #{(r,c): c + 1 < W, x[r][c] = u, x[r][c+1] = v}: the horizontal adjacency histogram.
//   K60  y[n][r][c] = (x[2r][2c] + x[2r][2c+1] + x[2r+1][2c] + x[2r+1][2c+1]) >> 2: Ker's calibration image.
//
// K58 and K59 are count kernels in the convention of wsu_count.h: the entry zeroes the table on the stream, a workgroup counts into LDS and
// adds every non-zero sum with one 64-bit vector atomic, so the bits depend on no order.  What both do about a constant plane, whose every
// update hits one LDS address (same-address LDS atomics serialise: profiles/r22, r29): the hot bin is not known beforehand as it is in K25 /
// K36, so HotBins' fixed fields do not fit.  A thread walks 16 consecutive pixels and adds a RUN of equal bins with one atomic, and where the
// runs that the lanes of a wave still hold at the end of their 16 pixels are all of one bin, the wave adds their sum once (wave_emit).
//
// K58: a workgroup owns HS_CHUNK consecutive path positions and walks the segments that cross them one after another: it counts the
// positions of one segment into a 256-bin histogram per wave, flushes it to that segment's row and goes on, so LDS is never indexed by s and
// S does not bound the LDS.  Two 64-bit divisions per segment piece, none per pixel.  The price is paid at large S: a pass has two barriers and
// a 256-thread flush whatever the segment's length, so at S = 4096 on 512 x 512 planes (segments of 64 pixels, 128 passes per workgroup, 4 of
// its 256 threads busy) the kernel takes 18 - 27 x its time at S = 100; the curve's S = 100 is what it is built for.
//
// K59: 65 536 bins as 16-bit fields, two to a word: 128 KiB of LDS, one workgroup of 1 024 threads per CU.  A workgroup's tile has at most
// AH_ROWS * CT_COLS = 49 152 pairs, so no field can carry into its neighbour even when one bin takes them all.  There is no data-dependent
// path: a pair's bin is u * 256 + v wherever it lies.  DESIGN.md section 4-hist has the readings and says why the banded layout was not built.
#include "wsu_count.h"

namespace {

// the run (bin, cnt) that each lane of the wave still holds (cnt 0: none): ONE add(bin, sum) where all of them are of one bin, else one per
// lane.  Every lane of the wave must get here.
template <class Add> __device__ __forceinline__ void wave_emit(int bin, uint32_t cnt, Add add) {
    const unsigned long long have = __ballot(cnt != 0u);
    if (!have) return;
    const int b0 = __shfl(bin, __ffsll(have) - 1, 64);
    if (__all(cnt == 0u || bin == b0)) {
        const uint32_t s = wave_sum(cnt);
        if ((threadIdx.x & 63) == 0) add(b0, s);
    } else if (cnt) {
        add(bin, cnt);
    }
}

// ---- K58 -------------------------------------------------------------------------------------------------------------------------------------
constexpr int HS_THREADS = 256, HS_WAVES = HS_THREADS / 64, HS_BINS = 256, HS_CHUNK = 2 * 16 * HS_THREADS;      // 8 192 positions per workgroup
static_assert(HS_THREADS == HS_BINS, "the flush gives every thread one bin");

// the pixels at the path positions p .. p + 15 of the plane (p < hw; positions from hw on repeat an earlier pixel and are never counted)
__device__ __forceinline__ u32x4 hs_load_unit(const uint8_t* __restrict__ img, unsigned long long p, unsigned long long hw, int h, int w, int order) {
    const int rem = (int)min(hw - p, 16ull);
    if (order == 0) return ct_load_strip(img + p, rem);
    const uint32_t r = (uint32_t)p / (uint32_t)w, c = (uint32_t)p - r * (uint32_t)w;        // hw < 2^32 (the entry checks)
    if (c + 16u <= (uint32_t)w) return ct_load_strip(img + (size_t)(h - 1 - (int)r) * w + c, 16);
    uint32_t v[4] = {0u, 0u, 0u, 0u};                                                       // the unit crosses a row end: pixel by pixel
    for (int i = 0; i < rem; ++i) {
        const uint32_t pi = (uint32_t)p + i, ri = pi / (uint32_t)w, ci = pi - ri * (uint32_t)w;
        v[i >> 2] |= (uint32_t)img[(size_t)(h - 1 - (int)ri) * w + ci] << (8 * (i & 3));
    }
    return mk_u4(v[0], v[1], v[2], v[3]);
}

__global__ __launch_bounds__(HS_THREADS) void hist_segments_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ table,
                                                                   int h, int w, int segments, int order) {
    __shared__ uint32_t hist[HS_WAVES][HS_BINS];
    const int tid = threadIdx.x, wave = tid >> 6;
    const unsigned long long hw = (unsigned long long)h * w, S = (unsigned long long)segments;
    const unsigned long long t0 = (unsigned long long)blockIdx.x * HS_CHUNK, t1 = min(t0 + HS_CHUNK, hw);
    const uint8_t* img = xu8 + (size_t)blockIdx.y * hw;
    unsigned long long* out = table + (size_t)blockIdx.y * S * HS_BINS;
    uint32_t* hwv = hist[wave];
#pragma unroll
    for (int j = 0; j < HS_WAVES; ++j) hist[j][tid] = 0u;
    __syncthreads();
    unsigned long long cur = t0;
#pragma unroll 1
    while (cur < t1) {                                                                      // uniform: one pass per segment that crosses the chunk
        const unsigned long long s = cur * S / hw;                                          // cur < 2^32, S <= 4096
        const unsigned long long e = min(t1, ((s + 1) * hw + S - 1) / S);                   // the first position of segment s + 1; > cur
#pragma unroll 1
        for (unsigned long long base = t0 + ((cur - t0) & ~15ull); base < e; base += 16ull * HS_THREADS) {
            const unsigned long long p = base + 16ull * tid;                                // this thread's unit: positions p .. p + 15
            const int a = (int)(max(cur, p) - p), b = p < e ? (int)(min(e, p + 16) - p) : 0;
            const uint32_t m = b > a ? ((1u << b) - 1u) & ~((1u << a) - 1u) : 0u;           // bit i: position p + i is in cur .. e - 1
            int bin = 0;
            uint32_t cnt = 0u;
            if (m) {
                const u32x4 px = hs_load_unit(img, p, hw, h, w, order);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int v = ct_px(px, i);
                    if ((m >> i) & 1u) {
                        if (cnt && v == bin) {
                            ++cnt;
                        } else {
                            if (cnt) atomicAdd(&hwv[bin], cnt);
                            bin = v;
                            cnt = 1u;
                        }
                    }
                }
            }
            wave_emit(bin, cnt, [&](int b_, uint32_t c_) { atomicAdd(&hwv[b_], c_); });
        }
        __syncthreads();
        uint32_t sum = 0u;
#pragma unroll
        for (int j = 0; j < HS_WAVES; ++j) { sum += hist[j][tid]; hist[j][tid] = 0u; }
        if (sum) atomicAdd(&out[s * HS_BINS + tid], (unsigned long long)sum);
        __syncthreads();
        cur = e;
    }
}

// ---- K59 -------------------------------------------------------------------------------------------------------------------------------------
constexpr int AH_THREADS = 1024, AH_GROUPS = AH_THREADS / CT_STRIPS, AH_TRT = 3, AH_ROWS = AH_GROUPS * AH_TRT;   // a tile of 96 x 512 pixels
constexpr int AH_BINS = 256 * 256, AH_WORDS = AH_BINS / 2, AH_LDS = AH_WORDS * (int)sizeof(uint32_t);
static_assert((long long)AH_ROWS * CT_COLS <= 65535, "a 16-bit field must hold every pair of the tile");
static_assert(AH_LDS <= WSU_LDS_CU, "the packed table must fit a CU's LDS");

__device__ __forceinline__ void ah_add(uint32_t* __restrict__ packed, int bin, uint32_t cnt) { atomicAdd(&packed[bin >> 1], cnt << (16 * (bin & 1))); }

__global__ __launch_bounds__(AH_THREADS) void adjacency_hist_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ table,
                                                                    int h, int w, int tiles_c) {
    extern __shared__ uint32_t packed[];                // [AH_WORDS]: bin b in bits 16 (b & 1) .. of word b >> 1
    const int nn = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < AH_WORDS / 4; i += AH_THREADS) reinterpret_cast<u32x4*>(packed)[i] = mk_u4(0u, 0u, 0u, 0u);
    __syncthreads();
    const long long c = (long long)(blockIdx.x % tiles_c) * CT_COLS + (tid & (CT_STRIPS - 1)) * 16;
    const long long r0 = (long long)(blockIdx.x / tiles_c) * AH_ROWS + (tid / CT_STRIPS) * AH_TRT;
    const int rem = (int)min(max((long long)w - c, 0ll), 17ll);          // pixels of the row from c on, capped at the strip and its right neighbour
    const uint8_t* img = xu8 + (size_t)nn * h * w + c;
    const uint32_t pairs = (1u << max(rem - 1, 0)) - 1u;                 // bit i: pixel c + i has a right neighbour in the row
#pragma unroll 1
    for (int k = 0; k < AH_TRT; ++k) {
        const long long r = r0 + k;
        const bool row_in = rem > 1 && r < h;
        u32x4 cur = mk_u4(0u, 0u, 0u, 0u);
        int right = 0;
        if (row_in) {
            cur = ct_load_strip(img + (size_t)r * w, min(rem, 16));
            if (rem > 16) right = (int)img[(size_t)r * w + 16];
        }
        const uint32_t m = row_in ? pairs : 0u;
        int bin = 0;
        uint32_t cnt = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int b = ct_px(cur, i) * 256 + (i < 15 ? ct_px(cur, i + 1) : right);
            if ((m >> i) & 1u) {
                if (cnt && b == bin) {
                    ++cnt;
                } else {
                    if (cnt) ah_add(packed, bin, cnt);
                    bin = b;
                    cnt = 1u;
                }
            }
        }
        wave_emit(bin, cnt, [&](int b_, uint32_t c_) { ah_add(packed, b_, c_); });
    }
    __syncthreads();
    unsigned long long* out = table + (size_t)nn * AH_BINS;
    for (int i = tid; i < AH_WORDS; i += AH_THREADS) {
        const uint32_t wd = packed[i];
        if (wd & 0xffffu) atomicAdd(&out[2 * i], (unsigned long long)(wd & 0xffffu));
        if (wd >> 16) atomicAdd(&out[2 * i + 1], (unsigned long long)(wd >> 16));
    }
}

// ---- K60 -------------------------------------------------------------------------------------------------------------------------------------
constexpr int DS_THREADS = 256, DS_ROWS = DS_THREADS / 64, DS_COLS = 64 * 4;            // a workgroup: 4 output rows of 64 threads x 4 pixels

__global__ __launch_bounds__(DS_THREADS) void downsample2x2_kernel(const uint8_t* __restrict__ xu8, uint8_t* __restrict__ y, int h, int w, int ho,
                                                                   int wo, int tiles_c) {
    const long long co = (long long)(blockIdx.x % tiles_c) * DS_COLS + (threadIdx.x & 63) * 4;
    const long long ro = (long long)(blockIdx.x / tiles_c) * DS_ROWS + (threadIdx.x >> 6);
    if (ro >= ho || co >= wo) return;
    const int cnt = (int)min((long long)wo - co, 4ll);
    const uint8_t* p0 = xu8 + (size_t)blockIdx.y * h * w + (size_t)(2 * ro) * w + 2 * co;
    const uint8_t* p1 = p0 + w;
    uint8_t* q = y + (size_t)blockIdx.y * ho * wo + (size_t)ro * wo + co;
    if (cnt == 4 && ((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1)) & 7) == 0 && (reinterpret_cast<uintptr_t>(q) & 3) == 0) {
        const u32x2 a = *reinterpret_cast<const u32x2*>(p0), b = *reinterpret_cast<const u32x2*>(p1);
        uint32_t o = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t wa = a[j >> 1] >> (16 * (j & 1)), wb = b[j >> 1] >> (16 * (j & 1));
            o |= (((wa & 255u) + ((wa >> 8) & 255u) + (wb & 255u) + ((wb >> 8) & 255u)) >> 2) << (8 * j);
        }
        *reinterpret_cast<uint32_t*>(q) = o;
    } else {
        for (int j = 0; j < cnt; ++j) q[j] = (uint8_t)(((int)p0[2 * j] + p0[2 * j + 1] + p1[2 * j] + p1[2 * j + 1]) >> 2);
    }
}

}  // namespace

extern "C" {

int wsu_hist_segments(const uint8_t* x_u8, unsigned long long* table, int n, int h, int w, int segments, int order, void* stream) {
    WSU_REQUIRE(x_u8 && table, "hist_segments: null pointer");
    WSU_REQUIRE_SHAPE("hist_segments", WSU_COUNTER_PIXELS, "counters");
    WSU_REQUIRE(segments >= 1 && segments <= 4096, "hist_segments: segments=%d outside 1..4096", segments);
    WSU_REQUIRE(order == 0 || order == 1, "hist_segments: order=%d outside {0,1}", order);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(table, 0, (size_t)n * segments * HS_BINS * sizeof(unsigned long long), s) != hipSuccess) return wsu_check_launch("hist_segments memset");
    const long long chunks = ((long long)h * w + HS_CHUNK - 1) / HS_CHUNK;
    hipLaunchKernelGGL(hist_segments_kernel, dim3((unsigned)chunks, n), dim3(HS_THREADS), 0, s, x_u8, table, h, w, segments, order);
    return wsu_check_launch("hist_segments_kernel");
}

int wsu_adjacency_hist(const uint8_t* x_u8, unsigned long long* table, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && table, "adjacency_hist: null pointer");
    WSU_REQUIRE(n >= 1 && n <= 65535 && h >= 1 && w >= 1, "adjacency_hist: bad shape n=%d h=%d w=%d", n, h, w);
    static bool attr_done = false;     // benign race: idempotent
    if (!attr_done) {
        if (int rc = wsu_raise_lds(adjacency_hist_kernel, AH_LDS, "adjacency_hist")) return rc;
        attr_done = true;
    }
    return count_launch("adjacency_hist", "adjacency_hist memset", "adjacency_hist_kernel", adjacency_hist_kernel, AH_THREADS, AH_LDS, x_u8, table,
                        AH_BINS, n, h, w, 0, AH_ROWS, CT_COLS, stream);
}

int wsu_downsample2x2(const uint8_t* x_u8, uint8_t* y_u8, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && y_u8, "downsample2x2: null pointer");
    WSU_REQUIRE(n >= 1 && n <= 65535 && h >= 2 && w >= 2, "downsample2x2: bad shape n=%d h=%d w=%d (h, w >= 2)", n, h, w);
    const int ho = h / 2, wo = w / 2;
    const long long tr = ((long long)ho + DS_ROWS - 1) / DS_ROWS, tc = ((long long)wo + DS_COLS - 1) / DS_COLS;
    WSU_REQUIRE(tr * tc <= 0x7fffffffll, "downsample2x2: image of %d x %d has too many tiles", h, w);
    hipLaunchKernelGGL(downsample2x2_kernel, dim3((unsigned)(tr * tc), n), dim3(DS_THREADS), 0, static_cast<hipStream_t>(stream), x_u8, y_u8, h, w,
                       ho, wo, (int)tc);
    return wsu_check_launch("downsample2x2_kernel");
}

}  // extern "C"
