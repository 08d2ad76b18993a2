// K16-K18: the KB-stratified absolute-error box table, src/error_boxes.py `plot_error` (results/prediction/ae_boxes_3.csv):
//
//   AE per predictor  |y - x @ f| (filter, fp64)  or  |x - y*255| (network output, K10's float32 residual), interior [1:-1,1:-1],
//                     concatenated image-major over the test split (optionally subsampled per image, `subset_residual`)
//   slices            rank = position in the stable sort by (anchor AE, global index); c_j = #(anchor <= e_j);
//                     bound_j = c_j - 1 if 0 < c_j < N else N - 1 (the reference's `argmin(sorted <= e) - 1`, -1 as a slice bound);
//                     slice j = ranks [B_j, B_j+1) with B = (0, bound_0 .. bound_3, N)  (Python slicing, empty when B_j >= B_j+1)
//   statistics        per (predictor, slice): min, pandas `quantile(.25/.5/.75)` (numpy 'linear'), max -- the lerp and the IQR clip
//                     are done on the host in fp64 from the order statistics computed here.
//
// K16 writes one float32 key per pixel and predictor (exact: a dyadic filter's AE, or K10's float32 residual).  K17 reduces the anchor's
// keys to c_j, the key at rank c_j - 1 (the lexicographic maximum of (a, index) over a <= e_j) and the key at rank N - 1 (the global
// maximum), from which the host forms every slice as a pair of boundary keys: a pixel belongs to a slice iff its (a, index) lies
// between them, which also covers the reference's overlapping slices.  K18 is an exact multi-rank radix select over the float32 bit
// patterns (non-negative, so monotone as uint32), wsu_metric.h's 11/11/10-bit digits for every predictor x slice x rank at once: one pass over the
// keys per digit level (the rank's own prefix decides which keys count), then one pass for count(c <= a) and min(c > a), which gives
// c_(k+1) next to a = c_(k).  min and max are reductions of the first pass.  Counts are 32-bit inside a workgroup and 64-bit across
// workgroups, every cross-workgroup combination is an integer atomic (add / max), and results pass between kernels only at kernel
// boundaries: deterministic, and independent of how the keys were batched.
// numpy's float64 operation sequence for the filter residual: plain operators, no fused multiply-adds (wsu_metric.h)
#pragma clang fp contract(off)
#include "wsu_metric.h"

namespace {

constexpr int AE_THREADS = 256;
constexpr int AE_MAX_EDGES = 5;                 // K17
constexpr int AE_MAX_SLICES = AE_MAX_EDGES + 1; // K18
constexpr int AE_HIST_THREADS = 1024;           // K18's histogram passes (one workgroup may hold 144 KiB of LDS histograms)
constexpr int AE_RANKS = 3;                     // target ranks per slice (the three quantiles)
constexpr int AE_BINS = 2048;
constexpr int AE_MAX_PRED = 16;
constexpr int AE_STATE = 4;                     // u64 per (predictor, slice, rank): prefix bits, remaining rank, count(<= a), ~min(> a)

using DTaps = Taps3x3<double>;

// ---- K16 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AE_THREADS) void ae_values_kernel(const uint8_t* __restrict__ x, const float* __restrict__ xhat, float hat_scale,
                                                               int use_filter, DTaps taps, const long long* __restrict__ idx, int num_idx,
                                                               float* __restrict__ keys, uint32_t* __restrict__ flag, int h, int w) {
    const int nn = blockIdx.y;
    const long long ih = h - 2, iw = w - 2;
    const long long per = num_idx > 0 ? num_idx : ih * iw;
    const long long j = (long long)blockIdx.x * AE_THREADS + threadIdx.x;
    if (j >= per) return;
    long long q = j;
    if (num_idx > 0) {
        q = idx[(size_t)nn * num_idx + j];
        if (q < 0 || q >= ih * iw) {                 // the host draws q in [0, ih*iw); anything else is reported, never read
            atomicOr(flag, 2u);
            return;
        }
    }
    const int r = (int)(q / iw) + 1, c = (int)(q % iw) + 1;
    const uint8_t* img = x + (size_t)nn * h * w;
    float ae;
    if (use_filter) {
        // get_filter_residuals: y - x @ filter in float64 (filters/evaluate.py:53-76); exact for the dyadic taps the host admits
        ae = (float)fabs((double)img[(size_t)r * w + c] - filter_hat64<false>(taps, img, r, c, w));
    } else {
        // K10's float32 residual x - float32(y*255), the product rounded before the subtraction; x_hat is full-frame here
        ae = fabsf(residual_f32((float)img[(size_t)r * w + c], xhat[hat_index(1, hat_base(1, nn, h, w), r, c, w)], hat_scale));
    }
    if (!(ae <= 3.402823466e38f)) atomicOr(flag, 1u); // NaN or +inf
    keys[(size_t)nn * per + j] = ae;
}

// key bits: non-negative floats order as uint32; -0 is 0
__device__ __forceinline__ uint32_t ae_bits(const float* __restrict__ p, size_t i) {
    const uint32_t u = __float_as_uint(p[i]);
    return u == 0x80000000u ? 0u : u;
}

// ---- K17 ------------------------------------------------------------------------------------------------------------------
struct Edges { double e[AE_MAX_EDGES]; int ne; };
// out: [ne + 1][3] u64 {count, max bits, max index + 1}; row ne is the global maximum (its count slot stays 0: the caller knows N)

__global__ __launch_bounds__(AE_THREADS) void ae_slices_count_kernel(const float* __restrict__ a, long long count, Edges ed,
                                                                     unsigned long long* __restrict__ out) {
    __shared__ uint32_t lc[AE_MAX_EDGES + 1], lm[AE_MAX_EDGES + 1];
    const int tid = threadIdx.x;
    if (tid <= AE_MAX_EDGES) { lc[tid] = 0u; lm[tid] = 0u; }
    __syncthreads();
    uint32_t cnt[AE_MAX_EDGES] = {}, mx[AE_MAX_EDGES + 1] = {};
    for (size_t i = (size_t)blockIdx.x * AE_THREADS + tid; i < (size_t)count; i += (size_t)gridDim.x * AE_THREADS) {
        const uint32_t u = ae_bits(a, i);
        const double v = (double)__uint_as_float(u);
#pragma unroll
        for (int j = 0; j < AE_MAX_EDGES; ++j)
            if (j < ed.ne && v <= ed.e[j]) { ++cnt[j]; mx[j] = max(mx[j], u); }
        mx[AE_MAX_EDGES] = max(mx[AE_MAX_EDGES], u);
    }
#pragma unroll
    for (int j = 0; j < AE_MAX_EDGES; ++j)
        if (j < ed.ne) { if (cnt[j]) atomicAdd(&lc[j], cnt[j]); atomicMax(&lm[j], mx[j]); }
    atomicMax(&lm[AE_MAX_EDGES], mx[AE_MAX_EDGES]);
    __syncthreads();
    if (tid < ed.ne) {
        if (lc[tid]) atomicAdd(&out[tid * 3 + 0], (unsigned long long)lc[tid]);
        atomicMax(&out[tid * 3 + 1], (unsigned long long)lm[tid]);
    } else if (tid == AE_MAX_EDGES) {
        atomicMax(&out[ed.ne * 3 + 1], (unsigned long long)lm[AE_MAX_EDGES]);
    }
}

// the largest index among the keys equal to each maximum: the lexicographic maximum of (a, index)
__global__ __launch_bounds__(AE_THREADS) void ae_slices_index_kernel(const float* __restrict__ a, long long count, Edges ed,
                                                                     unsigned long long* __restrict__ out) {
    __shared__ unsigned long long li[AE_MAX_EDGES + 1];
    const int tid = threadIdx.x;
    if (tid <= AE_MAX_EDGES) li[tid] = 0ull;
    __syncthreads();
    uint32_t mb[AE_MAX_EDGES + 1];
#pragma unroll
    for (int j = 0; j < AE_MAX_EDGES; ++j) mb[j] = j < ed.ne ? (uint32_t)out[j * 3 + 1] : 0u;
    mb[AE_MAX_EDGES] = (uint32_t)out[ed.ne * 3 + 1];
    unsigned long long ix[AE_MAX_EDGES + 1] = {};
    for (size_t i = (size_t)blockIdx.x * AE_THREADS + tid; i < (size_t)count; i += (size_t)gridDim.x * AE_THREADS) {
        const uint32_t u = ae_bits(a, i);
        const double v = (double)__uint_as_float(u);
#pragma unroll
        for (int j = 0; j < AE_MAX_EDGES; ++j)
            if (j < ed.ne && v <= ed.e[j] && u == mb[j]) ix[j] = i + 1;          // i grows along the loop: the last hit is the largest
        if (u == mb[AE_MAX_EDGES]) ix[AE_MAX_EDGES] = i + 1;
    }
#pragma unroll
    for (int j = 0; j <= AE_MAX_EDGES; ++j)
        if (ix[j]) atomicMax(&li[j], ix[j]);
    __syncthreads();
    if (tid < ed.ne) {
        if (li[tid]) atomicMax(&out[tid * 3 + 2], li[tid]);
    } else if (tid == AE_MAX_EDGES) {
        if (li[AE_MAX_EDGES]) atomicMax(&out[ed.ne * 3 + 2], li[AE_MAX_EDGES]);
    }
}

// ---- K18 ------------------------------------------------------------------------------------------------------------------
// A slice as the pair of boundary keys the host formed from K17: lo <= (a, index) < hi, each bound optional; size 0 = empty.
struct Slices {
    uint32_t lo_bits[AE_MAX_SLICES], hi_bits[AE_MAX_SLICES];
    unsigned long long lo_idx[AE_MAX_SLICES], hi_idx[AE_MAX_SLICES];
    long long size[AE_MAX_SLICES], rank[AE_MAX_SLICES][AE_RANKS];
    int has_lo[AE_MAX_SLICES], has_hi[AE_MAX_SLICES];
    int ns;
};

__device__ __forceinline__ uint32_t ae_member(const Slices& s, uint32_t a, unsigned long long i) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < AE_MAX_SLICES; ++j) {
        if (j >= s.ns || s.size[j] == 0) continue;
        const bool lo = !s.has_lo[j] || a > s.lo_bits[j] || (a == s.lo_bits[j] && i >= s.lo_idx[j]);
        const bool hi = !s.has_hi[j] || a < s.hi_bits[j] || (a == s.hi_bits[j] && i < s.hi_idx[j]);
        if (lo && hi) m |= 1u << j;
    }
    return m;
}

struct AeWs {
    unsigned long long* hist;                   // [3 levels][P][AE_MAX_SLICES][AE_RANKS][AE_BINS]  (level 0 uses rank slot 0)
    unsigned long long* state;                  // [P][AE_MAX_SLICES][AE_RANKS][AE_STATE]
    unsigned long long* minmax;                 // [P][AE_MAX_SLICES][2]  {~min bits, max bits} (both by atomicMax; 0 = none)
};

__host__ __device__ __forceinline__ size_t ae_hist_words(int np) { return (size_t)3 * np * AE_MAX_SLICES * AE_RANKS * AE_BINS; }
__host__ __device__ __forceinline__ size_t ae_state_words(int np) { return (size_t)np * AE_MAX_SLICES * AE_RANKS * AE_STATE; }

__device__ __forceinline__ AeWs ae_ws(void* ws, int np) {
    AeWs p;
    p.hist = static_cast<unsigned long long*>(ws);
    p.state = p.hist + ae_hist_words(np);
    p.minmax = p.state + ae_state_words(np);
    return p;
}

__device__ __forceinline__ unsigned long long* ae_hist_row(const AeWs& p, int np, int level, int pred, int j, int t) {
    return p.hist + ((((size_t)level * np + pred) * AE_MAX_SLICES + j) * AE_RANKS + t) * AE_BINS;
}

__device__ __forceinline__ unsigned long long* ae_state(const AeWs& p, int pred, int j, int t) {
    return p.state + (((size_t)pred * AE_MAX_SLICES + j) * AE_RANKS + t) * AE_STATE;
}

// One digit level, one pass over the keys for every slice and rank: grid (parts, P).  Level 0 has no prefix yet, so its histogram is
// shared by the ranks of a slice, and the pass also reduces min / max and screens the keys; levels 1 and 2 keep one histogram per
// (slice, rank), each counting the keys that match that rank's prefix.  Dynamic LDS: ns x AE_BINS u32 at level 0, ns x AE_RANKS x
// bins u32 at levels 1 (2 048 bins: up to 144 KiB) and 2 (1 024 bins: up to 72 KiB) -- a workgroup can fill most of a CU's 160 KiB,
// so it has AE_HIST_THREADS (16 waves) to keep its loads in flight.
__global__ __launch_bounds__(AE_HIST_THREADS) void ae_select_hist_kernel(const float* __restrict__ keys, size_t stride, int np, int anchor,
                                                                         long long count, Slices sl, int level, void* __restrict__ workspace,
                                                                         uint32_t* __restrict__ flags) {
    extern __shared__ uint32_t lh[];
    __shared__ uint32_t lmin[AE_MAX_SLICES], lmax[AE_MAX_SLICES], lbad;
    const int tid = threadIdx.x, pred = blockIdx.y;
    const AeWs p = ae_ws(workspace, np);
    const RadixDigit dg = radix_digit(level);
    const int nr = level == 0 ? 1 : AE_RANKS;                // histograms per slice
    const int nb = sl.ns * nr * dg.bins;
    uint32_t prefix[AE_MAX_SLICES][AE_RANKS];
#pragma unroll
    for (int j = 0; j < AE_MAX_SLICES; ++j)
#pragma unroll
        for (int t = 0; t < AE_RANKS; ++t)
            prefix[j][t] = (level > 0 && j < sl.ns && sl.size[j] > 0) ? (uint32_t)ae_state(p, pred, j, t)[0] : 0u;
    for (int b = tid; b < nb; b += AE_HIST_THREADS) lh[b] = 0u;
    if (tid < AE_MAX_SLICES) { lmin[tid] = 0u; lmax[tid] = 0u; }
    if (tid == 0) lbad = 0u;
    __syncthreads();
    const float* kp = keys + (size_t)pred * stride;
    const float* ka = keys + (size_t)anchor * stride;
    uint32_t mn[AE_MAX_SLICES] = {}, mx[AE_MAX_SLICES] = {}, bad = 0u;
    for (size_t i = (size_t)blockIdx.x * AE_HIST_THREADS + tid; i < (size_t)count; i += (size_t)gridDim.x * AE_HIST_THREADS) {
        const uint32_t u = ae_bits(kp, i);
        const uint32_t m = ae_member(sl, pred == anchor ? u : ae_bits(ka, i), i);
        const uint32_t digit = (u >> dg.shift) & (dg.bins - 1);
        if (level == 0) {
            bad |= (u >> 31) | ((u & 0x7F800000u) == 0x7F800000u ? 1u : 0u);
#pragma unroll
            for (int j = 0; j < AE_MAX_SLICES; ++j) {
                if (!((m >> j) & 1u)) continue;
                atomicAdd(&lh[j * AE_BINS + digit], 1u);
                mn[j] = max(mn[j], ~u);
                mx[j] = max(mx[j], u);
            }
        } else {
#pragma unroll
            for (int j = 0; j < AE_MAX_SLICES; ++j) {
                if (!((m >> j) & 1u)) continue;
#pragma unroll
                for (int t = 0; t < AE_RANKS; ++t)
                    if ((u & dg.mask) == prefix[j][t]) atomicAdd(&lh[(j * AE_RANKS + t) * dg.bins + digit], 1u);
            }
        }
    }
    if (level == 0) {
#pragma unroll
        for (int j = 0; j < AE_MAX_SLICES; ++j)
            if (mn[j]) { atomicMax(&lmin[j], mn[j]); atomicMax(&lmax[j], mx[j]); }
        if (bad) atomicOr(&lbad, 1u);
    }
    __syncthreads();
    for (int b = tid; b < nb; b += AE_HIST_THREADS) {
        const int hh = b / dg.bins, bin = b % dg.bins;           // hh = j * nr + t
        if (lh[b]) atomicAdd(&ae_hist_row(p, np, level, pred, hh / nr, hh % nr)[bin], (unsigned long long)lh[b]);
    }
    if (level == 0 && tid < sl.ns && lmin[tid]) {
        atomicMax(&p.minmax[((size_t)pred * AE_MAX_SLICES + tid) * 2 + 0], (unsigned long long)lmin[tid]);
        atomicMax(&p.minmax[((size_t)pred * AE_MAX_SLICES + tid) * 2 + 1], (unsigned long long)lmax[tid]);
    }
    if (level == 0 && tid == 0 && lbad) atomicOr(&flags[pred], 1u);
}

// one workgroup per (predictor, slice, rank): the bin that holds the remaining rank, by a fixed-order scan of the 64-bit histogram
__global__ __launch_bounds__(AE_THREADS) void ae_select_pick_kernel(int np, Slices sl, int level, void* __restrict__ workspace) {
    __shared__ unsigned long long part[AE_THREADS];
    const int tid = threadIdx.x;
    const int t = blockIdx.x % AE_RANKS, j = (blockIdx.x / AE_RANKS) % AE_MAX_SLICES, pred = blockIdx.x / (AE_RANKS * AE_MAX_SLICES);
    if (j >= sl.ns || sl.size[j] == 0) return;
    const AeWs p = ae_ws(workspace, np);
    unsigned long long* st = ae_state(p, pred, j, t);
    radix_pick<unsigned long long>(ae_hist_row(p, np, level, pred, j, level == 0 ? 0 : t), st,
                                   level == 0 ? (unsigned long long)sl.rank[j][t] : st[1], level, part, tid);
}

// count(c <= a) and max(~c) over c > a within each slice, for every rank's a = c_(k): grid (parts, P)
__global__ __launch_bounds__(AE_THREADS) void ae_select_next_kernel(const float* __restrict__ keys, size_t stride, int np, int anchor,
                                                                    long long count, Slices sl, void* __restrict__ workspace) {
    __shared__ uint32_t lc[AE_MAX_SLICES][AE_RANKS], lm[AE_MAX_SLICES][AE_RANKS];
    const int tid = threadIdx.x, pred = blockIdx.y;
    const AeWs p = ae_ws(workspace, np);
    uint32_t av[AE_MAX_SLICES][AE_RANKS];
#pragma unroll
    for (int j = 0; j < AE_MAX_SLICES; ++j)
#pragma unroll
        for (int t = 0; t < AE_RANKS; ++t) av[j][t] = (j < sl.ns && sl.size[j] > 0) ? (uint32_t)ae_state(p, pred, j, t)[0] : 0u;
    if (tid < AE_MAX_SLICES * AE_RANKS) { lc[tid / AE_RANKS][tid % AE_RANKS] = 0u; lm[tid / AE_RANKS][tid % AE_RANKS] = 0u; }
    __syncthreads();
    const float* kp = keys + (size_t)pred * stride;
    const float* ka = keys + (size_t)anchor * stride;
    uint32_t cnt[AE_MAX_SLICES][AE_RANKS] = {}, mx[AE_MAX_SLICES][AE_RANKS] = {};
    for (size_t i = (size_t)blockIdx.x * AE_THREADS + tid; i < (size_t)count; i += (size_t)gridDim.x * AE_THREADS) {
        const uint32_t u = ae_bits(kp, i);
        const uint32_t m = ae_member(sl, pred == anchor ? u : ae_bits(ka, i), i);
#pragma unroll
        for (int j = 0; j < AE_MAX_SLICES; ++j) {
            if (!((m >> j) & 1u)) continue;
#pragma unroll
            for (int t = 0; t < AE_RANKS; ++t) {
                if (u <= av[j][t]) ++cnt[j][t];
                else mx[j][t] = max(mx[j][t], ~u);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < AE_MAX_SLICES; ++j)
#pragma unroll
        for (int t = 0; t < AE_RANKS; ++t) {
            if (cnt[j][t]) atomicAdd(&lc[j][t], cnt[j][t]);
            if (mx[j][t]) atomicMax(&lm[j][t], mx[j][t]);
        }
    __syncthreads();
    if (tid < AE_MAX_SLICES * AE_RANKS) {
        const int j = tid / AE_RANKS, t = tid % AE_RANKS;
        if (j < sl.ns && sl.size[j] > 0) {
            unsigned long long* st = ae_state(p, pred, j, t);
            if (lc[j][t]) atomicAdd(&st[2], (unsigned long long)lc[j][t]);
            if (lm[j][t]) atomicMax(&st[3], (unsigned long long)lm[j][t]);
        }
    }
}

// out[P][ns][8] u32 key bits: {min, max, c_(k0), c_(k0+1), c_(k1), c_(k1+1), c_(k2), c_(k2+1)} (c_(k+1) clamped to the slice's last)
__global__ __launch_bounds__(64) void ae_select_finish_kernel(int np, Slices sl, const void* __restrict__ workspace, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= np * sl.ns) return;
    const int pred = i / sl.ns, j = i % sl.ns;
    uint32_t* o = out + (size_t)i * 8;
    if (sl.size[j] == 0) {
        for (int q = 0; q < 8; ++q) o[q] = 0x7FC00000u;                       // NaN: an empty slice (the host writes a NaN row)
        return;
    }
    const AeWs p = ae_ws(const_cast<void*>(workspace), np);
    o[0] = ~(uint32_t)p.minmax[((size_t)pred * AE_MAX_SLICES + j) * 2 + 0];
    o[1] = (uint32_t)p.minmax[((size_t)pred * AE_MAX_SLICES + j) * 2 + 1];
    for (int t = 0; t < AE_RANKS; ++t) {
        const unsigned long long* st = ae_state(p, pred, j, t);
        o[2 + 2 * t] = (uint32_t)st[0];
        o[3 + 2 * t] = radix_next_bits((uint32_t)st[0], sl.rank[j][t], sl.size[j], (long long)st[2], (uint32_t)st[3]);
    }
}

int ae_parts(long long count) {
    const long long per = (long long)AE_THREADS * 64;
    const long long parts = (count + per - 1) / per;
    return (int)(parts < 1 ? 1 : parts > 1024 ? 1024 : parts);
}

}  // namespace

extern "C" {

int wsu_ae_values(const uint8_t* x_u8, const float* x_hat, const double* pixel_filter, float hat_scale, const long long* idx, int num_idx,
                  float* keys, size_t key_offset, size_t key_capacity, uint32_t* flag, int n, int h, int w, void* stream) {
    WSU_REQUIRE(x_u8 && keys && flag, "ae_values: null pointer");
    WSU_REQUIRE((x_hat != nullptr) != (pixel_filter != nullptr), "ae_values: give exactly one of x_hat / pixel_filter");
    WSU_REQUIRE(n > 0 && n <= 65535 && h >= 3 && w >= 3, "ae_values: bad shape n=%d h=%d w=%d", n, h, w);
    WSU_REQUIRE(num_idx >= 0 && (num_idx == 0) == (idx == nullptr), "ae_values: num_idx=%d does not match the index list", num_idx);
    const long long per = num_idx > 0 ? (long long)num_idx : (long long)(h - 2) * (w - 2);
    WSU_REQUIRE(key_offset <= key_capacity && (size_t)n * (size_t)per <= key_capacity - key_offset,
                "ae_values: %d x %lld keys at offset %zu exceed the key array of %zu", n, per, key_offset, key_capacity);
    const long long blocks = (per + AE_THREADS - 1) / AE_THREADS;
    WSU_REQUIRE(blocks <= 0x7FFFFFFFLL, "ae_values: %lld keys per image", per);
    const DTaps t = taps_from_weights(pixel_filter);
    hipLaunchKernelGGL(ae_values_kernel, dim3((unsigned)blocks, n), dim3(AE_THREADS), 0, static_cast<hipStream_t>(stream), x_u8, x_hat,
                       hat_scale, pixel_filter ? 1 : 0, t, idx, num_idx, keys + key_offset, flag, h, w);
    return wsu_check_launch("ae_values_kernel");
}

int wsu_ae_slices(const float* anchor_keys, long long count, const double* edges, int num_edges, unsigned long long* out, void* stream) {
    WSU_REQUIRE(anchor_keys && edges && out, "ae_slices: null pointer");
    WSU_REQUIRE(count > 0, "ae_slices: count=%lld", count);
    WSU_REQUIRE(num_edges >= 1 && num_edges <= AE_MAX_EDGES, "ae_slices: %d edges (1..%d)", num_edges, AE_MAX_EDGES);
    Edges ed{};
    ed.ne = num_edges;
    for (int j = 0; j < num_edges; ++j) ed.e[j] = edges[j];
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out, 0, (size_t)(num_edges + 1) * 3 * sizeof(unsigned long long), s) != hipSuccess)
        return wsu_check_launch("ae_slices memset");
    const int parts = ae_parts(count);
    hipLaunchKernelGGL(ae_slices_count_kernel, dim3(parts), dim3(AE_THREADS), 0, s, anchor_keys, count, ed, out);
    int rc = wsu_check_launch("ae_slices_count_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(ae_slices_index_kernel, dim3(parts), dim3(AE_THREADS), 0, s, anchor_keys, count, ed, out);
    return wsu_check_launch("ae_slices_index_kernel");
}

size_t wsu_ae_select_workspace_bytes(int num_pred) {
    return num_pred > 0 ? (ae_hist_words(num_pred) + ae_state_words(num_pred) + (size_t)num_pred * AE_MAX_SLICES * 2) * sizeof(unsigned long long)
                        : 0;
}

int wsu_ae_select(const float* keys, size_t stride, int num_pred, int anchor, long long count, const long long* slices, int num_slices,
                  uint32_t* out, uint32_t* flags, void* workspace, size_t workspace_bytes, void* stream) {
    WSU_REQUIRE(keys && slices && out && flags && workspace, "ae_select: null pointer");
    WSU_REQUIRE(num_pred >= 1 && num_pred <= AE_MAX_PRED, "ae_select: %d predictors (1..%d)", num_pred, AE_MAX_PRED);
    WSU_REQUIRE(anchor >= 0 && anchor < num_pred, "ae_select: anchor %d of %d predictors", anchor, num_pred);
    WSU_REQUIRE(count > 0 && (size_t)count <= stride, "ae_select: count=%lld, stride=%zu", count, stride);
    WSU_REQUIRE(num_slices >= 1 && num_slices <= AE_MAX_SLICES, "ae_select: %d slices (1..%d)", num_slices, AE_MAX_SLICES);
    WSU_REQUIRE(workspace_bytes >= wsu_ae_select_workspace_bytes(num_pred), "ae_select: workspace too small (%zu < %zu bytes)",
                workspace_bytes, wsu_ae_select_workspace_bytes(num_pred));
    Slices sl{};
    sl.ns = num_slices;
    for (int j = 0; j < num_slices; ++j) {
        const long long* d = slices + (size_t)j * 10;   // {size, has_lo, lo_bits, lo_idx, has_hi, hi_bits, hi_idx, k0, k1, k2}
        WSU_REQUIRE(d[0] >= 0 && d[0] <= count, "ae_select: slice %d of size %lld", j, d[0]);
        sl.size[j] = d[0];
        sl.has_lo[j] = d[1] ? 1 : 0;
        sl.lo_bits[j] = (uint32_t)d[2];
        sl.lo_idx[j] = (unsigned long long)d[3];
        sl.has_hi[j] = d[4] ? 1 : 0;
        sl.hi_bits[j] = (uint32_t)d[5];
        sl.hi_idx[j] = (unsigned long long)d[6];
        for (int t = 0; t < AE_RANKS; ++t) {
            WSU_REQUIRE(d[0] == 0 || (d[7 + t] >= 0 && d[7 + t] < d[0]), "ae_select: rank %lld outside slice %d of %lld", d[7 + t], j, d[0]);
            sl.rank[j][t] = d[7 + t];
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(workspace, 0, wsu_ae_select_workspace_bytes(num_pred), s) != hipSuccess) return wsu_check_launch("ae_select memset");
    if (hipMemsetAsync(flags, 0, (size_t)num_pred * sizeof(uint32_t), s) != hipSuccess) return wsu_check_launch("ae_select memset");
    static bool attr_done = false;     // benign race: idempotent
    if (!attr_done) {
        if (int rc = wsu_raise_lds(ae_select_hist_kernel, AE_MAX_SLICES * AE_RANKS * AE_BINS * (int)sizeof(uint32_t), "ae_select_hist")) return rc;
        attr_done = true;
    }
    const int parts = ae_parts(count);
    const long long hist_per = (long long)AE_HIST_THREADS * 32;
    const long long hist_parts = (count + hist_per - 1) / hist_per;
    const int hparts = (int)(hist_parts > 512 ? 512 : hist_parts);
    for (int level = 0; level < 3; ++level) {
        const size_t lds = (size_t)num_slices * (level == 0 ? 1 : AE_RANKS) * (level == 2 ? AE_BINS / 2 : AE_BINS) * sizeof(uint32_t);
        hipLaunchKernelGGL(ae_select_hist_kernel, dim3(hparts, num_pred), dim3(AE_HIST_THREADS), lds, s, keys, stride, num_pred, anchor,
                           count, sl, level, workspace, flags);
        int rc = wsu_check_launch("ae_select_hist_kernel");
        if (rc) return rc;
        hipLaunchKernelGGL(ae_select_pick_kernel, dim3(num_pred * AE_MAX_SLICES * AE_RANKS), dim3(AE_THREADS), 0, s, num_pred, sl, level,
                           workspace);
        rc = wsu_check_launch("ae_select_pick_kernel");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ae_select_next_kernel, dim3(parts, num_pred), dim3(AE_THREADS), 0, s, keys, stride, num_pred, anchor, count, sl,
                       workspace);
    int rc = wsu_check_launch("ae_select_next_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(ae_select_finish_kernel, dim3((num_pred * num_slices + 63) / 64), dim3(64), 0, s, num_pred, sl, workspace, out);
    return wsu_check_launch("ae_select_finish_kernel");
}

}  // extern "C"
