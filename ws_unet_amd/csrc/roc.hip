// K19: exact confusion counts of a threshold sweep, src/ws/roc.py `produce_roc` (results/detection/auc_*.csv, roc_*.csv):
//
//   TP_j = #{pos: s > tau_j}   FP_j = #{neg: s > tau_j}   TN_j = #{neg: s <= tau_j}   FN_j = #{pos: s <= tau_j}
//
// for G groups of float64 scores at once (numpy's comparisons: a NaN score is in none of the four, +-inf are ordinary scores).
// The taus are strictly ascending, so a score s falls in ONE bin b = #{tau_j < s} in [0, t]: s > tau_j iff j < b.  Pass 1 builds a
// (label, bin) histogram per group -- taus staged in LDS, a binary search per score, equal bins of a wave merged before the LDS add
// (clipped WS scores of cover sets put most lanes into bin 0), one 64-bit global atomic per non-empty LDS bin; pass 2 turns each
// group's histogram into FN_j = sum_{b <= j} pos[b], TN_j = sum_{b <= j} neg[b], TP_j = P - FN_j, FP_j = Nn - TN_j.  Integer atomics
// only and results pass between the kernels at a kernel boundary: deterministic and independent of how the scores were split.
#include <algorithm>

#include "wsu_device.h"

namespace {

constexpr int ROC_THREADS = 256;
constexpr int ROC_UNROLL = 4;                   // scores per thread and step: four loads in flight before the searches
constexpr int ROC_MAX_T = 4096;
constexpr int ROC_MAX_PARTS = 1024;

struct RocWs {
    double* taus;                               // [t]
    long long* offsets;                         // [groups + 1]
    unsigned long long* hist;                   // [groups][2][t + 1]: label 0 (negative), label 1 (positive)
};

__host__ __device__ __forceinline__ size_t roc_hist_words(int groups, int t) { return (size_t)groups * 2 * (size_t)(t + 1); }

__host__ __device__ __forceinline__ RocWs roc_ws(void* ws, int groups, int t) {
    RocWs p;
    p.taus = static_cast<double*>(ws);
    p.offsets = reinterpret_cast<long long*>(p.taus + t);
    p.hist = reinterpret_cast<unsigned long long*>(p.offsets + groups + 1);
    return p;
}

// #{tau_j < s} over the ascending taus in LDS (s not NaN)
__device__ __forceinline__ int roc_bin(const double* __restrict__ lt, int t, double s) {
    int lo = 0, n = t;
    while (n > 0) {
        const int half = n >> 1;
        if (lt[lo + half] < s) { lo += half + 1; n -= half + 1; }
        else n = half;
    }
    return lo;
}

// one LDS add per distinct key of the wave for the (up to) two most frequent keys it meets first, one per lane for the rest
__device__ __forceinline__ void roc_add(uint32_t* __restrict__ lh, int key) {
    const int lane = (int)__lane_id();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long live = __ballot(key >= 0);
        if (live == 0ull) return;
        const int lead = __ffsll((long long)live) - 1;
        const int k0 = __builtin_amdgcn_readlane(key, lead);
        const unsigned long long same = __ballot(key == k0);
        if (lane == lead) atomicAdd(&lh[k0], (uint32_t)__popcll(same));
        if (key == k0) key = -1;
    }
    if (key >= 0) atomicAdd(&lh[key], 1u);
}

// pass 1: grid (parts, groups); dynamic LDS = t doubles + 2 (t + 1) u32
__global__ __launch_bounds__(ROC_THREADS) void roc_hist_kernel(const double* __restrict__ scores, const signed char* __restrict__ labels,
                                                               int t, void* __restrict__ workspace, int groups) {
    extern __shared__ double roc_lds[];
    double* lt = roc_lds;
    uint32_t* lh = reinterpret_cast<uint32_t*>(roc_lds + t);
    const int tid = threadIdx.x, g = blockIdx.y;
    const RocWs p = roc_ws(workspace, groups, t);
    const long long begin = p.offsets[g], end = p.offsets[g + 1];
    if ((long long)blockIdx.x * ROC_THREADS * ROC_UNROLL >= end - begin) return;      // nothing for this workgroup (uniform)
    const int nb = 2 * (t + 1);
    for (int j = tid; j < t; j += ROC_THREADS) lt[j] = p.taus[j];
    for (int b = tid; b < nb; b += ROC_THREADS) lh[b] = 0u;
    __syncthreads();
    const long long step = (long long)gridDim.x * ROC_THREADS * ROC_UNROLL;
    for (long long base = begin + (long long)blockIdx.x * ROC_THREADS * ROC_UNROLL; base < end; base += step) {   // block-uniform trip count
        double s[ROC_UNROLL];
        int lab[ROC_UNROLL];
#pragma unroll
        for (int u = 0; u < ROC_UNROLL; ++u) {
            const long long i = base + u * ROC_THREADS + tid;
            const bool in = i < end;
            s[u] = in ? scores[i] : 0.0;
            lab[u] = in ? (int)labels[i] : -1;
        }
#pragma unroll
        for (int u = 0; u < ROC_UNROLL; ++u) {
            const bool valid = (lab[u] == 0 || lab[u] == 1) && !__builtin_isnan(s[u]);
            roc_add(lh, valid ? lab[u] * (t + 1) + roc_bin(lt, t, s[u]) : -1);
        }
    }
    __syncthreads();
    unsigned long long* gh = p.hist + (size_t)g * nb;
    for (int b = tid; b < nb; b += ROC_THREADS)
        if (lh[b]) atomicAdd(&gh[b], (unsigned long long)lh[b]);
}

// pass 2: one workgroup per group, a fixed-order scan of its 2 (t + 1) bins; counts[g][j] = {TP, FP, TN, FN}
__global__ __launch_bounds__(ROC_THREADS) void roc_scan_kernel(int t, int groups, const void* __restrict__ workspace,
                                                               long long* __restrict__ counts) {
    __shared__ unsigned long long part_n[ROC_THREADS], part_p[ROC_THREADS];
    const int tid = threadIdx.x, g = blockIdx.x;
    const RocWs p = roc_ws(const_cast<void*>(workspace), groups, t);
    const unsigned long long* hn = p.hist + (size_t)g * 2 * (t + 1);
    const unsigned long long* hp = hn + (t + 1);
    const int nb = t + 1, per = (nb + ROC_THREADS - 1) / ROC_THREADS;
    const int b0 = min(tid * per, nb), b1 = min(b0 + per, nb);
    unsigned long long sn = 0, sp = 0;
    for (int b = b0; b < b1; ++b) { sn += hn[b]; sp += hp[b]; }
    part_n[tid] = sn;
    part_p[tid] = sp;
    __syncthreads();
    unsigned long long cn = 0, cp = 0, tn = 0, tp = 0;                 // before this thread's bins / over all bins
    for (int q = 0; q < ROC_THREADS; ++q) {
        if (q < tid) { cn += part_n[q]; cp += part_p[q]; }
        tn += part_n[q];
        tp += part_p[q];
    }
    long long* out = counts + (size_t)g * t * 4;
    for (int b = b0; b < b1 && b < t; ++b) {
        cn += hn[b];
        cp += hp[b];
        out[(size_t)b * 4 + 0] = (long long)(tp - cp);               // TP: positives above tau_b
        out[(size_t)b * 4 + 1] = (long long)(tn - cn);               // FP
        out[(size_t)b * 4 + 2] = (long long)cn;                      // TN: negatives at or below tau_b
        out[(size_t)b * 4 + 3] = (long long)cp;                      // FN
    }
}

size_t roc_lds_bytes(int t) { return (size_t)t * sizeof(double) + (size_t)2 * (t + 1) * sizeof(uint32_t); }

}  // namespace

extern "C" {

size_t wsu_roc_counts_workspace_bytes(int groups, int t) {
    if (groups < 1 || groups > 65535 || t < 1 || t > ROC_MAX_T) return 0;
    return ((size_t)t + (size_t)groups + 1 + roc_hist_words(groups, t)) * 8;
}

int wsu_roc_counts(const double* scores, const signed char* labels, const long long* offsets, int groups, const double* taus, int t,
                   long long* counts, void* workspace, size_t workspace_bytes, void* stream) {
    WSU_REQUIRE(offsets && taus && counts && workspace, "roc_counts: null pointer");
    WSU_REQUIRE(groups >= 1 && groups <= 65535, "roc_counts: groups=%d (1..65535)", groups);
    WSU_REQUIRE(t >= 1 && t <= ROC_MAX_T, "roc_counts: t=%d (1..%d)", t, ROC_MAX_T);
    for (int j = 0; j < t; ++j) {
        WSU_REQUIRE(taus[j] == taus[j] && taus[j] - taus[j] == 0.0, "roc_counts: tau[%d]=%g is not finite", j, taus[j]);
        WSU_REQUIRE(j == 0 || taus[j] > taus[j - 1], "roc_counts: taus are not strictly ascending at %d (%.17g after %.17g)", j, taus[j],
                    taus[j - 1]);
    }
    WSU_REQUIRE(offsets[0] == 0, "roc_counts: offsets[0]=%lld (must be 0)", offsets[0]);
    long long longest = 0;
    for (int g = 0; g < groups; ++g) {
        WSU_REQUIRE(offsets[g + 1] >= offsets[g], "roc_counts: offsets decrease at group %d (%lld after %lld)", g, offsets[g + 1], offsets[g]);
        longest = std::max(longest,offsets[g + 1] - offsets[g]);
    }
    WSU_REQUIRE(offsets[groups] == 0 || (scores && labels), "roc_counts: null pointer");
    WSU_REQUIRE(workspace_bytes >= wsu_roc_counts_workspace_bytes(groups, t), "roc_counts: workspace too small (%zu < %zu bytes)", workspace_bytes,
                wsu_roc_counts_workspace_bytes(groups, t));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const RocWs p = roc_ws(workspace, groups, t);
    // the host arrays are pageable: the copies are staged before the calls return
    if (hipMemcpyAsync(p.taus, taus, (size_t)t * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess) return wsu_check_launch("roc_counts copy");
    if (hipMemcpyAsync(p.offsets, offsets, (size_t)(groups + 1) * sizeof(long long), hipMemcpyHostToDevice, s) != hipSuccess)
        return wsu_check_launch("roc_counts copy");
    if (hipMemsetAsync(p.hist, 0, roc_hist_words(groups, t) * 8, s) != hipSuccess) return wsu_check_launch("roc_counts memset");
    static bool attr_done = false;     // benign race: idempotent
    if (!attr_done) {
        if (int rc = wsu_raise_lds(roc_hist_kernel, (int)roc_lds_bytes(ROC_MAX_T), "roc_hist")) return rc;
        attr_done = true;
    }
    if (longest > 0) {
        // at least 16 scores per histogram bin and workgroup, so that the flush of the LDS histogram stays small beside the pass
        const long long per = std::max((long long)ROC_THREADS * ROC_UNROLL * 8, 16LL * 2 * (t + 1));
        const long long parts = std::min((long long)ROC_MAX_PARTS, (longest + per - 1) / per);
        hipLaunchKernelGGL(roc_hist_kernel, dim3((unsigned)parts, groups), dim3(ROC_THREADS), roc_lds_bytes(t), s, scores, labels, t, workspace,
                           groups);
        int rc = wsu_check_launch("roc_hist_kernel");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(roc_scan_kernel, dim3(groups), dim3(ROC_THREADS), 0, s, t, groups, workspace, counts);
    return wsu_check_launch("roc_scan_kernel");
}

}  // extern "C"
