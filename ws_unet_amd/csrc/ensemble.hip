// K53: the bootstrap-weighted scatter (Gram) matrices of the FLD ensemble's base learners, float64 on the f64 matrix pipe.
//
//   G[l][a][b] = sum_i weights[l][i] * zt[idx[l][a]][i] * zt[idx[l][b]][i]          (include/wsu.h has the contract)
//
// One launch serves many learners: blockIdx.y is the learner, blockIdx.x a tile ON OR BELOW the diagonal of its (d_sub, d_sub) result.
// zt is feature-major, so a gathered feature is one contiguous row and both operands stream coalesced along the summed index i; the
// gather costs nothing but the row pointer.
//
// Tile shape: a workgroup of 4 waves makes a 64 x 64 output tile, each wave a 32 x 32 quarter as 2 x 2 tiles of
// v_mfma_f64_16x16x4_f64 (16 accumulator doubles = 32 VGPRs per lane), and SG_KC = 32 values of i are staged per step.  Why this one:
//   * 4 independent accumulators per wave cover the MFMA's dependent latency with one wave per SIMD;
//   * a step loads 2 x 64 x 32 doubles for 2 x 64 x 64 x 32 flops: 8 flops per byte, which L2 serves, since the tiles of one learner walk i
//     together and share their rows;
//   * d_sub = 500 is 36 tiles per learner: a 128 x 128 tile would halve the traffic but leave 10 tiles per learner, too few workgroups
//     for 256 CUs at the L of a few learners that fits a launch's memory budget;
//   * 2 x 64 x 34 doubles of LDS (34 816 B) let four workgroups share a CU, so one's staging hides behind another's matrix work.
// LDS rows are [feature][i] with a stride of SG_KC + 2 doubles: a fragment read takes row (lane & 15), i = 4 ks + (lane >> 4), and
// 8-byte reads bank on (address / 4) mod 64 over half a wave, i.e. on (34 row + i) mod 32 = (2 row + i) mod 32 in doubles: the 16 rows
// x 2 values of i of a half-wave are the 32 distinct residues.  The staging writes (32 consecutive i of one row per half-wave) are
// conflict-free for any stride.
//
// Arithmetic: the weight is folded into the A operand where it is staged, fl(w * z_a), so an entry is a sum of fl(w z_a) z_b accumulated
// by the MFMA's fma chain: one extra rounding per term.  An entry is accumulated by ONE accumulator over i = 0 .. n_rows-1 in steps of 4
// (no split over i, no atomics), so its summation order depends on n_rows alone, not on L, the launch split or the tile's neighbours.
// fl(w z_a) z_b and fl(w z_b) z_a differ, so only entries with a >= b are taken from the accumulators and each is written twice, at
// [a][b] and at [b][a]: G[l] is symmetric bit for bit.  Diagonal tiles skip the quarter above the diagonal.
// Tails: a feature slot at or past d_sub and a value of i at or past n_rows are staged as zeros; nothing is read for them.
#include "wsu_device.h"

namespace {

constexpr int SG_TILE = 64;              // rows and columns of a workgroup's output tile
constexpr int SG_KC = 32;                // values of the summed index staged per step
constexpr int SG_LD = SG_KC + 2;         // LDS row stride in doubles (see above)
constexpr int SG_THREADS = 256;
constexpr int SG_ROWS_PER_THREAD = SG_TILE * SG_KC / SG_THREADS;      // 8 staged values per operand and thread
typedef __attribute__((ext_vector_type(4))) double f64x4;

__global__ __launch_bounds__(SG_THREADS) void subspace_gram_kernel(const double* __restrict__ zt, const int* __restrict__ idx,
                                                                   const int* __restrict__ weights, double* __restrict__ G, int n_rows,
                                                                   int d_sub) {
    __shared__ double As[SG_TILE * SG_LD];
    __shared__ double Bs[SG_TILE * SG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l = blockIdx.y;
    // the tile (bi, bj), bj <= bi, of the linear index t = bi (bi + 1) / 2 + bj
    const int t = blockIdx.x;
    int bi = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    while (bi > 0 && (long long)bi * (bi + 1) / 2 > t) --bi;
    while ((long long)(bi + 1) * (bi + 2) / 2 <= t) ++bi;
    const int bj = t - (int)((long long)bi * (bi + 1) / 2);

    // staging: a thread owns one value of i (kk) and 8 feature slots of each operand
    const int kk = tid & (SG_KC - 1), f0 = tid / SG_KC;
    const int* idx_l = idx + (size_t)l * d_sub;
    const int* w_l = weights + (size_t)l * n_rows;
    long long rowa[SG_ROWS_PER_THREAD], rowb[SG_ROWS_PER_THREAD];       // offset of the slot's feature row in zt, -1 for a slot past d_sub
#pragma unroll
    for (int j = 0; j < SG_ROWS_PER_THREAD; ++j) {
        const int a = bi * SG_TILE + f0 + j * (SG_THREADS / SG_KC), b = bj * SG_TILE + f0 + j * (SG_THREADS / SG_KC);
        rowa[j] = a < d_sub ? (long long)idx_l[a] * n_rows : -1;
        rowb[j] = b < d_sub ? (long long)idx_l[b] * n_rows : -1;
    }
    double ra[SG_ROWS_PER_THREAD], rb[SG_ROWS_PER_THREAD];
    auto fetch = [&](int chunk) {
        const int i = chunk * SG_KC + kk;
        const bool in = i < n_rows;
        const double w = in ? (double)w_l[i] : 0.;
#pragma unroll
        for (int j = 0; j < SG_ROWS_PER_THREAD; ++j) {
            ra[j] = in && rowa[j] >= 0 ? w * zt[rowa[j] + i] : 0.;
            rb[j] = in && rowb[j] >= 0 ? zt[rowb[j] + i] : 0.;
        }
    };

    const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;                  // the wave's quarter of the tile
    const bool live = bi != bj || wm >= wn;                            // a diagonal tile's upper quarter is never written
    f64x4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0., 0., 0., 0.};
    const double* afrag = As + (wm + (lane & 15)) * SG_LD + (lane >> 4);
    const double* bfrag = Bs + (wn + (lane & 15)) * SG_LD + (lane >> 4);

    const int chunks = (n_rows + SG_KC - 1) / SG_KC;
    fetch(0);
    for (int c = 0; c < chunks; ++c) {
#pragma unroll
        for (int j = 0; j < SG_ROWS_PER_THREAD; ++j) {
            As[(f0 + j * (SG_THREADS / SG_KC)) * SG_LD + kk] = ra[j];
            Bs[(f0 + j * (SG_THREADS / SG_KC)) * SG_LD + kk] = rb[j];
        }
        __syncthreads();
        if (c + 1 < chunks) fetch(c + 1);                               // the next step's loads fly during this step's matrix work
        if (live) {
#pragma unroll
            for (int ks = 0; ks < SG_KC / 4; ++ks) {
                const double a0 = afrag[ks * 4], a1 = afrag[16 * SG_LD + ks * 4];
                const double b0 = bfrag[ks * 4], b1 = bfrag[16 * SG_LD + ks * 4];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (!live) return;
    // the f64 C/D map: column = lane & 15, row = (lane >> 4) + 4 * register
    double* G_l = G + (size_t)l * d_sub * d_sub;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = bi * SG_TILE + wm + mi * 16 + (lane >> 4) + 4 * r, b = bj * SG_TILE + wn + ni * 16 + (lane & 15);
                if (a < d_sub && b <= a) {
                    const double v = acc[mi][ni][r];
                    G_l[(size_t)a * d_sub + b] = v;
                    if (a != b) G_l[(size_t)b * d_sub + a] = v;
                }
            }
}

// A register-only loop of the f64 MFMA: 4 independent accumulators per wave, no memory in the loop.  tools/bench_ensemble.py times it in
// the same process to have a measured ceiling to quote K53's rate against.
__global__ __launch_bounds__(SG_THREADS) void mfma_f64_loop_kernel(double* __restrict__ sink, int iters) {
    f64x4 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = f64x4{0., 0., 0., 0.};
    double a = 1e-3 * (threadIdx.x & 15), b = 1e-3 * (threadIdx.x >> 4);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[k], 0, 0, 0);
    }
    sink[(size_t)blockIdx.x * SG_THREADS + threadIdx.x] = acc[0][0] + acc[1][1] + acc[2][2] + acc[3][3];
}

}  // namespace

extern "C" {

int wsu_subspace_gram_f64(const double* zt, const int32_t* idx, const int32_t* weights, double* G, int n_rows, int d, int d_sub, int L,
                          void* stream) {
    WSU_REQUIRE(zt && idx && weights && G, "subspace_gram_f64: null pointer");
    WSU_REQUIRE(n_rows >= 1 && d >= 1 && d_sub >= 1 && L >= 1, "subspace_gram_f64: bad shape n_rows=%d d=%d d_sub=%d L=%d", n_rows, d, d_sub, L);
    WSU_REQUIRE(L <= 65535 && d_sub <= (1 << 20), "subspace_gram_f64: L=%d above 65535 or d_sub=%d above 2^20", L, d_sub);
    const long long tiles = (d_sub + SG_TILE - 1) / SG_TILE;
    hipLaunchKernelGGL(subspace_gram_kernel, dim3((unsigned)(tiles * (tiles + 1) / 2), (unsigned)L), dim3(SG_THREADS), 0,
                       static_cast<hipStream_t>(stream), zt, idx, weights, G, n_rows, d_sub);
    return wsu_check_launch("subspace_gram_kernel");
}

int wsu_mfma_f64_loop(double* sink, int blocks, int iters, void* stream) {
    WSU_REQUIRE(sink, "mfma_f64_loop: null pointer");
    WSU_REQUIRE(blocks >= 1 && blocks <= 65535 && iters >= 1, "mfma_f64_loop: bad shape blocks=%d iters=%d", blocks, iters);
    hipLaunchKernelGGL(mfma_f64_loop_kernel, dim3((unsigned)blocks), dim3(SG_THREADS), 0, static_cast<hipStream_t>(stream), sink, iters);
    return wsu_check_launch("mfma_f64_loop_kernel");
}

}  // extern "C"
