// K52: the WEIGHTED co-occurrence sums of the linear SRM submodels, the integer half of the selection-channel-aware features of
// ws_unet_amd/srm.py (maxSRM: Denemark, Sedighi, Holub, Cogranne, Fridrich, WIFS 2014).  Not part of the reference.  include/wsu.h has the
// definition: K49's residuals, digits, runs, bins and tables, and a counted run adds the LARGEST of the 16-bit weights at its four residual
// positions instead of 1.
//
// K49's walk (srm.hip: the strip tile of wsu_count.h, SR_TRT rows per thread, five pixel rows in registers, one row of 19 digits per
// residual and step, scan v from the byte that remembers the three digits above), written out again here so that srm.hip stays as it is,
// with four differences:
//   * the weight of a run.  A residual's positions are its centres: row rho + u of the step, column c + t - o of digit t.  Scan h, run i:
//     the largest of four neighbours in that row; scan v, the run that ends in this row at column c + i + d: the largest of that column's
//     rows rho + u - 3 .. rho + u.  The weights are READ WHERE THEY ARE USED, a row segment at a time through the caches, and not held in a
//     window of 60 or more registers: a step is ~20 000 instructions of a wave that has its SIMD to itself, and the ~660 two-byte loads
//     of a step are a few per cent of it (sw_segment: an immediate offset each where the segment lies in the plane, clamped indices at
//     the plane's two ends).  A weight is cleared where its run is not counted, so the bin test needs no validity mask of its own and a
//     run of weight 0 takes no atomic;
//   * the centre bins.  K49 gives the centre what is left of the thread's counted RUNS; here what is left is a weight sum.  The total
//     weight of a thread's counted runs depends on the run's geometry (residual, scan) alone, not on q: 16 sums per thread, folded over
//     the wave into 16 words of LDS.  No run ever adds to a centre bin in the row loop; at the end a wave sums a table's 625 bins and
//     writes centre = total[geometry] - that sum.  A constant plane therefore takes no LDS atomic at all;
//   * three walks of the strip (sw_walk), each with a third of the kinds of digit, because one walk with the weights beside it does not
//     fit the registers;
//   * 32-bit bins still hold a tile (static_assert below); count_flush adds them to the image's 64-bit sums.
#include "wsu_count.h"

namespace {

constexpr int SW_TRT = 8, SW_STEPS = SW_TRT + 3, SW_ROWS = CT_GROUPS * SW_TRT, SW_WIN = 5, SW_DIGITS = 19;
constexpr int SW_TABLES = 44, SW_BINS = 625, SW_CENTRE = 312, SW_GEOMETRIES = 16;
static_assert((long long)SW_ROWS * CT_COLS * 65535 < (1ll << 32), "a tile's 32-bit bins must hold every position of the tile at the largest weight");

struct SwState {
    uint32_t* hist;                                     // [SW_TABLES][SW_BINS], the workgroup's
    uint32_t total[SW_GEOMETRIES];                      // per (residual, scan): the weight of the thread's counted runs
    uint32_t above[SW_TABLES / 2][4];                   // per kind: byte i = the digits (+2) of the three rows above in column i, base 5
};

// the geometry (residual, scan) of a table, 0 .. 15: S1 hh hv vh vv, S2 .., S3 .., S3x3 nh nv, S5x5 nh nv
__host__ __device__ constexpr int sw_geometry(int table) {
    return table < 8 ? table & 3 : table < 20 ? 4 + ((table - 8) & 3) : table < 32 ? 8 + ((table - 20) & 3) : table < 38 ? 12 + (table & 1)
                                                                                                                          : 14 + (table & 1);
}

// bit i of a mask as 0 or -1
__device__ __forceinline__ uint32_t sw_bit(uint32_t mask, int i) { return (uint32_t)((int)(mask << (31 - i)) >> 31); }

// one run of TABLE of weight wt (0 where the run is not counted): outside the centre bin it takes the LDS atomic; the centre bin is made
// at the end from the geometry's total
template <int TABLE> __device__ __forceinline__ void sw_count(SwState& s, uint32_t bin, uint32_t wt) {
    uint32_t both = min(bin ^ (uint32_t)SW_CENTRE, wt);                  // not zero: another bin and a weight.  ONE test of a vector value:
    asm volatile("" : "+v"(both));                                       // as two, `wt != 0` waits in 32 scalar register pairs per residual
    if (both != 0u) atomicAdd(&s.hist[TABLE * SW_BINS + bin], wt);
}

// K49's sr_tables with a weight per run: wh[i] of scan h's run i, wv[i] of scan v's run that ends at digit i + S
template <int TABLE, int S, int Q2>
__device__ __forceinline__ void sw_tables(SwState& s, const int (&mag)[SW_DIGITS], const int (&sgn)[SW_DIGITS], const uint32_t (&wh)[16],
                                          const uint32_t (&wv)[16]) {
    int dg[SW_DIGITS];
#pragma unroll
    for (int t = 0; t < SW_DIGITS; ++t) {
        const int m = (4 * mag[t] >= Q2 ? 1 : 0) + (4 * mag[t] >= 3 * Q2 ? 1 : 0);
        dg[t] = (m ^ sgn[t]) - sgn[t] + 2;
    }
    int pair[SW_DIGITS - 1];
#pragma unroll
    for (int t = 0; t < SW_DIGITS - 1; ++t) pair[t] = dg[t] * 5 + dg[t + 1];
#pragma unroll
    for (int i = 0; i < 16; ++i) sw_count<TABLE>(s, (uint32_t)(pair[i] * 25 + pair[i + 2]), wh[i]);
    uint32_t (&above)[4] = s.above[TABLE >> 1];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        uint32_t now = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * g + j;
            const uint32_t bin = ((above[g] >> (8 * j)) & 255u) * 5u + (uint32_t)dg[i + S];
            sw_count<TABLE + 1>(s, bin, wv[i]);
            now |= (bin % 125u) << (8 * j);
        }
        above[g] = now;
    }
}

// N weights plane[first .. first + N), `first` the plane index of a row's column col0 (-1 .. w - 1): ONE decision per segment, as in
// ct_load_row.  Where the segment lies in the plane: loads at immediate offsets of one address -- a segment that runs past its row's end (the
// last strips) or begins at column -1 (the first strip) then reads the neighbouring row's weights, which belong to no counted run.  Else (the
// first strip of the first row, the last strips of the last row): every index clamped into the plane, one load after the other.
template <int N> __device__ __forceinline__ void sw_segment(const uint16_t* __restrict__ plane, long long first, long long hw, uint32_t (&v)[N]) {
    if (first >= 0 && first + N <= hw) {
        const uint16_t* p = plane + first;
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = p[i];
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            v[i] = plane[min(max(first + i, 0ll), hw - 1)];
            asm volatile("" : "+v"(v[i]));            // (rare: no N addresses at once)
        }
    }
}

// The weights of one residual's runs at a step.  wimg: the image's weight plane; the residuals' row is rho + U (U <= 2: it may lie past
// the image in a step that counts nothing, so every row index is clamped into the plane); scan h's run i covers columns c - O + i .. + 3,
// scan v's run i ends in column c + D + i of that row and began three rows up.  Cleared where bit i of mh / mv is not set, and the sums
// of what is left added to the two geometries' totals.
template <int GEOMETRY, int U, int O, int D>
__device__ __forceinline__ void sw_weights(SwState& s, const uint16_t* __restrict__ wimg, long long rho, long long c, int h, int w,
                                           uint32_t mh, uint32_t mv, uint32_t (&wh)[16], uint32_t (&wv)[16]) {
    // the masks' bits are tested here, not ahead of the loop in scalar register pairs; the segments' addresses are made here, not shared
    // by the residuals of a step and kept
    asm volatile("" : "+v"(mh), "+v"(mv), "+v"(c));
    const long long last = (long long)h - 1, hw = (long long)h * w;
    {
        uint32_t seg[SW_DIGITS];
        sw_segment<SW_DIGITS>(wimg, min(rho + U, last) * w + c - O, hw, seg);
        uint32_t sum = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            wh[i] = max(max(seg[i], seg[i + 1]), max(seg[i + 2], seg[i + 3])) & sw_bit(mh, i);
            sum += wh[i];
        }
        s.total[GEOMETRY] += sum;
    }
    {
        uint32_t top[16], seg[16];
        sw_segment<16>(wimg, min(max(rho + U - 3, 0ll), last) * w + c + D, hw, top);
#pragma unroll
        for (int k = 2; k >= 0; --k) {
            sw_segment<16>(wimg, min(max(rho + U - k, 0ll), last) * w + c + D, hw, seg);
#pragma unroll
            for (int i = 0; i < 16; ++i) top[i] = max(top[i], seg[i]);
        }
        uint32_t sum = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            wv[i] = top[i] & sw_bit(mv, i);
            sum += wv[i];
        }
        s.total[GEOMETRY + 1] += sum;
    }
}

// one residual at its two or three steps (QC = 0: two); TABLE: its first table, TSTEP tables on per step
template <int TABLE, int TSTEP, int S, int QA, int QB, int QC>
__device__ __forceinline__ void sw_residual(SwState& s, const int (&R)[SW_DIGITS], const uint32_t (&wh)[16], const uint32_t (&wv)[16]) {
    int mag[SW_DIGITS], sgn[SW_DIGITS];
#pragma unroll
    for (int t = 0; t < SW_DIGITS; ++t) {
        mag[t] = abs(R[t]);
        sgn[t] = R[t] >> 31;
    }
    sw_tables<TABLE, S, QA>(s, mag, sgn, wh, wv);
    sw_tables<TABLE + TSTEP, S, QB>(s, mag, sgn, wh, wv);
    if constexpr (QC != 0) sw_tables<TABLE + 2 * TSTEP, S, QC>(s, mag, sgn, wh, wv);
}

__device__ __forceinline__ uint32_t sw_low_bits(int n) { return (1u << min(max(n, 0), 16)) - 1u; }

// between two residuals: what one of them unpacked from the window is not kept for the next
__device__ __forceinline__ void sw_forget(CtRow (&win)[SW_WIN]) {
#pragma unroll
    for (int j = 0; j < SW_WIN; ++j) asm volatile("" : "+v"(win[j].left), "+v"(win[j].mid), "+v"(win[j].right));
}

// One walk of the thread's strip for the residuals of PASS: 0 takes S1 and S2 h (7 kinds of digit), 1 takes S2 v and the 3x3 kernel made of
// it (6), 2 takes S3 and the 5x5 kernel (9).  One walk for all 22 is K49's, and beside the weights it does not fit the registers: the bytes of
// `above` alone are 88; the walk with every kind compiled to 290 spilled registers, two walks of 13 and 9 kinds to 18.  Three walks read the
// pixel rows three times and compute every residual once.
template <int PASS>
__device__ __forceinline__ void sw_walk(const uint8_t* __restrict__ img, const uint16_t* __restrict__ wimg, uint32_t* __restrict__ hist,
                                        uint32_t* __restrict__ total, const CtStrip& st, int h, int w) {
    const long long c = st.c, r0 = st.r0;
    const int rem = st.rem;
    const bool live = c < w && r0 < h;
    SwState s;
    s.hist = hist;
#pragma unroll
    for (int g = 0; g < SW_GEOMETRIES; ++g) s.total[g] = 0u;
#pragma unroll
    for (int k = 0; k < SW_TABLES / 2; ++k)
#pragma unroll
        for (int g = 0; g < 4; ++g) s.above[k][g] = 0u;
    if (live) {
        CtRow win[SW_WIN];
#pragma unroll
        for (int j = 0; j < SW_WIN; ++j) win[j] = r0 + j < h ? ct_load_row(img + (size_t)(r0 + j) * w, c, w) : ct_no_row();
        // the columns of a run B + 1 pixels wide whose leftmost is c - S + i (scan h) or c + i (scan v, S = 0): bit i set when it is in the row
        const uint32_t first = c > 0 ? 0xffffu : 0u;
        auto cols = [&](int B, int S) { return sw_low_bits(rem - B + S) & (first | ~((1u << S) - 1u)); };
#pragma unroll 1
        for (int m = 0; m < SW_STEPS; ++m) {
            const long long rho = r0 + m;
            auto px = [&](int j, int col) { return ct_px(win[j], col); };
            // scan h counts at steps 0 .. SW_TRT-1, scan v at 3 .. SW_TRT+2; both where the residuals' lowest row rho + ud is in the image
            auto rows_h = [&](int ud) { return m < SW_TRT && rho + ud < h ? 0xffffu : 0u; };
            auto rows_v = [&](int ud) { return m >= 3 && rho + ud < h ? 0xffffu : 0u; };
            int R[SW_DIGITS];
            uint32_t wh[16], wv[16];
            if constexpr (PASS == 0) {
                // S1 h: position (rho, c + t)
#pragma unroll
                for (int t = 0; t < SW_DIGITS; ++t) R[t] = px(0, t + 1) - px(0, t);
                sw_weights<0, 0, 0, 0>(s, wimg, rho, c, h, w, cols(4, 0) & rows_h(0), cols(1, 0) & rows_v(0), wh, wv);
                sw_residual<0, 4, 0, 2, 4, 0>(s, R, wh, wv);
                sw_forget(win);
                // S1 v: position (rho, c + t)
#pragma unroll
                for (int t = 0; t < SW_DIGITS; ++t) R[t] = px(1, t) - px(0, t);
                sw_weights<2, 0, 0, 0>(s, wimg, rho, c, h, w, cols(3, 0) & rows_h(1), cols(0, 0) & rows_v(1), wh, wv);
                sw_residual<2, 4, 0, 2, 4, 0>(s, R, wh, wv);
                sw_forget(win);
                // S2 h: centre (rho, c + t) (the run's leftmost pixel is c - 1 + i; scan v takes digit i + 1, centre column c + i + 1)
#pragma unroll
                for (int t = 0; t < SW_DIGITS; ++t) R[t] = px(0, t - 1) - 2 * px(0, t) + px(0, t + 1);
                sw_weights<4, 0, 0, 1>(s, wimg, rho, c, h, w, cols(5, 1) & rows_h(0), cols(2, 0) & rows_v(0), wh, wv);
                sw_residual<8, 4, 1, 4, 6, 8>(s, R, wh, wv);
            } else if constexpr (PASS == 1) {
                // S2 v, and the 3x3 kernel from it: KB = -(1,-2,1)^T (1,-2,1).  Both have their centres in row rho + 1, columns c-1 .. c+19
                int sv[SW_DIGITS + 2];
#pragma unroll
                for (int t = 0; t < SW_DIGITS + 2; ++t) sv[t] = px(0, t - 1) - 2 * px(1, t - 1) + px(2, t - 1);
#pragma unroll
                for (int t = 0; t < SW_DIGITS; ++t) R[t] = 2 * sv[t + 1] - sv[t] - sv[t + 2];
                sw_weights<12, 1, 0, 1>(s, wimg, rho, c, h, w, cols(5, 1) & rows_h(2), cols(2, 0) & rows_v(2), wh, wv);
                sw_residual<32, 2, 1, 8, 12, 16>(s, R, wh, wv);
#pragma unroll
                for (int t = 0; t < SW_DIGITS; ++t) R[t] = sv[t + 1];
                sw_weights<6, 1, 0, 0>(s, wimg, rho, c, h, w, cols(3, 0) & rows_h(2), cols(0, 0) & rows_v(2), wh, wv);
                sw_residual<10, 4, 0, 4, 6, 8>(s, R, wh, wv);
            } else {
                // S3 h: centre (rho, c - 1 + t) (leftmost pixel c - 2 + i; scan v takes digit i + 2, centre column c + i + 1)
#pragma unroll
                for (int t = 0; t < SW_DIGITS; ++t) R[t] = px(0, t - 2) - 3 * px(0, t - 1) + 3 * px(0, t) - px(0, t + 1);
                sw_weights<8, 0, 1, 1>(s, wimg, rho, c, h, w, cols(6, 2) & rows_h(0), cols(3, 0) & rows_v(0), wh, wv);
                sw_residual<20, 4, 2, 6, 9, 12>(s, R, wh, wv);
                sw_forget(win);
                // S3 v: centre (rho + 1, c + t)
#pragma unroll
                for (int t = 0; t < SW_DIGITS; ++t) R[t] = px(0, t) - 3 * px(1, t) + 3 * px(2, t) - px(3, t);
                sw_weights<10, 1, 0, 0>(s, wimg, rho, c, h, w, cols(3, 0) & rows_h(3), cols(0, 0) & rows_v(3), wh, wv);
                sw_residual<22, 4, 0, 6, 9, 12>(s, R, wh, wv);
                sw_forget(win);
                // 5x5: centre (rho + 2, c - 1 + t) (leftmost pixel c - 3 + i; scan v takes digit i + 3, centre column c + i + 2).  Rows +-2
                // and +-1 have the same weights, so a column x contributes v0 at offset 0, v1 at +-1, v2 at +-2; x = c-3 .. c+19
                {
                    int v0[SW_DIGITS + 4], v1[SW_DIGITS + 4], v2[SW_DIGITS + 4];
#pragma unroll
                    for (int t = 0; t < SW_DIGITS + 4; ++t) {
                        const int A = px(0, t - 3) + px(4, t - 3), B = px(1, t - 3) + px(3, t - 3), C = px(2, t - 3);
                        v0[t] = -2 * A + 8 * B - 12 * C;
                        v1[t] = 2 * A - 6 * B + 8 * C;
                        v2[t] = -A + 2 * B - 2 * C;
                    }
#pragma unroll
                    for (int t = 0; t < SW_DIGITS; ++t) R[t] = v0[t + 2] + v1[t + 1] + v1[t + 3] + v2[t] + v2[t + 4];
                }
                sw_weights<14, 2, 1, 2>(s, wimg, rho, c, h, w, cols(7, 3) & rows_h(4), cols(4, 0) & rows_v(4), wh, wv);
                sw_residual<38, 2, 3, 24, 36, 48>(s, R, wh, wv);
            }
#pragma unroll
            for (int j = 0; j < SW_WIN - 1; ++j) win[j] = win[j + 1];
            long long cc = c;
            asm volatile("" : "+v"(cc));                // the load's 24 clamped column offsets are made here, not kept across the loop
            win[SW_WIN - 1] = m + 1 < SW_STEPS && rho + SW_WIN < h ? ct_load_row(img + (size_t)(rho + SW_WIN) * w, cc, w) : ct_no_row();
        }
    }
    // the totals of the walk's geometries over the workgroup
#pragma unroll
    for (int g = 0; g < SW_GEOMETRIES; ++g) {
        if (PASS != (g < 6 ? 0 : g < 8 || g == 12 || g == 13 ? 1 : 2)) continue;
        const uint32_t t = wave_sum(s.total[g]);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(&total[g], t);
    }
}

__global__ __launch_bounds__(CT_THREADS) void srm_weighted_counts_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ sums,
                                                                         int h, int w, int tiles_c, const uint16_t* __restrict__ weights) {
    __shared__ uint32_t hist[SW_TABLES * SW_BINS];
    __shared__ uint32_t total[SW_GEOMETRIES];
    const int nn = blockIdx.y, tid = threadIdx.x;
    const CtStrip st = ct_strip_rows<SW_TRT>(tiles_c, w);
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const uint16_t* wimg = weights + (size_t)nn * h * w;
    for (int i = tid; i < SW_TABLES * SW_BINS; i += CT_THREADS) hist[i] = 0u;
    if (tid < SW_GEOMETRIES) total[tid] = 0u;
    __syncthreads();
    sw_walk<0>(img, wimg, hist, total, st, h, w);
    sw_walk<1>(img, wimg, hist, total, st, h, w);
    sw_walk<2>(img, wimg, hist, total, st, h, w);
    __syncthreads();
    // the centre bins, which no run has added to: a wave per table sums its bins; centre = the geometry's total - that sum
    for (int t = tid >> 6; t < SW_TABLES; t += CT_WAVES) {
        uint32_t other = 0u;
        for (int b = tid & 63; b < SW_BINS; b += 64) other += hist[t * SW_BINS + b];
        other = wave_sum(other);
        if ((tid & 63) == 0) hist[t * SW_BINS + SW_CENTRE] = total[sw_geometry(t)] - other;
    }
    count_flush<CT_WAVES, uint32_t, 1>(hist, SW_TABLES * SW_BINS, sums, (size_t)nn * SW_TABLES * SW_BINS);
}

}  // namespace

extern "C" {

int wsu_srm_weighted_counts(const uint8_t* x_u8, const uint16_t* weights_u16, unsigned long long* sums, int n, int h, int w, void* stream) {
    WSU_REQUIRE(weights_u16, "srm_weighted_counts: null pointer");
    return count_launch("srm_weighted_counts", "srm_weighted_counts memset", "srm_weighted_counts_kernel", srm_weighted_counts_kernel,
                        CT_THREADS, 0, x_u8, sums, (size_t)SW_TABLES * SW_BINS, n, h, w, 0, SW_ROWS, CT_COLS, stream, weights_u16);
}

}  // extern "C"
