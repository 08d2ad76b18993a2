// K49: the co-occurrence counts of the linear ("spam"-type) submodels of the spatial rich model (SRM; Fridrich, Kodovsky, IEEE TIFS 7(3),
// 2012), the integer half of the detector of ws_unet_amd/srm.py.  Not part of the reference.  include/wsu.h has the definition: eight linear
// residuals per pixel, each quantised at two or three steps q into a digit -2 .. 2, 22 digits in all; a table counts the runs of four
// digits of one kind along a row (scan h) or down a column (scan v): 44 tables of 625 bins.
//
// A count kernel on the strip tile of wsu_count.h, a thread walking SR_TRT rows of its strip.  A digit is computed ONCE per pixel and step:
//   * a step has the five pixel rows rho .. rho+4 in registers (CtRow each) and computes, per kind, the 19 digits of ONE row of residual
//     centres, row rho + u (u: how far the residual reaches up).  No residual reaches over more than five rows;
//   * scan h: the 16 runs of that row, run i from digits i .. i+3.  Their leftmost pixel is column c - s + i, s = max(b - 4, 0) for a run
//     that is b + 1 pixels wide, so that the widest (5x5: 8 pixels, s = 3) reads c-3 .. c+19, which CtRow has;
//   * scan v: the run that ENDS in this row, from a byte per kind and column that holds the three digits above as a base-5 number
//     (22 x 4 registers).  The run's top row is rho - 3, so a thread takes SR_TRT + 3 steps: steps 0 .. SR_TRT-1 count scan h, steps
//     3 .. SR_TRT+2 scan v, and every run belongs to exactly one thread.
// ONE set of tables per workgroup (110 000 bytes of LDS; a copy per wave as in K36 would be 440 000) that its four waves add to with
// LDS atomics -- except the 44 centre bins, which a smooth or saturated plane sends every update to.  A thread counts in HotBins
// fields, four tables to a register, the runs that went to ANOTHER bin (beside their LDS atomic, under the same test), and the centre
// bin gets what is left of the thread's counted runs: a centre run costs one test and no more.
#include "wsu_count.h"

namespace {

constexpr int SR_TRT = 8, SR_STEPS = SR_TRT + 3, SR_ROWS = CT_GROUPS * SR_TRT, SR_WIN = 5, SR_DIGITS = 19;
constexpr int SR_TABLES = 44, SR_BINS = 625, SR_CENTRE = 312;
static_assert((long long)SR_ROWS * CT_COLS < (1ll << 32), "a tile's 32-bit bins must hold every position of the tile");
using SrHot = HotBins<4, 8, 16 * SR_TRT>;               // four tables to a register; a thread sees 16 * SR_TRT runs of a table

struct SrState {
    uint32_t* hist;                                     // [SR_TABLES][SR_BINS], the workgroup's
    SrHot other[SR_TABLES / 4];                         // per table: the thread's counted runs that did NOT go to the centre bin
    uint32_t above[SR_TABLES / 2][4];                   // per kind: byte i = the digits (+2) of the three rows above in column i, base 5
};

// bit i of a mask as 0 or -1
__device__ __forceinline__ uint32_t sr_bit(uint32_t mask, int i) { return (uint32_t)((int)(mask << (31 - i)) >> 31); }

// one run of TABLE, counted when `counted` is -1 (not 0): a run outside the centre bin takes the LDS atomic and is noted in `other`; the
// centre bin is what is left of the thread's counted runs at the end, so neither a centre run nor an uncounted one costs more than this test
template <int TABLE> __device__ __forceinline__ void sr_count(SrState& s, uint32_t bin, uint32_t counted) {
    if (((bin ^ (uint32_t)SR_CENTRE) & counted) != 0u) {
        atomicAdd(&s.hist[TABLE * SR_BINS + bin], 1u);
        s.other[TABLE >> 2].add(TABLE & 3, true);
    }
}

// One kind at one step: its residuals' magnitudes and signs (R >> 31) at the 19 centres of the row, quantised at q = Q2 / 2:
// digit = sign(R) min((4|R| + Q2) / (2 Q2), 2), which is (4|R| >= Q2) + (4|R| >= 3 Q2) with the sign.  TABLE (even): scan h, run i of
// digits i .. i+3, counted where bit i of mh is set; TABLE + 1: scan v, digit i + S under the three above it, where bit i of mv is set.
template <int TABLE, int S, int Q2>
__device__ __forceinline__ void sr_tables(SrState& s, const int (&mag)[SR_DIGITS], const int (&sgn)[SR_DIGITS], uint32_t mh, uint32_t mv) {
    asm volatile("" : "+v"(mh), "+v"(mv));            // the masks' bits are tested here, not ahead of the loop in 256 scalar register pairs
    int dg[SR_DIGITS];
#pragma unroll
    for (int t = 0; t < SR_DIGITS; ++t) {
        const int m = (4 * mag[t] >= Q2 ? 1 : 0) + (4 * mag[t] >= 3 * Q2 ? 1 : 0);
        dg[t] = (m ^ sgn[t]) - sgn[t] + 2;
    }
    int pair[SR_DIGITS - 1];
#pragma unroll
    for (int t = 0; t < SR_DIGITS - 1; ++t) pair[t] = dg[t] * 5 + dg[t + 1];
#pragma unroll
    for (int i = 0; i < 16; ++i) sr_count<TABLE>(s, (uint32_t)(pair[i] * 25 + pair[i + 2]), sr_bit(mh, i));
    uint32_t (&above)[4] = s.above[TABLE >> 1];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        uint32_t now = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * g + j;
            const uint32_t bin = ((above[g] >> (8 * j)) & 255u) * 5u + (uint32_t)dg[i + S];
            sr_count<TABLE + 1>(s, bin, sr_bit(mv, i));
            now |= (bin % 125u) << (8 * j);
        }
        above[g] = now;
    }
}

// one residual at its two or three steps (QC = 0: two); TABLE: its first table, TSTEP tables on per step
template <int TABLE, int TSTEP, int S, int QA, int QB, int QC>
__device__ __forceinline__ void sr_residual(SrState& s, const int (&R)[SR_DIGITS], uint32_t mh, uint32_t mv) {
    int mag[SR_DIGITS], sgn[SR_DIGITS];
#pragma unroll
    for (int t = 0; t < SR_DIGITS; ++t) {
        mag[t] = abs(R[t]);
        sgn[t] = R[t] >> 31;
    }
    sr_tables<TABLE, S, QA>(s, mag, sgn, mh, mv);
    sr_tables<TABLE + TSTEP, S, QB>(s, mag, sgn, mh, mv);
    if constexpr (QC != 0) sr_tables<TABLE + 2 * TSTEP, S, QC>(s, mag, sgn, mh, mv);
}

__device__ __forceinline__ uint32_t sr_low_bits(int n) { return (1u << min(max(n, 0), 16)) - 1u; }

// between two residuals: what one of them unpacked from the window is not kept for the next (23 columns of 5 rows would stay in registers)
__device__ __forceinline__ void sr_forget(CtRow (&win)[SR_WIN]) {
#pragma unroll
    for (int j = 0; j < SR_WIN; ++j) asm volatile("" : "+v"(win[j].left), "+v"(win[j].mid), "+v"(win[j].right));
}

__global__ __launch_bounds__(CT_THREADS) void srm_counts_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ counts,
                                                                int h, int w, int tiles_c) {
    __shared__ uint32_t hist[SR_TABLES * SR_BINS];
    const int nn = blockIdx.y, tid = threadIdx.x;
    const CtStrip st = ct_strip_rows<SR_TRT>(tiles_c, w);
    const long long c = st.c, r0 = st.r0;
    const int rem = st.rem;
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const bool live = c < w && r0 < h;
    SrState s;
    s.hist = hist;
#pragma unroll
    for (int k = 0; k < SR_TABLES / 2; ++k)
#pragma unroll
        for (int g = 0; g < 4; ++g) s.above[k][g] = 0u;
    CtRow win[SR_WIN];
#pragma unroll
    for (int j = 0; j < SR_WIN; ++j) win[j] = live && r0 + j < h ? ct_load_row(img + (size_t)(r0 + j) * w, c, w) : ct_no_row();
    for (int i = tid; i < SR_TABLES * SR_BINS; i += CT_THREADS) hist[i] = 0u;           // (behind the window's loads)
    __syncthreads();
    // per class the thread's counted runs, a byte per table of one step q: S1, S2, S3 (h scanned h, h scanned v, v scanned h, v scanned v),
    // the 3x3 and the 5x5 kernel (scanned h, scanned v)
    uint32_t runs[5] = {0u, 0u, 0u, 0u, 0u};
    if (live) {
        // the columns of a run B + 1 pixels wide whose leftmost is c - S + i (scan h) or c + i (scan v, S = 0): bit i set when it is in the row
        const uint32_t first = c > 0 ? 0xffffu : 0u;
        auto cols = [&](int B, int S) { return sr_low_bits(rem - B + S) & (first | ~((1u << S) - 1u)); };
#pragma unroll 1
        for (int m = 0; m < SR_STEPS; ++m) {
            const long long rho = r0 + m;
            auto px = [&](int j, int col) { return ct_px(win[j], col); };
            // scan h counts at steps 0 .. SR_TRT-1, scan v at 3 .. SR_TRT+2; both where the residuals' lowest row rho + ud is in the image
            auto rows_h = [&](int ud) { return m < SR_TRT && rho + ud < h ? 0xffffu : 0u; };
            auto rows_v = [&](int ud) { return m >= 3 && rho + ud < h ? 0xffffu : 0u; };
            int R[SR_DIGITS];
            uint32_t mh, mv;
            // S1 h: centre column c + t
#pragma unroll
            for (int t = 0; t < SR_DIGITS; ++t) R[t] = px(0, t + 1) - px(0, t);
            mh = cols(4, 0) & rows_h(0), mv = cols(1, 0) & rows_v(0);
            runs[0] += (uint32_t)__popc(mh) + ((uint32_t)__popc(mv) << 8);
            sr_residual<0, 4, 0, 2, 4, 0>(s, R, mh, mv);
            sr_forget(win);
            // S1 v
#pragma unroll
            for (int t = 0; t < SR_DIGITS; ++t) R[t] = px(1, t) - px(0, t);
            mh = cols(3, 0) & rows_h(1), mv = cols(0, 0) & rows_v(1);
            runs[0] += ((uint32_t)__popc(mh) << 16) + ((uint32_t)__popc(mv) << 24);
            sr_residual<2, 4, 0, 2, 4, 0>(s, R, mh, mv);
            sr_forget(win);
            // S2 h: centre column c + t (the run's leftmost pixel is c - 1 + i)
#pragma unroll
            for (int t = 0; t < SR_DIGITS; ++t) R[t] = px(0, t - 1) - 2 * px(0, t) + px(0, t + 1);
            mh = cols(5, 1) & rows_h(0), mv = cols(2, 0) & rows_v(0);
            runs[1] += (uint32_t)__popc(mh) + ((uint32_t)__popc(mv) << 8);
            sr_residual<8, 4, 1, 4, 6, 8>(s, R, mh, mv);
            sr_forget(win);
            // S2 v, and the 3x3 kernel from it: KB = -(1,-2,1)^T (1,-2,1).  Both have their centres in row rho + 1, columns c-1 .. c+19
            int sv[SR_DIGITS + 2];
#pragma unroll
            for (int t = 0; t < SR_DIGITS + 2; ++t) sv[t] = px(0, t - 1) - 2 * px(1, t - 1) + px(2, t - 1);
#pragma unroll
            for (int t = 0; t < SR_DIGITS; ++t) R[t] = 2 * sv[t + 1] - sv[t] - sv[t + 2];
            mh = cols(5, 1) & rows_h(2), mv = cols(2, 0) & rows_v(2);
            runs[3] += (uint32_t)__popc(mh) + ((uint32_t)__popc(mv) << 8);
            sr_residual<32, 2, 1, 8, 12, 16>(s, R, mh, mv);
#pragma unroll
            for (int t = 0; t < SR_DIGITS; ++t) R[t] = sv[t + 1];
            mh = cols(3, 0) & rows_h(2), mv = cols(0, 0) & rows_v(2);
            runs[1] += ((uint32_t)__popc(mh) << 16) + ((uint32_t)__popc(mv) << 24);
            sr_residual<10, 4, 0, 4, 6, 8>(s, R, mh, mv);
            sr_forget(win);
            // S3 h: centre column c - 1 + t (leftmost pixel c - 2 + i)
#pragma unroll
            for (int t = 0; t < SR_DIGITS; ++t) R[t] = px(0, t - 2) - 3 * px(0, t - 1) + 3 * px(0, t) - px(0, t + 1);
            mh = cols(6, 2) & rows_h(0), mv = cols(3, 0) & rows_v(0);
            runs[2] += (uint32_t)__popc(mh) + ((uint32_t)__popc(mv) << 8);
            sr_residual<20, 4, 2, 6, 9, 12>(s, R, mh, mv);
            sr_forget(win);
            // S3 v: centre row rho + 1
#pragma unroll
            for (int t = 0; t < SR_DIGITS; ++t) R[t] = px(0, t) - 3 * px(1, t) + 3 * px(2, t) - px(3, t);
            mh = cols(3, 0) & rows_h(3), mv = cols(0, 0) & rows_v(3);
            runs[2] += ((uint32_t)__popc(mh) << 16) + ((uint32_t)__popc(mv) << 24);
            sr_residual<22, 4, 0, 6, 9, 12>(s, R, mh, mv);
            sr_forget(win);
            // 5x5: centre row rho + 2, centre column c - 1 + t (leftmost pixel c - 3 + i).  Rows +-2 and +-1 have the same weights, so
            // a column x contributes v0 at offset 0, v1 at +-1, v2 at +-2; x = c-3 .. c+19
            {
                int v0[SR_DIGITS + 4], v1[SR_DIGITS + 4], v2[SR_DIGITS + 4];
#pragma unroll
                for (int t = 0; t < SR_DIGITS + 4; ++t) {
                    const int A = px(0, t - 3) + px(4, t - 3), B = px(1, t - 3) + px(3, t - 3), C = px(2, t - 3);
                    v0[t] = -2 * A + 8 * B - 12 * C;
                    v1[t] = 2 * A - 6 * B + 8 * C;
                    v2[t] = -A + 2 * B - 2 * C;
                }
#pragma unroll
                for (int t = 0; t < SR_DIGITS; ++t) R[t] = v0[t + 2] + v1[t + 1] + v1[t + 3] + v2[t] + v2[t + 4];
            }
            mh = cols(7, 3) & rows_h(4), mv = cols(4, 0) & rows_v(4);
            runs[4] += (uint32_t)__popc(mh) + ((uint32_t)__popc(mv) << 8);
            sr_residual<38, 2, 3, 24, 36, 48>(s, R, mh, mv);
#pragma unroll
            for (int j = 0; j < SR_WIN - 1; ++j) win[j] = win[j + 1];
            long long cc = c;
            asm volatile("" : "+v"(cc));                // the load's 24 clamped column offsets are made here, not kept across the loop
            win[SR_WIN - 1] = m + 1 < SR_STEPS && rho + SR_WIN < h ? ct_load_row(img + (size_t)(rho + SR_WIN) * w, cc, w) : ct_no_row();
        }
    }
    // the centre bins: the counted runs less those that went elsewhere, table by table in the fields of HotBins (tables 4g .. 4g+3)
#pragma unroll
    for (int g = 0; g < SR_TABLES / 4; ++g) {
        const uint32_t all = g < 2 ? runs[0] : g < 5 ? runs[1] : g < 8 ? runs[2] : g == 8 ? runs[3] | (runs[3] << 16) :
                             g == 9 ? runs[3] | (runs[4] << 16) : runs[4] | (runs[4] << 16);
        SrHot centre;
        centre.v = all - s.other[g].v;
        centre.fold(hist + 4 * g * SR_BINS + SR_CENTRE, SR_BINS);
    }
    count_flush<CT_WAVES, uint32_t, 1>(hist, SR_TABLES * SR_BINS, counts, (size_t)nn * SR_TABLES * SR_BINS);
}

}  // namespace

extern "C" {

int wsu_srm_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream) {
    return count_launch("srm_counts", "srm_counts memset", "srm_counts_kernel", srm_counts_kernel, CT_THREADS, 0, x_u8, counts,
                        (size_t)SR_TABLES * SR_BINS, n, h, w, 0, SR_ROWS, CT_COLS, stream);
}

}  // extern "C"
