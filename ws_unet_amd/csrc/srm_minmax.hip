// K50: the co-occurrence counts of the min/max submodels of the spatial rich model (SRM; Fridrich, Kodovsky, IEEE TIFS 7(3), 2012) on the
// directional first-, second- and third-order residuals, the integer part of ws_unet_amd/srm.py's `features_minmax`.  Not part of the
// reference.  include/wsu.h has the definition: four directional residuals per class and pixel, K49's digit -2 .. 2 of each at one step
// q2; a set of residuals has the digits lo = min and hi = max over its members; a table counts per run of four positions along a row
// (scan h) or down a column (scan v) the four lo digits at their bin and the four hi digits at the bin of their negation: 118 tables of
// 625 bins, 236 updates per pixel.
//
// 118 tables are 295 000 bytes, more than a CU's LDS, so the work is cut by (class, q2) into MM_SLICES = 8 slices of 14 (S1, S3: seven
// sets) or 16 (S2: eight) tables, 35 000 or 40 000 bytes: blockIdx.z is the slice, and a workgroup is K49's otherwise -- the strip tile of
// wsu_count.h, a thread walking MM_TRT rows of its strip:
//   * a step has the rows rho-UP .. rho+UP in registers (CtRow each; UP = 2 for S3, else 1) and computes the four members' digits at
//     the 19 centres of row rho, columns c - S + t (S = 1 for S3, whose E reads two columns to the right; else 0), ONCE, a byte each in
//     19 words; a set's lo and hi are v_min3 / v_max3 over the bytes it takes, and hi is negated (4 - hi in digits + 2), so both
//     halves count through the same code;
//   * scan h: the 16 runs of that row, run i from digits i .. i+3; scan v: the run that ENDS in this row at column c + i, from a byte
//     per set, half and column that holds the three digits above as a base-5 number.  The run's top row is rho - 3, so a thread takes
//     MM_TRT + 3 steps: steps 0 .. MM_TRT-1 count scan h, steps 3 .. MM_TRT+2 scan v, and every run belongs to exactly one thread;
//   * one set of tables per workgroup that its four waves add to with LDS atomics, except the centre bins, where a smooth or saturated
//     plane sends every update (lo = hi = 0): a thread notes in HotBins fields the updates that went to ANOTHER bin, and the centre
//     bin gets what is left of the thread's counted updates, which are a closed form of its rows and column masks.
// Registers, what was compiled and dropped, and the measurements: DESIGN.md 4-srmmm, profiles/r38/.
#include "wsu_count.h"

namespace {

constexpr int MM_TRT = 8, MM_STEPS = MM_TRT + 3, MM_ROWS = CT_GROUPS * MM_TRT, MM_DIGITS = 19;
constexpr int MM_TABLES = 118, MM_BINS = 625, MM_CENTRE = 312, MM_SLICES = 8, MM_SLICE_TABLES = 16;
static_assert(2ll * MM_ROWS * CT_COLS < (1ll << 32), "a tile's 32-bit bins must hold every update of the tile");
using MmHot = HotBins<2, 16, 2 * 16 * MM_TRT>;          // a set's two tables (scan h, scan v) to a register; a thread adds 2 x 16 x MM_TRT to one

// the members of a set as bits: S1 / S3 W, E, N, S; S2 h, v, d, m
constexpr int MA = 1, MB = 2, MC = 4, MD = 8;

template <int SETS> struct MmState {
    uint32_t* hist;                                     // [2 * SETS][MM_BINS], the workgroup's
    MmHot other[SETS];                                  // per set (field 0: scan h, 1: scan v) the thread's counted updates that did NOT go to the centre bin
    uint32_t above[2 * SETS][4];                        // per set and half (lo, hi): byte i = the digits (+2) of the three rows above in column c + i, base 5
};

// where the thread is: rem = how many of the row's pixels lie at or after its column c (capped at 32), first = c == 0; rho the centre
// row of the step m, h the image's rows
struct MmAt { int rem; bool first; long long rho; int h, m; };

__device__ __forceinline__ uint32_t mm_bit(uint32_t mask, int i) { return (uint32_t)((int)(mask << (31 - i)) >> 31); }
__device__ __forceinline__ uint32_t mm_low_bits(int n) { return (1u << min(max(n, 0), 16)) - 1u; }

// one update of TABLE (of the slice), counted when `counted` is -1 (not 0): outside the centre bin it takes the LDS atomic and is noted
template <int TABLE, int SETS> __device__ __forceinline__ void mm_count(MmState<SETS>& s, uint32_t bin, uint32_t counted) {
    if (((bin ^ (uint32_t)MM_CENTRE) & counted) != 0u) {
        atomicAdd(&s.hist[TABLE * MM_BINS + bin], 1u);
        s.other[TABLE >> 1].add(TABLE & 1, true);
    }
}

// one half of a set at one step: dg, its digits + 2 at the 19 centres.  Table 2 SET: scan h, run i of digits i .. i+3, counted where bit i
// of mh is set; table 2 SET + 1: scan v, digit i + S (column c + i) under the three above it, where bit i of mv is set
template <int SET, int HALF, int S, int SETS>
__device__ __forceinline__ void mm_runs(MmState<SETS>& s, const int (&dg)[MM_DIGITS], uint32_t mh, uint32_t mv) {
    asm volatile("" : "+v"(mh), "+v"(mv));            // the masks' bits are tested here, not ahead of the loop in scalar register pairs
    int pair[MM_DIGITS - 1];
#pragma unroll
    for (int t = 0; t < MM_DIGITS - 1; ++t) pair[t] = dg[t] * 5 + dg[t + 1];
#pragma unroll
    for (int i = 0; i < 16; ++i) mm_count<2 * SET>(s, (uint32_t)(pair[i] * 25 + pair[i + 2]), mm_bit(mh, i));
    uint32_t (&above)[4] = s.above[2 * SET + HALF];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        uint32_t now = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * g + j;
            const uint32_t bin = ((above[g] >> (8 * j)) & 255u) * 5u + (uint32_t)dg[i + S];
            mm_count<2 * SET + 1>(s, bin, mm_bit(mv, i));
            now |= (bin % 125u) << (8 * j);
        }
        above[g] = now;
    }
}

// the columns of a set that reaches l to the left and rt to the right: bit i set where the run of scan h that starts at column c - S + i
// (and ends three on), or the run of scan v in column c + i, has its taps in the row
template <int S> __device__ __forceinline__ uint32_t mm_cols_h(const MmAt& at, int l, int rt) {
    return mm_low_bits(at.rem + S - rt - 3) & ~(at.first ? mm_low_bits(l + S) : 0u);
}
__device__ __forceinline__ uint32_t mm_cols_v(const MmAt& at, int l, int rt) { return mm_low_bits(at.rem - rt) & ~(at.first ? mm_low_bits(l) : 0u); }

// One set at one step.  P: the four members' digits + 2 at the 19 centres, a byte each (member A the lowest); MEMBERS: which of them the
// set takes; REACH: how far the members' taps reach.  A run counts where the set's whole reach is in the image.
template <int SET, int MEMBERS, int S, class REACH, int SETS>
__device__ __forceinline__ void mm_set(MmState<SETS>& s, uint32_t (&P)[MM_DIGITS], const MmAt& at) {
    // what one set unpacked of P is not kept for the next (76 digits would stay in registers beside the 19 words they come from)
#pragma unroll
    for (int t = 0; t < MM_DIGITS; ++t) asm volatile("" : "+v"(P[t]));
    constexpr int u = REACH::of(MEMBERS, 0), dn = REACH::of(MEMBERS, 1), l = REACH::of(MEMBERS, 2), rt = REACH::of(MEMBERS, 3);
    const bool row_in = at.rho + dn < at.h;
    const uint32_t mh = at.m < MM_TRT && at.rho >= u && row_in ? mm_cols_h<S>(at, l, rt) : 0u;
    const uint32_t mv = at.m >= 3 && at.rho - 3 >= u && row_in ? mm_cols_v(at, l, rt) : 0u;
    int dg[MM_DIGITS];
#pragma unroll
    for (int t = 0; t < MM_DIGITS; ++t) {
        int mn = 4;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (MEMBERS >> k & 1) mn = min(mn, (int)(P[t] >> (8 * k) & 255u));
        dg[t] = mn;
    }
    mm_runs<SET, 0, S>(s, dg, mh, mv);
#pragma unroll
    for (int t = 0; t < MM_DIGITS; ++t) {
        int mx = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (MEMBERS >> k & 1) mx = max(mx, (int)(P[t] >> (8 * k) & 255u));
        dg[t] = 4 - mx;                                 // the negated digit
    }
    mm_runs<SET, 1, S>(s, dg, mh, mv);
}

// all the updates that the thread counted for a set over its steps, scan h in the low half and scan v in the high one (the fields of MmHot)
template <int MEMBERS, int S, class REACH> __device__ __forceinline__ uint32_t mm_counted(const MmAt& at, long long r0) {
    constexpr int u = REACH::of(MEMBERS, 0), dn = REACH::of(MEMBERS, 1), l = REACH::of(MEMBERS, 2), rt = REACH::of(MEMBERS, 3);
    const long long last = (long long)at.h - dn;        // centre rows rho < last
    const int rows_h = (int)max(min(r0 + MM_TRT, last) - max(r0, (long long)u), 0ll);
    const int rows_v = (int)max(min(r0 + MM_TRT + 3, last) - max(r0, (long long)u) - 3, 0ll);
    return 2u * (uint32_t)(rows_h * __popc(mm_cols_h<S>(at, l, rt))) + ((2u * (uint32_t)(rows_v * __popc(mm_cols_v(at, l, rt)))) << 16);
}

// the digit + 2 of a residual R at the step q2 / 2: sign(R) min((4|R| + q2) / (2 q2), 2) is (4|R| >= q2) + (4|R| >= 3 q2) with the sign
__device__ __forceinline__ int mm_digit(int R, int q2) {
    const int mag = 4 * abs(R), sgn = R >> 31;
    const int m = (mag >= q2 ? 1 : 0) + (mag >= 3 * q2 ? 1 : 0);
    return (m ^ sgn) - sgn + 2;
}

// reach of the members' taps (up, down, left, right), the largest over the members of a set
struct MmReach1 {                                       // S1: W, E, N, S
    static constexpr int of(int members, int side) {
        return side == 0 ? (members & MC ? 1 : 0) : side == 1 ? (members & MD ? 1 : 0) : side == 2 ? (members & MA ? 1 : 0) : (members & MB ? 1 : 0);
    }
};
struct MmReach2 { static constexpr int of(int, int) { return 1; } };     // S2: every set has h or v with d or m, or both h and v
struct MmReach3 {                                       // S3: W reaches 2 left and 1 right, E 1 and 2, N 2 up and 1 down, S 1 and 2
    static constexpr int of(int members, int side) {
        return side == 0 ? (members & MC ? 2 : members & MD ? 1 : 0) : side == 1 ? (members & MD ? 2 : members & MC ? 1 : 0)
             : side == 2 ? (members & MA ? 2 : members & MB ? 1 : 0) : (members & MB ? 2 : members & MA ? 1 : 0);
    }
};

// the sets' members in order: S1 / S3 WE, NS, WENS, WNE, ESW, SWN, NES; S2 hv, hvdm, hvd, hvm, hd, hm, vd, vm
constexpr int MM_SETS_13[7] = {MA | MB, MC | MD, MA | MB | MC | MD, MA | MC | MB, MB | MD | MA, MD | MA | MC, MC | MB | MD};
constexpr int MM_SETS_2[8] = {MA | MB, MA | MB | MC | MD, MA | MB | MC, MA | MB | MD, MA | MC, MA | MD, MB | MC, MB | MD};
template <int CLS, int K> constexpr int mm_members() { return CLS == 2 ? MM_SETS_2[K] : MM_SETS_13[K < 7 ? K : 0]; }

// every set of the class at one step
template <int CLS, int S, class REACH, int SETS, int... K>
__device__ __forceinline__ void mm_sets(MmState<SETS>& s, uint32_t (&P)[MM_DIGITS], const MmAt& at, std::integer_sequence<int, K...>) {
    (mm_set<K, mm_members<CLS, K>(), S, REACH>(s, P, at), ...);
}
// the centre bins: the counted updates less those that went elsewhere, a set's two tables in the two fields of MmHot
template <int CLS, int S, class REACH, int SETS, int... K>
__device__ __forceinline__ void mm_centres(const MmState<SETS>& s, const MmAt& at, long long r0, bool live, std::integer_sequence<int, K...>) {
    ([&] {
        MmHot centre;
        centre.v = live ? mm_counted<mm_members<CLS, K>(), S, REACH>(at, r0) - s.other[K].v : 0u;
        centre.fold(s.hist + 2 * K * MM_BINS + MM_CENTRE, MM_BINS);
    }(), ...);
}

// one slice: class CLS at the step q2, its tables to counts[row ..]
template <int CLS>
__device__ __forceinline__ void mm_slice(uint32_t* __restrict__ hist, const uint8_t* __restrict__ img, unsigned long long* __restrict__ counts,
                                         size_t row, int q2, int h, int w, int tiles_c) {
    constexpr int SETS = CLS == 2 ? 8 : 7, UP = CLS == 3 ? 2 : 1, WIN = 2 * UP + 1, S = CLS == 3 ? 1 : 0;
    using REACH = std::conditional_t<CLS == 1, MmReach1, std::conditional_t<CLS == 2, MmReach2, MmReach3>>;
    const auto sets = std::make_integer_sequence<int, SETS>{};
    const int tid = threadIdx.x;
    const CtStrip st = ct_strip_rows<MM_TRT>(tiles_c, w);
    const long long c = st.c, r0 = st.r0;
    const bool live = c < w && r0 < h;
    MmState<SETS> s;
    s.hist = hist;
#pragma unroll
    for (int k = 0; k < 2 * SETS; ++k)
#pragma unroll
        for (int g = 0; g < 4; ++g) s.above[k][g] = 0u;
    // the window: rows rho - UP .. rho + UP around the centre row rho = r0 + m; a row outside the image is never part of a counted run
    auto load = [&](long long r, long long cc) { return live && r >= 0 && r < h ? ct_load_row(img + (size_t)r * w, cc, w) : ct_no_row(); };
    CtRow win[WIN];
#pragma unroll
    for (int j = 0; j < WIN; ++j) win[j] = load(r0 - UP + j, c);
    for (int i = tid; i < 2 * SETS * MM_BINS; i += CT_THREADS) hist[i] = 0u;              // (behind the window's loads)
    __syncthreads();
    MmAt at;
    at.rem = st.rem, at.first = c == 0, at.h = h, at.rho = r0, at.m = 0;
    if (live) {
#pragma unroll 1
        for (int m = 0; m < MM_STEPS; ++m) {
            at.rho = r0 + m, at.m = m;
            auto px = [&](int j, int col) { return ct_px(win[UP + j], col - S); };         // pixel (rho + j, c - S + col)
            auto pack = [](int a, int b, int cc, int d) { return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)cc << 16 | (uint32_t)d << 24; };
            uint32_t P[MM_DIGITS];                      // the four members' digits + 2 at centre c - S + t, a byte each
            if constexpr (CLS == 1) {
                // W(t) = -g(t), E(t) = g(t + 1) with g(t) = X[t] - X[t-1]: the digit is odd, 4 - d in digits + 2
                int g[MM_DIGITS + 1];
#pragma unroll
                for (int t = 0; t < MM_DIGITS + 1; ++t) g[t] = mm_digit(px(0, t) - px(0, t - 1), q2);
#pragma unroll
                for (int t = 0; t < MM_DIGITS; ++t)
                    P[t] = pack(4 - g[t], g[t + 1], mm_digit(px(-1, t) - px(0, t), q2), mm_digit(px(1, t) - px(0, t), q2));
            } else if constexpr (CLS == 2) {
#pragma unroll
                for (int t = 0; t < MM_DIGITS; ++t) {
                    const int x2 = 2 * px(0, t);
                    P[t] = pack(mm_digit(px(0, t - 1) - x2 + px(0, t + 1), q2), mm_digit(px(-1, t) - x2 + px(1, t), q2),
                                mm_digit(px(-1, t - 1) - x2 + px(1, t + 1), q2), mm_digit(px(-1, t + 1) - x2 + px(1, t - 1), q2));
                }
            } else {
                // W(t) = -k(t), E(t) = k(t + 1) with k(t) = X[t-2] - 3 X[t-1] + 3 X[t] - X[t+1], which is E at the centre t - 1
                int k[MM_DIGITS + 1];
#pragma unroll
                for (int t = 0; t < MM_DIGITS + 1; ++t) k[t] = mm_digit(px(0, t - 2) - 3 * px(0, t - 1) + 3 * px(0, t) - px(0, t + 1), q2);
#pragma unroll
                for (int t = 0; t < MM_DIGITS; ++t)
                    P[t] = pack(4 - k[t], k[t + 1], mm_digit(px(1, t) - 3 * px(0, t) + 3 * px(-1, t) - px(-2, t), q2),
                                mm_digit(px(-1, t) - 3 * px(0, t) + 3 * px(1, t) - px(2, t), q2));
            }
            mm_sets<CLS, S, REACH>(s, P, at, sets);
#pragma unroll
            for (int j = 0; j < WIN - 1; ++j) win[j] = win[j + 1];
            long long cc = c;
            asm volatile("" : "+v"(cc));                // the load's 24 clamped column offsets are made here, not kept across the loop
            win[WIN - 1] = m + 1 < MM_STEPS ? load(at.rho + UP + 1, cc) : ct_no_row();
        }
    }
    mm_centres<CLS, S, REACH>(s, at, r0, live, sets);
    count_flush<CT_WAVES, uint32_t, 1>(hist, 2 * SETS * MM_BINS, counts, row);
}

__global__ __launch_bounds__(CT_THREADS) void srm_minmax_counts_kernel(const uint8_t* __restrict__ xu8, unsigned long long* __restrict__ counts,
                                                                       int h, int w, int tiles_c) {
    __shared__ uint32_t hist[MM_SLICE_TABLES * MM_BINS];
    const int nn = blockIdx.y, slice = blockIdx.z;      // slices 0, 1: S1 at q2 = 2, 4; 2 .. 4: S2 at 4, 6, 8; 5 .. 7: S3 at 6, 9, 12
    const uint8_t* img = xu8 + (size_t)nn * h * w;
    const size_t row = (size_t)nn * MM_TABLES * MM_BINS;
    if (slice < 2) mm_slice<1>(hist, img, counts, row + (size_t)(14 * slice) * MM_BINS, 2 + 2 * slice, h, w, tiles_c);
    else if (slice < 5) mm_slice<2>(hist, img, counts, row + (size_t)(28 + 16 * (slice - 2)) * MM_BINS, 2 * slice, h, w, tiles_c);
    else mm_slice<3>(hist, img, counts, row + (size_t)(76 + 14 * (slice - 5)) * MM_BINS, 3 * slice - 9, h, w, tiles_c);
}

}  // namespace

extern "C" {

int wsu_srm_minmax_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream) {
    return count_launch_slices("srm_minmax_counts", "srm_minmax_counts memset", "srm_minmax_counts_kernel", srm_minmax_counts_kernel,
                               CT_THREADS, 0, x_u8, counts, (size_t)MM_TABLES * MM_BINS, n, h, w, 0, MM_ROWS, CT_COLS, MM_SLICES, stream);
}

}  // extern "C"
