// What K50 (srm_minmax.hip), K54 (srm_fans.hip) and K55 (srm_edge.hip) share: a slice of min/max tables over the sets of up to eight member
// residuals, in K50's organisation (srm_minmax.hip has the account of it), the members' digits in WORDS words per centre.  The digit and
// the binning of a row's runs are srm_runs.h's.  A SPEC says what a class is:
//   UP, S        the rows above / below the centre row that its taps read, and the shift of the 19 centres (columns c - S + t);
//   WORDS        its members' digits + 2 packed a byte each, member k in byte k % 4 of word k / 4;
//   members(k)   the members of set k of the class as bits;  reach(member, side)  how far a member's taps reach up, down, left, right;
//   digits(px, q2, P)  the packed digits of the step, from px(j, col) = pixel (rho + j, c - S + col).
// A workgroup is K49's: the strip tile of wsu_count.h, a thread walking SS_TRT rows of its strip in SS_TRT + 3 steps, scan h in
// steps 0 .. SS_TRT-1 and the scan-v run that ENDS in the row in steps 3 .. SS_TRT+2; the tables of the slice in LDS that the four waves
// add to with LDS atomics, except the centre bins, which get what is left of the thread's counted updates (a closed form of its rows and
// column masks) after those that HotBins noted as gone elsewhere: a constant plane takes no atomic at all.
#pragma once
#include "srm_runs.h"

constexpr int SS_TRT = 8, SS_STEPS = SS_TRT + 3, SS_ROWS = CT_GROUPS * SS_TRT, SS_DIGITS = RUN_DIGITS, SS_BINS = RUN_BINS;
static_assert(2ll * SS_ROWS * CT_COLS < (1ll << 32), "a tile's 32-bit bins must hold every update of the tile");
using SsHot = HotBins<2, 16, 2 * 16 * SS_TRT>;          // a set's two tables (scan h, scan v) to a register; a thread adds 2 x 16 x SS_TRT to one

template <int SETS> struct SsState {
    uint32_t* hist;                                     // [2 * SETS][SS_BINS], the workgroup's
    SsHot other[SETS];                                  // per set (field 0: scan h, 1: scan v) the thread's counted updates that did NOT go to the centre bin
    uint32_t above[2 * SETS][4];                        // per set and half (lo, hi): byte i = the digits (+2) of the three rows above in column c + i, base 5
};

// where the thread is: rem = how many of the row's pixels lie at or after its column c (capped at 32), first = c == 0; rho the centre
// row of the step m, h the image's rows
struct SsAt { int rem; bool first; long long rho; int h, m; };

// a set's two tables 2 SET (scan h) and 2 SET + 1 (scan v) to run_bins: run i counts where bit i of mh / mv is set; outside the centre
// bin it takes the LDS atomic and is noted
template <int SETS> struct SsCounter {
    SsState<SETS>& s;
    uint32_t mh, mv;
    template <int TABLE, int SCAN> __device__ __forceinline__ void count(uint32_t bin, int i) {
        if (((bin ^ (uint32_t)RUN_CENTRE) & run_bit(SCAN ? mv : mh, i)) != 0u) {
            atomicAdd(&s.hist[(TABLE + SCAN) * SS_BINS + bin], 1u);
            s.other[TABLE >> 1].add(SCAN, true);
        }
    }
};

// one half of a set at one step: dg, its digits + 2 at the 19 centres
template <int SET, int HALF, int S, int SETS>
__device__ __forceinline__ void ss_runs(SsState<SETS>& s, const int (&dg)[SS_DIGITS], uint32_t mh, uint32_t mv) {
    asm volatile("" : "+v"(mh), "+v"(mv));            // the masks' bits are tested here, not ahead of the loop in scalar register pairs
    SsCounter<SETS> counter{s, mh, mv};
    run_bins<2 * SET, S>(counter, dg, s.above[2 * SET + HALF]);
}

// the columns of a set that reaches l to the left and rt to the right: bit i set where the run of scan h that starts at column c - S + i
// (and ends three on), or the run of scan v in column c + i, has its taps in the row
template <int S> __device__ __forceinline__ uint32_t ss_cols_h(const SsAt& at, int l, int rt) {
    return run_low_bits(at.rem + S - rt - 3) & ~(at.first ? run_low_bits(l + S) : 0u);
}
__device__ __forceinline__ uint32_t ss_cols_v(const SsAt& at, int l, int rt) { return run_low_bits(at.rem - rt) & ~(at.first ? run_low_bits(l) : 0u); }

// how far the taps of the members MEMBERS (bits) of SPEC reach on `side` (0 up, 1 down, 2 left, 3 right): the largest over the members
template <class SPEC> constexpr int ss_reach(int members, int side) {
    int r = 0;
    for (int k = 0; k < 4 * SPEC::WORDS; ++k)
        if (members >> k & 1) r = SPEC::reach(k, side) > r ? SPEC::reach(k, side) : r;
    return r;
}

// One set at one step.  P: the members' digits + 2 at the 19 centres; MEMBERS: which of them the set takes.  A run counts where the set's
// whole reach is in the image.
template <class SPEC, int SET, int MEMBERS, int SETS>
__device__ __forceinline__ void ss_set(SsState<SETS>& s, uint32_t (&P)[SPEC::WORDS][SS_DIGITS], const SsAt& at) {
    constexpr int S = SPEC::S;
    // what one set unpacked of P is not kept for the next
#pragma unroll
    for (int k = 0; k < SPEC::WORDS; ++k)
#pragma unroll
        for (int t = 0; t < SS_DIGITS; ++t) asm volatile("" : "+v"(P[k][t]));
    constexpr int u = ss_reach<SPEC>(MEMBERS, 0), dn = ss_reach<SPEC>(MEMBERS, 1), l = ss_reach<SPEC>(MEMBERS, 2), rt = ss_reach<SPEC>(MEMBERS, 3);
    const bool row_in = at.rho + dn < at.h;
    const uint32_t mh = at.m < SS_TRT && at.rho >= u && row_in ? ss_cols_h<S>(at, l, rt) : 0u;
    const uint32_t mv = at.m >= 3 && at.rho - 3 >= u && row_in ? ss_cols_v(at, l, rt) : 0u;
    int dg[SS_DIGITS];
#pragma unroll
    for (int t = 0; t < SS_DIGITS; ++t) {
        int mn = 4;
#pragma unroll
        for (int k = 0; k < 4 * SPEC::WORDS; ++k)
            if (MEMBERS >> k & 1) mn = min(mn, (int)(P[k >> 2][t] >> (8 * (k & 3)) & 255u));
        dg[t] = mn;
    }
    ss_runs<SET, 0, S>(s, dg, mh, mv);
#pragma unroll
    for (int t = 0; t < SS_DIGITS; ++t) {
        int mx = 0;
#pragma unroll
        for (int k = 0; k < 4 * SPEC::WORDS; ++k)
            if (MEMBERS >> k & 1) mx = max(mx, (int)(P[k >> 2][t] >> (8 * (k & 3)) & 255u));
        dg[t] = 4 - mx;                                 // the negated digit
    }
    ss_runs<SET, 1, S>(s, dg, mh, mv);
}

// all the updates that the thread counted for a set over its steps, scan h in the low half and scan v in the high one (the fields of SsHot)
template <class SPEC, int MEMBERS> __device__ __forceinline__ uint32_t ss_counted(const SsAt& at, long long r0) {
    constexpr int u = ss_reach<SPEC>(MEMBERS, 0), dn = ss_reach<SPEC>(MEMBERS, 1), l = ss_reach<SPEC>(MEMBERS, 2), rt = ss_reach<SPEC>(MEMBERS, 3);
    const long long last = (long long)at.h - dn;        // centre rows rho < last
    const int rows_h = (int)max(min(r0 + SS_TRT, last) - max(r0, (long long)u), 0ll);
    const int rows_v = (int)max(min(r0 + SS_TRT + 3, last) - max(r0, (long long)u) - 3, 0ll);
    return 2u * (uint32_t)(rows_h * __popc(ss_cols_h<SPEC::S>(at, l, rt))) + ((2u * (uint32_t)(rows_v * __popc(ss_cols_v(at, l, rt)))) << 16);
}

// the sets SET0 + K of the class at one step, and their centre bins: the counted updates less those that went elsewhere
template <class SPEC, int SET0, int SETS, int... K>
__device__ __forceinline__ void ss_sets(SsState<SETS>& s, uint32_t (&P)[SPEC::WORDS][SS_DIGITS], const SsAt& at, std::integer_sequence<int, K...>) {
    (ss_set<SPEC, K, SPEC::members(SET0 + K)>(s, P, at), ...);
}
template <class SPEC, int SET0, int SETS, int... K>
__device__ __forceinline__ void ss_centres(const SsState<SETS>& s, const SsAt& at, long long r0, bool live, std::integer_sequence<int, K...>) {
    ([&] {
        SsHot centre;
        centre.v = live ? ss_counted<SPEC, SPEC::members(SET0 + K)>(at, r0) - s.other[K].v : 0u;
        centre.fold(s.hist + 2 * K * SS_BINS + RUN_CENTRE, SS_BINS);
    }(), ...);
}

// one slice: the sets SET0 .. SET0 + SETS - 1 of the class SPEC at the step q2, their 2 SETS tables to counts[row ..]; hist: 2 SETS x 625 words
template <class SPEC, int SET0, int SETS>
__device__ __forceinline__ void ss_slice(uint32_t* __restrict__ hist, const uint8_t* __restrict__ img, unsigned long long* __restrict__ counts,
                                         size_t row, int q2, int h, int w, int tiles_c) {
    constexpr int UP = SPEC::UP, WIN = 2 * UP + 1, S = SPEC::S;
    const auto sets = std::make_integer_sequence<int, SETS>{};
    const int tid = threadIdx.x;
    const CtStrip st = ct_strip_rows<SS_TRT>(tiles_c, w);
    const long long c = st.c, r0 = st.r0;
    const bool live = c < w && r0 < h;
    SsState<SETS> s;
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
    for (int i = tid; i < 2 * SETS * SS_BINS; i += CT_THREADS) hist[i] = 0u;              // (behind the window's loads)
    __syncthreads();
    SsAt at;
    at.rem = st.rem, at.first = c == 0, at.h = h, at.rho = r0, at.m = 0;
    if (live) {
#pragma unroll 1
        for (int m = 0; m < SS_STEPS; ++m) {
            at.rho = r0 + m, at.m = m;
            auto px = [&](int j, int col) { return ct_px(win[UP + j], col - S); };         // pixel (rho + j, c - S + col)
            uint32_t P[SPEC::WORDS][SS_DIGITS];
            SPEC::digits(px, q2, P);
            ss_sets<SPEC, SET0>(s, P, at, sets);
#pragma unroll
            for (int j = 0; j < WIN - 1; ++j) win[j] = win[j + 1];
            long long cc = c;
            asm volatile("" : "+v"(cc));                // the load's 24 clamped column offsets are made here, not kept across the loop
            win[WIN - 1] = m + 1 < SS_STEPS ? load(at.rho + UP + 1, cc) : ct_no_row();
        }
    }
    ss_centres<SPEC, SET0>(s, at, r0, live, sets);
    count_flush<CT_WAVES, uint32_t, 1>(hist, 2 * SETS * SS_BINS, counts, row);
}
