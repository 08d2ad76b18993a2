// What the exact count kernels share (ols.hip: K24; ols5.hip: K56; structural.hip: K25, K26; spam.hip: K36; jpeg_history.hip: K31; the rich model's five
// -- srm.hip: K49, srm_weighted.hip: K52, and through srm_sets.h and srm_runs.h srm_minmax.hip: K50, srm_fans.hip: K54, srm_edge.hip: K55):
// the strip tile and its loaders, the wave fold, the packed counter of the hot bins, a workgroup's flush and the host's launch set-up.  Every output is a table of exact integers that the kernels only ADD to, so the bits depend on no order: the entry
// point zeroes the table on the stream, a workgroup sums its tile in 32- or 64-bit partials and adds each non-zero sum with one 64-bit
// vector atomic.
#pragma once
#include "wsu_device.h"

// ---- the strip tile (K25, K26, K36) ---------------------------------------------------------------------------------------------------------
// One workgroup owns CT_ROWS x CT_COLS pixels of one image: 32 strips of 16 columns by 8 row groups, a thread walking its strip down CT_TRT
// rows.  (K24's 64 x 256 interior tile and K31's runs of 8 x 8 blocks are their own.)
constexpr int CT_TRT = 4, CT_STRIPS = 32, CT_GROUPS = 8, CT_THREADS = CT_STRIPS * CT_GROUPS, CT_WAVES = CT_THREADS / 64;
constexpr int CT_COLS = CT_STRIPS * 16, CT_ROWS = CT_GROUPS * CT_TRT;

// a thread's strip in workgroup blockIdx.x of a grid with tiles_c column tiles: its first column c (a multiple of 16), its first row r0 (past
// h in the last tile's idle groups) and rem, how many of the row's w pixels lie at or after c: 0 where the strip is outside the image,
// capped at 16 + reach, which is all a kernel that looks `reach` columns past the strip asks
struct CtStrip { long long c, r0; int rem; };
__device__ __forceinline__ CtStrip ct_strip(int tiles_c, int w, int reach) {
    CtStrip s;
    s.c = (long long)(blockIdx.x % tiles_c) * CT_COLS + (threadIdx.x & (CT_STRIPS - 1)) * 16;
    s.r0 = (long long)(blockIdx.x / tiles_c) * CT_ROWS + (threadIdx.x / CT_STRIPS) * CT_TRT;
    s.rem = (int)min(max((long long)w - s.c, 0ll), (long long)(16 + reach));
    return s;
}
// the same for a kernel whose threads walk TRT rows (the rich model's: 8, a tile of CT_GROUPS * TRT rows): c, r0, and rem capped at 32
template <int TRT> __device__ __forceinline__ CtStrip ct_strip_rows(int tiles_c, int w) {
    CtStrip s;
    s.c = (long long)(blockIdx.x % tiles_c) * CT_COLS + (threadIdx.x & (CT_STRIPS - 1)) * 16;
    s.r0 = (long long)(blockIdx.x / tiles_c) * (CT_GROUPS * TRT) + (threadIdx.x / CT_STRIPS) * TRT;
    s.rem = (int)min(max((long long)w - s.c, 0ll), 32ll);
    return s;
}

// ---- loads: no load is outside the image; a missing pixel only clears a predicate of the caller -----------------------------------------------
// the pixels row[first + i], i < 4 * WORDS, as little-endian words, every index clamped into 0 .. last (not branched on: independent byte
// loads).  A clamped pixel repeats the row's first or last one and is never counted.
template <int WORDS, class I>
__device__ __forceinline__ void ct_load_clamped(const uint8_t* __restrict__ row, I first, I last, uint32_t (&v)[WORDS]) {
#pragma unroll
    for (int i = 0; i < WORDS; ++i) v[i] = 0u;
#pragma unroll
    for (int i = 0; i < 4 * WORDS; ++i) v[i >> 2] |= (uint32_t)row[min(max(first + (I)i, (I)0), last)] << (8 * (i & 3));
}

// a strip p[0 .. 15] of a row that has rem >= 1 pixels left from p on: ONE 16-byte load where the strip lies inside the row and its address is a
// multiple of 16, else (the ragged last strip of a row, every strip of a row whose base the width or the plane's base has shifted) byte loads
__device__ __forceinline__ u32x4 ct_load_strip(const uint8_t* __restrict__ p, int rem) {
    if (rem >= 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const u32x4*>(p);
    uint32_t v[4];
    ct_load_clamped<4>(p, 0, rem - 1, v);
    return mk_u4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ int ct_px(const u32x4& s, int i) { return (int)((s[i >> 2] >> (8 * (i & 3))) & 255u); }

// a strip with the four columns on either side of it: c-4 .. c-1 (left), c .. c+15 (mid), c+16 .. c+19 (right)
struct CtRow { uint32_t left; u32x4 mid; uint32_t right; };
__device__ __forceinline__ CtRow ct_no_row() { CtRow r; r.left = 0u; r.mid = mk_u4(0u, 0u, 0u, 0u); r.right = 0u; return r; }

// ... of the strip at column c < w of the image row `row`, by ONE decision per row (a decision per word made every word wait for the one
// before it).  Words: the strip is whole (c + 16 <= w), its address a multiple of 4 and the word right of it whole or wholly outside the
// row; the strip is one 16-byte load where its address allows it, four words else.  A side word outside the row (left of the first strip,
// right of a strip that ends the row) belongs to no counted run, so the strip's own first / last word is read in its place.  Bytes:
// everything else, 24 clamped loads.
__device__ __forceinline__ CtRow ct_load_row(const uint8_t* __restrict__ row, long long c, int w) {
    const uint8_t* p = row + c;
    CtRow r;
    if ((c + 20 <= w || c + 16 == w) && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        r.left = *reinterpret_cast<const uint32_t*>(p - (c > 0 ? 4 : 0));
        r.right = *reinterpret_cast<const uint32_t*>(p + (c + 20 <= w ? 16 : 12));
        if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            r.mid = *reinterpret_cast<const u32x4*>(p);
        } else {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
            r.mid = mk_u4(q[0], q[1], q[2], q[3]);
        }
    } else {
        uint32_t v[6];
        ct_load_clamped<6>(row, c - 4, (long long)w - 1, v);
        r.left = v[0];
        r.mid = mk_u4(v[1], v[2], v[3], v[4]);
        r.right = v[5];
    }
    return r;
}
// pixel at column c + i of the row, i = -4 .. 19
__device__ __forceinline__ int ct_px(const CtRow& r, int i) {
    const uint32_t wd = i < 0 ? r.left : i < 16 ? r.mid[i >> 2] : r.right;
    return (int)((wd >> (8 * (i & 3))) & 255u);
}

// ---- sums ------------------------------------------------------------------------------------------------------------------------------------
// sum over the wave (uint32_t, unsigned long long), valid in its lane 0
template <class T> __device__ __forceinline__ T wave_sum(T s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return s;
}

// The bins that a constant plane hits with EVERY update: same-address LDS atomics serialise (profiles/r22, profiles/r29), so a thread counts
// up to FIELDS of them in BITS-wide fields of one VGPR -- per lane, not per-wave ballots, whose masks wait in scalar register pairs and spill
// (profiles/r22) -- and the wave adds each field's sum to its histogram once.  UPDATES: what a thread adds to one field at the most.
template <int FIELDS, int BITS, int UPDATES> struct HotBins {
    static_assert(FIELDS * BITS <= 32, "the fields share one register");
    static_assert(UPDATES < (1 << BITS), "a field must hold every update of the thread");
    uint32_t v = 0u;
    __device__ __forceinline__ void add(int field, bool p) { v += p ? 1u << (BITS * field) : 0u; }
    // every lane of the wave: hist[f * stride] += the wave's sum of field f
    __device__ __forceinline__ void fold(uint32_t* __restrict__ hist, int stride) const {
#pragma unroll
        for (int f = 0; f < FIELDS; ++f) {
            const uint32_t s = wave_sum((v >> (BITS * f)) & ((1u << BITS) - 1u));
            if ((threadIdx.x & 63) == 0 && s) atomicAdd(&hist[f * stride], s);
        }
    }
};

// The end of every count kernel, by all WAVES * 64 threads of the workgroup: part holds the waves' partial sums [WAVES][k] in LDS (written
// by plain stores or LDS atomics before the call; the barrier is in here); out[row + b] += the sum over the waves, b < k, one 64-bit vector
// atomic per non-zero sum.  COPIES: how many partial tables part holds when that is not one per wave (K49, K50: one that its waves share).
template <int WAVES, class T, int COPIES = WAVES>
__device__ __forceinline__ void count_flush(const T* __restrict__ part, int k, unsigned long long* __restrict__ out, size_t row) {
    __syncthreads();
    for (int b = threadIdx.x; b < k; b += WAVES * 64) {
        T s = 0;
#pragma unroll
        for (int j = 0; j < COPIES; ++j) s += part[j * k + b];
        if (s) atomicAdd(&out[row + b], (unsigned long long)s);
    }
}

// ---- the launch ------------------------------------------------------------------------------------------------------------------------------
// The set-up of an entry over n planes of h x w pixels whose kernel(x, out, h, w, tiles_c, tail...) takes a tile of tile_r x tile_c pixels
// of a plane without its `border` outermost rows and columns per workgroup, grid (row tiles x column tiles, n): the argument checks, the
// table of n x row sums zeroed on the stream (a count kernel only adds), the launch.  The three names as in embed_launch (wsu_embed.h).
// count_launch_slices: the same with `slices` workgroups per tile and plane (grid z; K50 cuts its tables into slices that a workgroup's LDS
// holds); count_launch is the one-slice form that every other kernel takes.
template <class... P, class... A>
inline int count_launch_slices(const char* who, const char* memset_name, const char* kernel_name, void (*kernel)(P...), int threads, size_t lds,
                               const uint8_t* x, unsigned long long* out, size_t row, int n, int h, int w, int border, int tile_r, int tile_c,
                               int slices, void* stream, A... tail) {
    WSU_REQUIRE(x && out, "%s: null pointer", who);
    WSU_REQUIRE(n >= 1 && n <= 65535 && h > 2 * border && w > 2 * border, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    const long long tr = ((long long)h - 2 * border + tile_r - 1) / tile_r, tc = ((long long)w - 2 * border + tile_c - 1) / tile_c;
    WSU_REQUIRE(tr * tc <= 0x7fffffffll, "%s: image of %d x %d has too many tiles", who, h, w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out, 0, (size_t)n * row * sizeof(unsigned long long), s) != hipSuccess) return wsu_check_launch(memset_name);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tr * tc), n, slices), dim3(threads), lds, s, x, out, h, w, (int)tc, tail...);
    return wsu_check_launch(kernel_name);
}
template <class... P, class... A>
inline int count_launch(const char* who, const char* memset_name, const char* kernel_name, void (*kernel)(P...), int threads, size_t lds,
                        const uint8_t* x, unsigned long long* out, size_t row, int n, int h, int w, int border, int tile_r, int tile_c,
                        void* stream, A... tail) {
    return count_launch_slices(who, memset_name, kernel_name, kernel, threads, lds, x, out, row, n, h, w, border, tile_r, tile_c, 1, stream,
                               tail...);
}
