// Training-batch assembly (data/pairs.py): gather + dihedral transform + u8 -> [0,1] fp32, inputs and targets of a whole batch in ONE launch.
//   inputs[s] = D(op[s])(planes[idx_in[s]]) / 255.0f        covers[s] = D(op[s])(planes[idx_cov[s]]) / 255.0f
// op (include/wsu.h): bit 0 mirrors the columns, bit 1 the rows, bit 2 transposes last; output pixel (i, j) reads source (r, c) with
// (r, c) = bit 2 ? (j, i) : (i, j), then r = h-1-r if bit 1, c = w-1-c if bit 0.
//
// A workgroup owns one 64 x 64 SOURCE tile of one sample.  Its image under D is a 64 x 64 block of the output, so both sides move whole row
// segments for every op:
//   * ops 0-3 never leave the registers: a lane loads 4 source bytes of a row and stores their 4 floats to the (mirrored) output row; the
//     column mirror is the order in which the word's bytes are converted, lanes keep their order.
//   * ops 4-7 go through an LDS byte tile: rows are written as they are loaded, then a lane reads a 4 x 4 block (4 words, rows 4a..4a+3, word
//     column b) and stores one 16-byte vector to each of the 4 output rows that the block's 4 source columns become.
// LDS layout, by the bank rule of ds_read_b32 / ds_write_b32 (32 banks of 4 bytes, conflicts counted inside each 32-lane half):
//   word (row, wc) lives at dword row * 17 + (wc ^ ((row >> 5) << 1)).
//   A plain 16-dword (64-byte) pitch puts rows 4a + k of all 16 a on (k & 1) * 16 + wc: 16 lanes of a half on ONE bank.  With 17 dwords the
//   block read's bank is (4a + 17k + wc') % 32: a = 0..7 take the eight 4-bank slots, a = 8..15 would take them again -- their rows are >= 32,
//   where wc' = wc ^ 2 moves the half's two word columns {2m, 2m+1} to the other pair of banks in the slot.  32 lanes, 32 banks.
//   The row writes of a half cover two rows; 16 rows apart (16 * 17 = 16 mod 32) they take banks x..x+15 and x+16..x+31.
//   The byte-wise kernel reads one column of 32 consecutive rows per half: (17 row + const) % 32, all distinct (17 is odd; the swizzle is
//   constant inside a half); its byte writes put 4 lanes on every dword of a row, which costs that kernel nothing that matters.
#include "wsu_device.h"

namespace {

constexpr int PB_TILE = 64;            // source tile edge in pixels (= bytes)
constexpr int PB_PD = 17;              // LDS row pitch in dwords
constexpr int PB_TILE_WORDS = PB_TILE * PB_PD;

__device__ __forceinline__ int pb_lds_word(int row, int wc) { return row * PB_PD + (wc ^ ((row >> 5) << 1)); }
__device__ __forceinline__ int pb_lds_byte(int row, int col) { return 4 * pb_lds_word(row, col >> 2) + (col & 3); }

__device__ __forceinline__ float pb_unit(uint32_t byte) { return (float)byte / 255.0f; }      // IEEE division, as u8_to_unit_kernel
// the 4 bytes of a word as floats, first byte first, or last byte first (a mirrored run)
__device__ __forceinline__ f32x4 pb_unit4(uint32_t wd, bool rev) {
    const float b0 = pb_unit(wd & 0xFFu), b1 = pb_unit((wd >> 8) & 0xFFu), b2 = pb_unit((wd >> 16) & 0xFFu), b3 = pb_unit(wd >> 24);
    return rev ? mk_f4(b3, b2, b1, b0) : mk_f4(b0, b1, b2, b3);
}
// byte m of 4 words (a column of a 4 x 4 block) as floats, top row first or bottom row first
__device__ __forceinline__ f32x4 pb_col4(const uint32_t (&wd)[4], int m, bool rev) {
    const float b0 = pb_unit((wd[0] >> (8 * m)) & 0xFFu), b1 = pb_unit((wd[1] >> (8 * m)) & 0xFFu);
    const float b2 = pb_unit((wd[2] >> (8 * m)) & 0xFFu), b3 = pb_unit((wd[3] >> (8 * m)) & 0xFFu);
    return rev ? mk_f4(b3, b2, b1, b0) : mk_f4(b0, b1, b2, b3);
}

struct PbSample {
    const uint8_t *pa, *pb;            // the input's and the target's source plane
    float *oa, *ob;
    int r0, c0;                        // origin of this workgroup's source tile
    bool same, fh, fv, tr;
};

// false: the sample's index or op is out of range (the host wrapper validates; the kernel then writes nothing)
__device__ __forceinline__ bool pb_sample(PbSample& sm, const uint8_t* planes, int files, int h, int w, const int32_t* idx_in,
                                          const int32_t* idx_cov, const uint8_t* op, int max_op, int tiles_x, int tiles,
                                          float* inputs, float* covers) {
    const int s = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x % (unsigned)tiles);
    const int ia = idx_in[s], ib = idx_cov[s], o = op[s];
    if (ia < 0 || ia >= files || ib < 0 || ib >= files || o > max_op) return false;
    const size_t hw = (size_t)h * w;
    sm.pa = planes + (size_t)ia * hw; sm.pb = planes + (size_t)ib * hw;
    sm.oa = inputs + (size_t)s * hw; sm.ob = covers + (size_t)s * hw;
    sm.r0 = (t / tiles_x) * PB_TILE; sm.c0 = (t % tiles_x) * PB_TILE;
    sm.same = ia == ib; sm.fh = o & 1; sm.fv = o & 2; sm.tr = o & 4;
    return true;
}

// rows are multiples of 4 pixels and every base pointer is aligned: 4-byte loads, 16-byte stores
__global__ __launch_bounds__(256) void pair_batch_vec_kernel(const uint8_t* __restrict__ planes, int files, int h, int w,
                                                             const int32_t* __restrict__ idx_in, const int32_t* __restrict__ idx_cov,
                                                             const uint8_t* __restrict__ op, int max_op, int tiles_x, int tiles,
                                                             float* __restrict__ inputs, float* __restrict__ covers) {
    __shared__ uint32_t tile[2][PB_TILE_WORDS];
    PbSample sm;
    if (!pb_sample(sm, planes, files, h, w, idx_in, idx_cov, op, max_op, tiles_x, tiles, inputs, covers)) return;
    const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
    if (!sm.tr) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = sm.r0 + g + 16 * p, c = sm.c0 + 4 * q;
            if (r >= h || c >= w) continue;
            const size_t src = (size_t)r * w + c;
            const size_t dst = (size_t)(sm.fv ? h - 1 - r : r) * w + (sm.fh ? w - 4 - c : c);
            const f32x4 va = pb_unit4(*reinterpret_cast<const uint32_t*>(sm.pa + src), sm.fh);
            *reinterpret_cast<f32x4*>(sm.oa + dst) = va;
            *reinterpret_cast<f32x4*>(sm.ob + dst) = sm.same ? va : pb_unit4(*reinterpret_cast<const uint32_t*>(sm.pb + src), sm.fh);
        }
        return;
    }
    // (the two rows that a 32-lane half writes are 16 apart: banks x..x+15 and x+16..x+31; adjacent rows would meet on one bank)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int lr = (g >> 1) + 16 * (g & 1) + 8 * (p & 1) + 32 * (p >> 1), r = sm.r0 + lr, c = sm.c0 + 4 * q;
        if (r >= h || c >= w) continue;                                  // never read back: the block reads below test the same bounds
        const size_t src = (size_t)r * w + c;
        tile[0][pb_lds_word(lr, q)] = *reinterpret_cast<const uint32_t*>(sm.pa + src);
        if (!sm.same) tile[1][pb_lds_word(lr, q)] = *reinterpret_cast<const uint32_t*>(sm.pb + src);
    }
    __syncthreads();
    // block (a, b) = (q, g): source rows r..r+3 become 4 consecutive pixels of the output rows that source columns c..c+3 become (h == w here)
    const int r = sm.r0 + 4 * q, c = sm.c0 + 4 * g;
    if (r >= h || c >= w) return;
    uint32_t wa[4], wb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        wa[k] = tile[0][pb_lds_word(4 * q + k, g)];
        wb[k] = sm.same ? wa[k] : tile[1][pb_lds_word(4 * q + k, g)];
    }
    const int j = sm.fv ? h - 4 - r : r;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int i = sm.fh ? w - 1 - (c + m) : c + m;
        const size_t dst = (size_t)i * w + j;
        const f32x4 va = pb_col4(wa, m, sm.fv);
        *reinterpret_cast<f32x4*>(sm.oa + dst) = va;
        *reinterpret_cast<f32x4*>(sm.ob + dst) = sm.same ? va : pb_col4(wb, m, sm.fv);
    }
}

// any h, w >= 1 (rows of w % 4 != 0 pixels start unaligned in both the u8 planes and the fp32 outputs): one pixel per lane and access
__global__ __launch_bounds__(256) void pair_batch_any_kernel(const uint8_t* __restrict__ planes, int files, int h, int w,
                                                             const int32_t* __restrict__ idx_in, const int32_t* __restrict__ idx_cov,
                                                             const uint8_t* __restrict__ op, int max_op, int tiles_x, int tiles,
                                                             float* __restrict__ inputs, float* __restrict__ covers) {
    __shared__ uint32_t tile[2][PB_TILE_WORDS];
    uint8_t* ta = reinterpret_cast<uint8_t*>(tile[0]);
    uint8_t* tb = reinterpret_cast<uint8_t*>(tile[1]);
    PbSample sm;
    if (!pb_sample(sm, planes, files, h, w, idx_in, idx_cov, op, max_op, tiles_x, tiles, inputs, covers)) return;
    const int x = threadIdx.x & 63, y0 = threadIdx.x >> 6;
    if (!sm.tr) {
        const int c = sm.c0 + x;
        if (c >= w) return;
        for (int y = y0; y < PB_TILE; y += 4) {
            const int r = sm.r0 + y;
            if (r >= h) break;
            const size_t src = (size_t)r * w + c;
            const size_t dst = (size_t)(sm.fv ? h - 1 - r : r) * w + (sm.fh ? w - 1 - c : c);
            const float va = pb_unit(sm.pa[src]);
            sm.oa[dst] = va;
            sm.ob[dst] = sm.same ? va : pb_unit(sm.pb[src]);
        }
        return;
    }
    for (int y = y0; y < PB_TILE; y += 4) {
        const int r = sm.r0 + y, c = sm.c0 + x;
        if (r >= h || c >= w) continue;
        const size_t src = (size_t)r * w + c;
        ta[pb_lds_byte(y, x)] = sm.pa[src];
        if (!sm.same) tb[pb_lds_byte(y, x)] = sm.pb[src];
    }
    __syncthreads();
    // lane x walks down a source column: consecutive pixels of one output row (h == w here)
    const int r = sm.r0 + x;
    if (r >= h) return;
    const int j = sm.fv ? h - 1 - r : r;
    for (int y = y0; y < PB_TILE; y += 4) {
        const int c = sm.c0 + y;
        if (c >= w) break;
        const size_t dst = (size_t)(sm.fh ? w - 1 - c : c) * w + j;
        const float va = pb_unit(ta[pb_lds_byte(x, y)]);
        sm.oa[dst] = va;
        sm.ob[dst] = sm.same ? va : pb_unit(tb[pb_lds_byte(x, y)]);
    }
}

// ---- the same assembly with side-information planes behind the image (wsu_pair_batch_planes_f32; the reference's ParityOracle / DemosaicOracle,
// src/_defs/loader.py:73-103, which run BEFORE its flips and rotation: every plane is a function of the SOURCE pixel (r, c) and its value v):
//   parity  float(v & 1)          R  r, c both even          G  r + c odd          B  r, c both odd
// Tiling, lane roles, LDS layout and the conversion of the image plane are those of the two kernels above (plane 0 and covers hold their
// bits); a vector store of a side plane covers the 4 output pixels of the image store beside it.  A run of 4 output pixels walks 4
// consecutive source columns (ops 0-3) or rows (ops 4-7) from a multiple of 4, forwards or backwards, while the other coordinate is
// fixed: R, G and B are symmetric in (r, c), so one helper serves both.  The three Bayer planes are pure stores.
struct PbSide {
    float *par, *bay;                  // this sample's parity plane and the first of its three Bayer planes, or nullptr
    size_t hw;
};

__device__ __forceinline__ bool pb_sample_planes(PbSample& sm, PbSide& sd, const uint8_t* planes, int files, int h, int w, const int32_t* idx_in,
                                                 const int32_t* idx_cov, const uint8_t* op, int max_op, int tiles_x, int tiles, int side,
                                                 float* inputs, float* covers) {
    const int s = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x % (unsigned)tiles);
    const int ia = idx_in[s], ib = covers ? idx_cov[s] : ia, o = op[s];
    if (ia < 0 || ia >= files || ib < 0 || ib >= files || o > max_op) return false;
    const size_t hw = (size_t)h * w;
    const int np = 1 + (side & 1) + 3 * ((side >> 1) & 1);
    sm.pa = planes + (size_t)ia * hw; sm.pb = planes + (size_t)ib * hw;
    sm.oa = inputs + (size_t)s * np * hw; sm.ob = covers ? covers + (size_t)s * hw : nullptr;
    sm.r0 = (t / tiles_x) * PB_TILE; sm.c0 = (t % tiles_x) * PB_TILE;
    sm.same = ia == ib; sm.fh = o & 1; sm.fv = o & 2; sm.tr = o & 4;
    sd.par = (side & 1) ? sm.oa + hw : nullptr;
    sd.bay = (side & 2) ? sm.oa + (size_t)(1 + (side & 1)) * hw : nullptr;
    sd.hw = hw;
    return true;
}

__device__ __forceinline__ float pb_lsb(uint32_t byte) { return (float)(byte & 1u); }
__device__ __forceinline__ f32x4 pb_lsb4(uint32_t wd, bool rev) {
    const float b0 = pb_lsb(wd), b1 = pb_lsb(wd >> 8), b2 = pb_lsb(wd >> 16), b3 = pb_lsb(wd >> 24);
    return rev ? mk_f4(b3, b2, b1, b0) : mk_f4(b0, b1, b2, b3);
}
__device__ __forceinline__ f32x4 pb_lsbcol4(const uint32_t (&wd)[4], int m, bool rev) {
    const float b0 = pb_lsb(wd[0] >> (8 * m)), b1 = pb_lsb(wd[1] >> (8 * m)), b2 = pb_lsb(wd[2] >> (8 * m)), b3 = pb_lsb(wd[3] >> (8 * m));
    return rev ? mk_f4(b3, b2, b1, b0) : mk_f4(b0, b1, b2, b3);
}
// 4 output pixels at dst: their parities `lsb` (in output order) and the Bayer indicators of a run whose walking coordinate starts at a
// multiple of 4 (backwards from its last element if rev) beside a fixed coordinate of parity `fixed`
__device__ __forceinline__ void pb_side_store4(const PbSide& sd, size_t dst, f32x4 lsb, int fixed, bool rev) {
    if (sd.par) *reinterpret_cast<f32x4*>(sd.par + dst) = lsb;
    if (sd.bay) {
        const float e0 = rev ? 0.f : 1.f, e1 = 1.f - e0;
        const f32x4 even = mk_f4(e0, e1, e0, e1), odd = mk_f4(e1, e0, e1, e0), zero = mk_f4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<f32x4*>(sd.bay + dst) = fixed ? zero : even;
        *reinterpret_cast<f32x4*>(sd.bay + sd.hw + dst) = fixed ? even : odd;
        *reinterpret_cast<f32x4*>(sd.bay + 2 * sd.hw + dst) = fixed ? odd : zero;
    }
}
// one output pixel at dst from source pixel (r, c) of value v
__device__ __forceinline__ void pb_side_store1(const PbSide& sd, size_t dst, uint32_t v, int r, int c) {
    if (sd.par) sd.par[dst] = pb_lsb(v);
    if (sd.bay) {
        const int rp = r & 1, cp = c & 1;
        sd.bay[dst] = (rp | cp) ? 0.f : 1.f;
        sd.bay[sd.hw + dst] = (rp ^ cp) ? 1.f : 0.f;
        sd.bay[2 * sd.hw + dst] = (rp & cp) ? 1.f : 0.f;
    }
}

// covers == nullptr (inference): the inputs alone; idx_cov is then not read
__global__ __launch_bounds__(256) void pair_planes_vec_kernel(const uint8_t* __restrict__ planes, int files, int h, int w,
                                                              const int32_t* __restrict__ idx_in, const int32_t* __restrict__ idx_cov,
                                                              const uint8_t* __restrict__ op, int max_op, int tiles_x, int tiles, int side,
                                                              float* __restrict__ inputs, float* __restrict__ covers) {
    __shared__ uint32_t tile[2][PB_TILE_WORDS];
    PbSample sm;
    PbSide sd;
    if (!pb_sample_planes(sm, sd, planes, files, h, w, idx_in, idx_cov, op, max_op, tiles_x, tiles, side, inputs, covers)) return;
    const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
    const bool cov = sm.ob != nullptr;
    if (!sm.tr) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = sm.r0 + g + 16 * p, c = sm.c0 + 4 * q;
            if (r >= h || c >= w) continue;
            const size_t src = (size_t)r * w + c;
            const size_t dst = (size_t)(sm.fv ? h - 1 - r : r) * w + (sm.fh ? w - 4 - c : c);
            const uint32_t wa = *reinterpret_cast<const uint32_t*>(sm.pa + src);
            const f32x4 va = pb_unit4(wa, sm.fh);
            *reinterpret_cast<f32x4*>(sm.oa + dst) = va;
            if (cov) *reinterpret_cast<f32x4*>(sm.ob + dst) = sm.same ? va : pb_unit4(*reinterpret_cast<const uint32_t*>(sm.pb + src), sm.fh);
            pb_side_store4(sd, dst, pb_lsb4(wa, sm.fh), r & 1, sm.fh);
        }
        return;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int lr = (g >> 1) + 16 * (g & 1) + 8 * (p & 1) + 32 * (p >> 1), r = sm.r0 + lr, c = sm.c0 + 4 * q;
        if (r >= h || c >= w) continue;
        const size_t src = (size_t)r * w + c;
        tile[0][pb_lds_word(lr, q)] = *reinterpret_cast<const uint32_t*>(sm.pa + src);
        if (!sm.same) tile[1][pb_lds_word(lr, q)] = *reinterpret_cast<const uint32_t*>(sm.pb + src);
    }
    __syncthreads();
    const int r = sm.r0 + 4 * q, c = sm.c0 + 4 * g;
    if (r >= h || c >= w) return;
    uint32_t wa[4], wb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        wa[k] = tile[0][pb_lds_word(4 * q + k, g)];
        wb[k] = sm.same ? wa[k] : tile[1][pb_lds_word(4 * q + k, g)];
    }
    const int j = sm.fv ? h - 4 - r : r;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int i = sm.fh ? w - 1 - (c + m) : c + m;
        const size_t dst = (size_t)i * w + j;
        const f32x4 va = pb_col4(wa, m, sm.fv);
        *reinterpret_cast<f32x4*>(sm.oa + dst) = va;
        if (cov) *reinterpret_cast<f32x4*>(sm.ob + dst) = sm.same ? va : pb_col4(wb, m, sm.fv);
        pb_side_store4(sd, dst, pb_lsbcol4(wa, m, sm.fv), m & 1, sm.fv);
    }
}

__global__ __launch_bounds__(256) void pair_planes_any_kernel(const uint8_t* __restrict__ planes, int files, int h, int w,
                                                              const int32_t* __restrict__ idx_in, const int32_t* __restrict__ idx_cov,
                                                              const uint8_t* __restrict__ op, int max_op, int tiles_x, int tiles, int side,
                                                              float* __restrict__ inputs, float* __restrict__ covers) {
    __shared__ uint32_t tile[2][PB_TILE_WORDS];
    uint8_t* ta = reinterpret_cast<uint8_t*>(tile[0]);
    uint8_t* tb = reinterpret_cast<uint8_t*>(tile[1]);
    PbSample sm;
    PbSide sd;
    if (!pb_sample_planes(sm, sd, planes, files, h, w, idx_in, idx_cov, op, max_op, tiles_x, tiles, side, inputs, covers)) return;
    const int x = threadIdx.x & 63, y0 = threadIdx.x >> 6;
    const bool cov = sm.ob != nullptr;
    if (!sm.tr) {
        const int c = sm.c0 + x;
        if (c >= w) return;
        for (int y = y0; y < PB_TILE; y += 4) {
            const int r = sm.r0 + y;
            if (r >= h) break;
            const size_t src = (size_t)r * w + c;
            const size_t dst = (size_t)(sm.fv ? h - 1 - r : r) * w + (sm.fh ? w - 1 - c : c);
            const uint32_t v = sm.pa[src];
            const float va = pb_unit(v);
            sm.oa[dst] = va;
            if (cov) sm.ob[dst] = sm.same ? va : pb_unit(sm.pb[src]);
            pb_side_store1(sd, dst, v, r, c);
        }
        return;
    }
    for (int y = y0; y < PB_TILE; y += 4) {
        const int r = sm.r0 + y, c = sm.c0 + x;
        if (r >= h || c >= w) continue;
        const size_t src = (size_t)r * w + c;
        ta[pb_lds_byte(y, x)] = sm.pa[src];
        if (!sm.same) tb[pb_lds_byte(y, x)] = sm.pb[src];
    }
    __syncthreads();
    const int r = sm.r0 + x;
    if (r >= h) return;
    const int j = sm.fv ? h - 1 - r : r;
    for (int y = y0; y < PB_TILE; y += 4) {
        const int c = sm.c0 + y;
        if (c >= w) break;
        const size_t dst = (size_t)(sm.fh ? w - 1 - c : c) * w + j;
        const uint32_t v = ta[pb_lds_byte(x, y)];
        const float va = pb_unit(v);
        sm.oa[dst] = va;
        if (cov) sm.ob[dst] = sm.same ? va : pb_unit(tb[pb_lds_byte(x, y)]);
        pb_side_store1(sd, dst, v, r, c);
    }
}

}  // namespace

extern "C" int wsu_pair_batch_planes_f32(const uint8_t* planes, int files, int h, int w, const int32_t* idx_in, const int32_t* idx_cov,
                                         const uint8_t* op, int n, int allow_transpose, int side, float* inputs, float* covers, void* stream) {
    WSU_REQUIRE(planes && idx_in && op && inputs, "pair_batch_planes_f32: null pointer");
    WSU_REQUIRE((idx_cov == nullptr) == (covers == nullptr), "pair_batch_planes_f32: idx_cov and covers are given or NULL together");
    WSU_REQUIRE(side >= 0 && side <= 3, "pair_batch_planes_f32: side=%d outside 0..3 (bit 0: parity plane, bit 1: demosaic planes)", side);
    WSU_REQUIRE(files >= 1 && h >= 1 && w >= 1 && n >= 0, "pair_batch_planes_f32: bad shape files=%d h=%d w=%d n=%d", files, h, w, n);
    WSU_REQUIRE(!allow_transpose || h == w, "pair_batch_planes_f32: transposing ops need square planes (h=%d w=%d)", h, w);
    if (n == 0) return WSU_OK;
    const int tiles_x = (w + PB_TILE - 1) / PB_TILE, tiles_y = (h + PB_TILE - 1) / PB_TILE;
    const long long blocks = (long long)tiles_x * tiles_y * n;
    WSU_REQUIRE(blocks <= 0x7FFFFFFFll, "pair_batch_planes_f32: %lld tiles exceed one launch", blocks);
    const int max_op = allow_transpose ? 7 : 3;
    // (W % 4 == 0 keeps every plane of a sample 16-byte aligned behind an aligned base)
    const bool vec = w % 4 == 0 && (h % 4 == 0 || !allow_transpose) && reinterpret_cast<uintptr_t>(planes) % 4 == 0 &&
                     reinterpret_cast<uintptr_t>(inputs) % 16 == 0 && reinterpret_cast<uintptr_t>(covers) % 16 == 0;
    hipLaunchKernelGGL(vec ? pair_planes_vec_kernel : pair_planes_any_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), planes, files, h, w, idx_in, idx_cov, op, max_op, tiles_x, tiles_x * tiles_y, side,
                       inputs, covers);
    return wsu_check_launch("pair_planes_kernel");
}

extern "C" int wsu_pair_batch_f32(const uint8_t* planes, int files, int h, int w, const int32_t* idx_in, const int32_t* idx_cov,
                                  const uint8_t* op, int n, int allow_transpose, float* inputs, float* covers, void* stream) {
    WSU_REQUIRE(planes && idx_in && idx_cov && op && inputs && covers, "pair_batch_f32: null pointer");
    WSU_REQUIRE(files >= 1 && h >= 1 && w >= 1 && n >= 0, "pair_batch_f32: bad shape files=%d h=%d w=%d n=%d", files, h, w, n);
    WSU_REQUIRE(!allow_transpose || h == w, "pair_batch_f32: transposing ops need square planes (h=%d w=%d)", h, w);
    if (n == 0) return WSU_OK;
    const int tiles_x = (w + PB_TILE - 1) / PB_TILE, tiles_y = (h + PB_TILE - 1) / PB_TILE;
    const long long blocks = (long long)tiles_x * tiles_y * n;
    WSU_REQUIRE(blocks <= 0x7FFFFFFFll, "pair_batch_f32: %lld tiles exceed one launch", blocks);
    const int max_op = allow_transpose ? 7 : 3;
    const bool vec = w % 4 == 0 && (h % 4 == 0 || !allow_transpose) && reinterpret_cast<uintptr_t>(planes) % 4 == 0 &&
                     reinterpret_cast<uintptr_t>(inputs) % 16 == 0 && reinterpret_cast<uintptr_t>(covers) % 16 == 0;
    hipLaunchKernelGGL(vec ? pair_batch_vec_kernel : pair_batch_any_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), planes, files, h, w, idx_in, idx_cov, op, max_op, tiles_x, tiles_x * tiles_y,
                       inputs, covers);
    return wsu_check_launch("pair_batch_kernel");
}
