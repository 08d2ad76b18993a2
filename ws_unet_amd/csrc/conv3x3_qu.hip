// K1u (round 4): the first conv of a decoder block TOGETHER with the transposed conv in front of it -- xd = relu(conv3x3(cat[convT2x2(x_low), skip]))
// (src/unet/model/unet.py:171-173, 177-179, 183-185) in ONE launch, in the arithmetic of the default inference mode 'f16f4p' (conv3x3_q.hip).
// There is no non-linearity between nn.ConvTranspose2d(k2, s2) and the 3x3 conv, so their composition is linear in x_low:
//   * an output pixel (2i + py, 2j + px) of PARITY CLASS (py, px) sees, through its 3x3 window on the upsampled tensor, exactly 2 x 2 pixels of
//     x_low -- rows i - 1 + py + dy, columns j - 1 + px + dx (dy, dx in {0, 1}) -- and the weights of that 2x2-tap conv are the products
//     Wc[py,px][dy,dx][co][c] = sum_{ci} sum_{(ky,kx) -> (dy,dx)} w3[co][ci][ky][kx] * wT[c][ci][sy][sx]  (pack kernel below, fp32);
//   * the reflect padding of the 3x3 conv at the high resolution is CLAMP padding of x_low (xu[-1] = xu[1] = the sub-position 1 of low row 0);
//   * the transposed conv's bias passes through all nine taps everywhere (reflect padding has no missing tap): one combined bias per co.
// So the upsampled half costs 4 taps x C_low = 512 multiply-adds per output and channel pair instead of 9 x C_low/2 = 576, the transposed conv
// (its launch, its 2.56 B/element output written and read back) disappears, and `xu` never exists.  The skip half is the ordinary 3x3 conv.
//
// Structure: the persistent workgroup of conv3x3_q.hip (one per CU, 16 x 32-pixel x 64-co tiles, 4 pure-DMA loader waves + 8 matrix waves, one
// s_barrier per step), with two differences forced by the parity classes:
//   * a matrix wave owns ONE class: wave = (class, half of the tile's 8 low rows), its two 32-pixel matrix tiles are 2 low rows x 16 low columns
//     of that class (so all 32 pixels of a matrix instruction share the combined weights).  The skip half's halo tile is therefore staged as four
//     class planes of 9 x 17 pixels -- the loaders' DMA gathers every other pixel of a row (per-lane source address, contiguous LDS
//     destination) -- and lanes 16-31 of a matrix tile hold their row's columns rotated by one, which makes the 16-byte fragment reads of two
//     rows 272 B (528 B in the low tile) apart conflict free (lane groups of ds_read_b128, MI355X guide, LDS);
//   * steps differ in kind: a skip chunk (9 taps, 28 KB of weights, 31 KB of input) or a whole low chunk (4 taps x 4 classes: two 25 KB weight
//     slices, dy = 0 and dy = 1, and a 17 KB input tile), one s_barrier each.  LDS holds two 78.75 KB step regions; step j of a workgroup
//     lives in region j & 1, so the loaders fetch step j + 1 while the matrix waves work on step j and wait for all of it (`s_waitcnt
//     vmcnt(0)`) before the barrier that opens it.  (Until round 5 a low chunk was two half-steps L0 / L1 in a ring of five 31.5 KB slots:
//     a barrier, a slice wait and an exposed first fragment read per 3 matrix units.)
// The step head (sync_step) forms the lane bases of a step's fragment reads in front of its barrier, as in conv3x3_q.hip.  A skip step's five
// fp4 units share one set of weight bases (the lane half's tap folded in, immediates per unit); on the pixel side the class planes leave no
// compile-time tap offsets (they depend on the wave's class), but which of a pair's two taps a lane reads is a constant of the lane, kept as five
// registers for the launch (tap_sel): one add and one shift-add per unit.  The ninth tap's lanes 32-63 read their zero operands from a zero block
// in the unused tail of the second step region.  A skip step issues 26-28 vector instructions beside its 56 matrix instructions (70-78 until
// profiles/r25); the low step is as it was.
// A skip step's 14 units run as the fragment pipeline of conv3x3_q.hip (reads of unit u + 1 before the matrix instructions of unit u, two
// fragment sets).  The low steps keep the compiler's order: in the stamps on record (profiles/r06/stamps_merged_step.log) a skip step's
// loaders are early (barrier wait 1823-1902 cycles, vmcnt wait 680-743) while its matrix waves lose 1256-1433 cycles at the barrier among
// themselves, whereas in a low step the loaders are the late ones (vmcnt wait 983-1071, loader barrier wait 176-285): a low step ends when
// its DMA lands, not when the fragments do.
// Accuracy: Wc is formed in fp32 and then split like any weight (f16 + fp4 residual terms); `xu` is never rounded to storage -- the fused
// result is closer to the exact composition than the two-kernel path.  Replaces ops.convt2x2_pl + ops.conv3x3_q in UNet._forward_planar.
// Format H (mode 'f16p', template argument FMT = WSU_PLANAR_H): planar H tensors in and out, the f16 products alone (no fp4 instruction, no Q /
// scale pieces), Wc rounded to f16 once; the same two step regions, each step's allocations smaller (skip input 19.1 KB, weights 18 KB; low
// input 10.3 KB, a dy slice of a low chunk's weights 16 KB).
#include "wsu_device.h"

namespace {

constexpr int TW = 32, TH = 16;
// skip half: the 18 x 34 halo tile as class planes [row parity][column parity][9][17]
constexpr int CW = 17, CH = 9, CPIX = CW * CH;            // 153
constexpr int NPIX_S = 4 * CPIX;                          // 612
constexpr int PLANE_S = NPIX_S * 16;                      // 9792
constexpr int SEG_S = (NPIX_S + 63) / 64;                 // 10
constexpr int IN_S = 3 * PLANE_S + SEG_S * 256;           // 31936: f16 ch 0-7 | f16 ch 8-15 | Q | one dword slot per pixel for the scale byte
// low half: (8 + 2) x (16 + 2) low-resolution pixels at a row pitch of 33 (528 B = 16 mod 256, like the class planes' 272 B)
constexpr int LP = 33, LH = TH / 2 + 2, LW_ = TW / 2 + 2;
constexpr int NPIX_L = LP * LH;                           // 330
constexpr int PLANE_L = NPIX_L * 16;                      // 5280
constexpr int SEG_L = (NPIX_L + 63) / 64;                 // 6
constexpr int IN_L = 3 * PLANE_L + SEG_L * 256;           // 17376
constexpr int W_GRAN_S = 9 * 3 * WSU_COB * 16;            // 27648
constexpr int W_S = W_GRAN_S + 1024;                      // the (block, chunk) slice of wsu_conv3x3_pack_f4
constexpr int W_UNITS_L = 8;                              // (class, dx) units of half a low chunk
constexpr int W_GRAN_L = W_UNITS_L * 3 * WSU_COB * 16;    // 24576
constexpr int W_L = W_GRAN_L + 1024;                      // + [8][64] scale bytes, padded to a DMA piece
constexpr int PIECES_S = W_S / 1024, PIECES_L = W_L / 1024;   // 28, 25
// a step's region: S = input [0, IN_S) + weights [IN_S, IN_S + W_S);  L = weights dy 0 [0, W_L) + input [W_L, W_L + IN_L) + weights dy 1 after it
constexpr int REGION = 80640;
constexpr int OFF_SW = IN_S, OFF_LIN = W_L, OFF_LW1 = W_L + IN_L;
constexpr int LDS_BIAS = 2 * REGION;                      // 161280
constexpr int MAX_COUT = 512;
constexpr int LDS_TOTAL = LDS_BIAS + MAX_COUT * 4;        // 163328
static_assert(IN_S + W_S <= REGION && OFF_LW1 + W_L <= REGION && (REGION & 0xF) == 0 && LDS_TOTAL <= 160 * 1024, "LDS budget");
static_assert((OFF_SW | OFF_LIN | OFF_LW1) % 16 == 0, "16-byte aligned allocations");
// format Q: a block of zeros -- what lanes 32-63 of the ninth tap's fp4 unit read in a skip step (sync_step): weights + m * 512, Q granules
// + q * 544, 16 bytes each.  It lies in the tail of the second step region, which no allocation of a step reaches (the bias area behind the
// regions fills LDS to 512 bytes)
constexpr int ZERO_BYTES = 576;
constexpr int LDS_ZERO = 2 * REGION - ZERO_BYTES;
static_assert(IN_S + W_S <= REGION - ZERO_BYTES && OFF_LW1 + W_L <= REGION - ZERO_BYTES && LDS_ZERO % 16 == 0 && ZERO_BYTES >= 2 * CW * 16 + 16 + 16, "zero block");
constexpr int NLOAD = 4, NWAVE = 8, NT = (NWAVE + NLOAD) * 64;
constexpr unsigned OOB = 0xFFFFFFF0u;
// format H: weight slices without the fp4 plane and the scale bytes
constexpr int W_S_H = 9 * 2 * WSU_COB * 16;               // 18432: the (block, chunk) slice of wsu_conv3x3_pack_h
constexpr int W_L_H = W_UNITS_L * 2 * WSU_COB * 16;       // 16384: [class 4][dx 2][plane 2][64 co][16 B]
constexpr int PIECES_S_H = W_S_H / 1024, PIECES_L_H = W_L_H / 1024;   // 18, 16

struct UArgs {
    const char* xl; const char* xs; const char* wps; const char* wpl; const float* bias;
    char* y;
    int n, h, w, hl, wl, cl, c2, cout;
    int tiles_x, tiles_y, ltiles_x, ncb, nchS, nchL;
    int relu, ntiles;
    unsigned* range_flag;
};

struct Tile { int n, y0, x0, cb; };
__device__ __forceinline__ Tile tile_of(const UArgs& a, int t) {
    Tile r;
    r.cb = t % a.ncb; t /= a.ncb;
    const int tx = t % a.tiles_x; t /= a.tiles_x;
    const int ty = t % a.tiles_y;
    r.n = t / a.tiles_y; r.y0 = ty * TH; r.x0 = tx * TW;
    return r;
}

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) char lds_char;

// `s_waitcnt vmcnt(n)` for a run-time n (the counter is 6 bits wide)
__device__ __forceinline__ void wait_vm(int n) {
#define WSU_VM_CASE(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    switch (n) {
        WSU_VM_CASE(0) WSU_VM_CASE(1) WSU_VM_CASE(2) WSU_VM_CASE(3) WSU_VM_CASE(4) WSU_VM_CASE(5) WSU_VM_CASE(6) WSU_VM_CASE(7) WSU_VM_CASE(8) WSU_VM_CASE(9)
        WSU_VM_CASE(10) WSU_VM_CASE(11) WSU_VM_CASE(12) WSU_VM_CASE(13) WSU_VM_CASE(14) WSU_VM_CASE(15) WSU_VM_CASE(16) WSU_VM_CASE(17) WSU_VM_CASE(18) WSU_VM_CASE(19)
        WSU_VM_CASE(20) WSU_VM_CASE(21) WSU_VM_CASE(22) WSU_VM_CASE(23) WSU_VM_CASE(24) WSU_VM_CASE(25) WSU_VM_CASE(26) WSU_VM_CASE(27) WSU_VM_CASE(28) WSU_VM_CASE(29)
        WSU_VM_CASE(30) WSU_VM_CASE(31) WSU_VM_CASE(32) WSU_VM_CASE(33) WSU_VM_CASE(34) WSU_VM_CASE(35) WSU_VM_CASE(36) WSU_VM_CASE(37) WSU_VM_CASE(38) WSU_VM_CASE(39)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;       // (never: a step of a wave is at most 24 instructions)
    }
#undef WSU_VM_CASE
}

// Steps of a tile: nchS skip chunks (kind S), then one step per low chunk (kind L).  Everything of a step dies with the step, so the region
// step j - 1 leaves at barrier j takes step j + 1.

// ================= loader wave LW: pure DMA, walks the allocation sequence ahead of the matrix waves ==========================================
// Format H: two input pieces per segment; skip weights 3 / 3 / 6 / 6 pieces, low weights 3 / 3 / 5 / 5 per dy slice (the low input: 4 / 4 / 2 / 2).
template <int FMT, int LW>
__device__ __forceinline__ void u_loader(const UArgs& a, char* smem, int lane, int lw, int G, int K) {
    constexpr bool H = FMT == WSU_PLANAR_H;
    constexpr int NSS = LW < 2 ? 3 : 2;                   // skip-input segments LW, LW + 4, LW + 8 (< 10)
    constexpr int NSL = LW < 2 ? 2 : 1;                   // low-input segments LW, LW + 4 (< 6)
    constexpr int OPS_INS = (H ? 2 : 4) * NSS, OPS_INL = (H ? 2 : 4) * NSL;
    constexpr int WS0 = H ? (LW < 2 ? LW * 3 : 6 + (LW - 2) * 6) : (LW < 2 ? LW * 5 : 10 + (LW - 2) * 9);
    constexpr int NWS = H ? (LW < 2 ? 3 : 6) : (LW < 2 ? 5 : 9);
    constexpr int WL0 = H ? (LW < 2 ? LW * 3 : 6 + (LW - 2) * 5) : (LW < 2 ? LW * 5 : (LW == 2 ? 10 : 17));
    constexpr int NWL = H ? (LW < 2 ? 3 : 5) : (LW < 2 ? 5 : (LW == 2 ? 7 : 8));
    constexpr int WSLICE_S = H ? W_S_H : W_S, WSLICE_L = H ? W_L_H : W_L;
    static_assert(2 * 5 + 2 * 9 == PIECES_S && 2 * 5 + 7 + 8 == PIECES_L, "weight pieces over the loader waves");
    static_assert(2 * 3 + 2 * 6 == PIECES_S_H && 2 * 3 + 2 * 5 == PIECES_L_H, "weight pieces over the loader waves (format H)");
    lds_char* smem3 = (lds_char*)smem;
    const unsigned hw16 = (unsigned)(a.h * a.w) * 16u, hwl16 = (unsigned)(a.hl * a.wl) * 16u;
    const unsigned cbytes_s = H ? (unsigned)wsu_h_chunk_bytes(a.h, a.w) : (unsigned)wsu_q_chunk_bytes(a.h, a.w);
    const unsigned cbytes_l = H ? (unsigned)wsu_h_chunk_bytes(a.hl, a.wl) : (unsigned)wsu_q_chunk_bytes(a.hl, a.wl);
    const int T = a.nchS + a.nchL;
    const int J = K * T;
    if (J <= 0) return;
    unsigned voS[NSS], soS[NSS], voL[NSL], soL[NSL];
    auto plan = [&](const Tile& t) __attribute__((always_inline)) {
        WSU_STATIC_FOR(NSS, k, {
            const int idx = min((LW + NLOAD * k) * 64 + lane, NPIX_S - 1);
            const int p = idx / CPIX, rem = idx - p * CPIX;
            const int lr = rem / CW, lc = rem - lr * CW;
            const int yy = wsu_reflect(t.y0 - 1 + 2 * lr + (p >> 1), a.h), xx = wsu_reflect(t.x0 - 1 + 2 * lc + (p & 1), a.w);
            voS[k] = (unsigned)(yy * a.w + xx) * 16u;
            if constexpr (!H) soS[k] = 3u * hw16 + wsu_q_soff(yy, xx, a.tiles_x);
        });
        WSU_STATIC_FOR(NSL, k, {
            const int idx = min((LW + NLOAD * k) * 64 + lane, NPIX_L - 1);
            const int r = idx / LP, c = min(idx - r * LP, LW_ - 1);                 // (columns 18..32 of a row are padding: any valid pixel)
            const int yy = min(max((t.y0 >> 1) - 1 + r, 0), a.hl - 1), xx = min(max((t.x0 >> 1) - 1 + c, 0), a.wl - 1);
            voL[k] = (unsigned)(yy * a.wl + xx) * 16u;
            if constexpr (!H) soL[k] = 3u * hwl16 + wsu_q_soff(yy, xx, a.ltiles_x);
        });
    };
    // ---- the step cursor: tile a_kt, chunk a_c of kind a_low; the allocation a_r of the step being issued (S: 0 input, 1 weights;
    // L: 0 weights dy 0, 1 input, 2 weights dy 1)
    int a_kt = 0, a_c = 0, a_r = 0; bool a_low = false;
    Tile at = tile_of(a, lw);
    unsigned region = 0;                                                  // byte offset of the next step's region
    auto issue_alloc = [&](lds_char* slot) __attribute__((always_inline)) {
        int nops;
        const bool is_in = a_low ? a_r == 1 : a_r == 0;
        if (is_in && !a_low) {
            const char* src = a.xs + ((size_t)at.n * a.nchS + a_c) * cbytes_s;
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(src), 0, (int)cbytes_s, 0x00020000);
            WSU_STATIC_FOR(NSS, k, {
                constexpr int seg = LW + NLOAD * k;
                if (seg < SEG_S - 1 || lane < NPIX_S - (SEG_S - 1) * 64) {
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + seg * 1024), 16, voS[k], 0, 0, 0);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + PLANE_S + seg * 1024), 16, voS[k], (int)hw16, 0, 0);
                    if constexpr (!H) {
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + 2 * PLANE_S + seg * 1024), 16, voS[k], (int)(2u * hw16), 0, 0);
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + 3 * PLANE_S + seg * 256), 1, soS[k], 0, 0, 0);
                    }
                }
            });
            nops = OPS_INS;
        } else if (is_in) {
            const char* src = a.xl + ((size_t)at.n * a.nchL + a_c) * cbytes_l;
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(src), 0, (int)cbytes_l, 0x00020000);
            WSU_STATIC_FOR(NSL, k, {
                constexpr int seg = LW + NLOAD * k;
                if (seg < SEG_L - 1 || lane < NPIX_L - (SEG_L - 1) * 64) {
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + seg * 1024), 16, voL[k], 0, 0, 0);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + PLANE_L + seg * 1024), 16, voL[k], (int)hwl16, 0, 0);
                    if constexpr (!H) {
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + 2 * PLANE_L + seg * 1024), 16, voL[k], (int)(2u * hwl16), 0, 0);
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + 3 * PLANE_L + seg * 256), 1, soL[k], 0, 0, 0);
                    }
                }
            });
            nops = OPS_INL;
        } else if (!a_low) {
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.wps), 0, 0x7FFFFFF0, 0x00020000);
            const int base = (at.cb * a.nchS + a_c) * WSLICE_S;
            WSU_STATIC_FOR(NWS, k, {
                constexpr int piece = WS0 + k;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + piece * 1024), 16, (unsigned)lane * 16u, base + piece * 1024, 0, 0);
            });
            nops = NWS;
        } else {
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.wpl), 0, 0x7FFFFFF0, 0x00020000);
            const int base = ((at.cb * a.nchL + a_c) * 2 + (a_r == 2 ? 1 : 0)) * WSLICE_L;
            WSU_STATIC_FOR(NWL, k, {
                constexpr int piece = WL0 + k;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(slot + piece * 1024), 16, (unsigned)lane * 16u, base + piece * 1024, 0, 0);
            });
            nops = NWL;
        }
        return nops;
    };
    auto issue_step = [&]() __attribute__((always_inline)) {             // the DMA of the next step into its region; its instruction count
        lds_char* base = smem3 + region;
        int nops;
        if (!a_low) {
            a_r = 0; nops = issue_alloc(base);
            a_r = 1; nops += issue_alloc(base + OFF_SW);
            if (++a_c == a.nchS) { a_c = 0; a_low = true; }
        } else {
            a_r = 0; nops = issue_alloc(base);
            a_r = 1; nops += issue_alloc(base + OFF_LIN);
            a_r = 2; nops += issue_alloc(base + OFF_LW1);
            if (++a_c == a.nchL) {                                        // (nchL == 0 never happens: the entry point requires a low half)
                a_low = false; a_c = 0;
                if (++a_kt < K) { at = tile_of(a, lw + a_kt * G); plan(at); }
            }
        }
        region ^= (unsigned)REGION;
        return nops;
    };
    plan(at);
    {
        issue_step();                                                     // steps 0 and 1: both regions are free
        const int n1 = J > 1 ? issue_step() : 0;
        wait_vm(n1);
    }
    for (int j = 0; ; ++j) {
        __builtin_amdgcn_s_barrier();                                     // barrier j: step j is complete in LDS; every matrix wave has left step j - 1
        asm volatile("" ::: "memory");
        if (j + 1 >= J) break;
        if (j >= 1) issue_step();                                         // step j + 1 into the region step j - 1 has left
        wait_vm(0);                                                       // step j + 1 has landed
    }
}

// FMT: storage format of x_low, x_skip and y -- WSU_PLANAR_Q (mode 'f16f4p') or WSU_PLANAR_H (mode 'f16p': the f16 products alone)
template <int FMT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(3, 3)))
void conv3x3_qu_kernel(const UArgs a) {
    constexpr bool H = FMT == WSU_PLANAR_H;
    constexpr int WPL = H ? 2 : 3;                                          // weight granule planes per tap / unit
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int G = gridDim.x;
    const int lw = (int)wsu_xcd_remap(blockIdx.x, G);
    const int K = a.ntiles > lw ? (a.ntiles - lw + G - 1) / G : 0;          // tiles walked by this workgroup
    float* s_bias = reinterpret_cast<float*>(smem + LDS_BIAS);
    for (int i = tid; i < a.cout; i += NT) s_bias[i] = a.bias ? a.bias[i] : 0.f;
    if constexpr (!H) {
        // the zero block: cleared once, nothing writes it afterwards.  Step 0 reads it right behind its barrier, so the stores are waited for here
        for (int i = tid; i < ZERO_BYTES / 4; i += NT) reinterpret_cast<unsigned*>(smem + LDS_ZERO)[i] = 0u;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    if (wv >= NWAVE) {
        switch (wv - NWAVE) {
            case 0: u_loader<FMT, 0>(a, smem, lane, lw, G, K); break;
            case 1: u_loader<FMT, 1>(a, smem, lane, lw, G, K); break;
            case 2: u_loader<FMT, 2>(a, smem, lane, lw, G, K); break;
            default: u_loader<FMT, 3>(a, smem, lane, lw, G, K); break;
        }
        return;
    }

    // ================= matrix waves ===================================================================================================
    const int cls = wv & 3, py = cls >> 1, px = cls & 1, rh = wv >> 2;      // wave-uniform
    const int l31 = lane & 31, hh = lane >> 5;
    const int lrow = l31 >> 4, lcol = lrow ? ((l31 + 15) & 15) : l31;       // lanes 16-31: the next low row, columns rotated by one (bank-conflict-free fragment reads)
    const unsigned laneS = (unsigned)(((4 * rh + lrow) * CW + lcol) * 16), laneL = (unsigned)(((4 * rh + lrow) * LP + lcol) * 16);
    constexpr unsigned QS = 2 * CW * 16, QL = 2 * LP * 16;                   // second matrix tile: two low rows further
    Tile cur = tile_of(a, lw);
    f32x16 acc[2][2];                                                       // [32-channel half][matrix tile]
    unsigned region = 0;                                                     // byte offset of the next step's region
    unsigned in_off = 0, w_off = 0;
    auto next_region = [&]() __attribute__((always_inline)) { const unsigned r = region; region ^= (unsigned)REGION; return r; };
    int hh_q = hh;
    typedef __attribute__((address_space(3))) const unsigned char lds_cuchar;
    typedef __attribute__((address_space(3))) const int lds_cint;
    typedef __attribute__((address_space(3))) const u32x4 lds_cu32x4;
    lds_char* L = (lds_char*)smem;
    const unsigned Lb = (unsigned)(size_t)L;                                 // the pinned bases are absolute LDS addresses (at())
    auto at = [](unsigned addr) __attribute__((always_inline)) { return (lds_char*)(size_t)addr; };
    // byte offset of tap (ky, kx)'s source pixel relative to the lane's own class pixel, in the class planes of the skip tile
    auto tap_s = [&](int ky, int kx) __attribute__((always_inline)) {
        return (unsigned)(((((py + ky) & 1) * 2 + ((px + kx) & 1)) * CPIX + ((py + ky) >> 1) * CW + ((px + kx) >> 1)) * 16);
    };
    // lane bases of a step's fragment reads, formed BEFORE the step's barrier (sync_step): a_off / b_off of the f16 products (weights: + the
    // unit's planes and the 32-channel half; input: + the tap's pixel offset and the matrix tile), hd_* of the fp4 unit that opens the step.
    // A skip step's five fp4 units (tap pair tp: lanes 0-31 tap 2 tp, lanes 32-63 tap 2 tp + 1) share ONE set of weight bases, as in
    // conv3x3_q.hip: x_w = plane 2 of tap hh (+ ((6 tp + 2) * 64 + m * 32) * 16), x_sa = scale byte of tap hh (+ 128 tp + 32 m).  The ninth
    // tap (pair 4) has no partner: lanes 32-63 multiply zeros, which they READ -- x_w4 / x_b4 are the tap's own weight / Q-granule bases in
    // lanes 0-31 and point lanes 32-63 at the zero block; both scale bytes keep real addresses, those of tap 8 itself (x_sa4, tap8_s).
    unsigned a_off = 0, b_off = 0, hd_w = 0, hd_sa = 0, hd_b = 0, hd_sb = 0, x_w = 0, x_w4 = 0, x_sa = 0, x_sa4 = 0, x_b4 = 0;
    constexpr unsigned W4_IMM = (unsigned)((8 * 3 + 2) * 64) * 16u;           // tap 8: weight plane 2
    // The pixel side has no compile-time tap offsets here (the class planes: tap_s depends on the wave's class), but the lane half's choice
    // between a pair's two taps is a constant of the lane: tap_sel[tp] = (its tap's offset + the lane's pixel) / 4, formed once per launch --
    // the scale slot's offset as it stands, the Q granule's times 4 (one add, one shift-add per unit)
    unsigned tap_sel[5] = {};
    if constexpr (!H) {
        WSU_STATIC_FOR(5, tp, {
            constexpr int t0 = 2 * tp, t1 = (2 * tp + 1 < 9) ? 2 * tp + 1 : 2 * tp;
            tap_sel[tp] = ((hh ? tap_s(t1 / 3, t1 % 3) : tap_s(t0 / 3, t0 % 3)) + laneS) >> 2;
            asm volatile("" : "+v"(tap_sel[tp]));
        });
    }
    // a step of kind S (LOW = false) or L: takes the next region and forms everything the step's first reads need -- it depends on the step
    // count, the wave and the lane only -- in front of the barrier, where a wave waits for the others anyway.  The empty asm statements pin the
    // values there (they and the barrier keep their order) and make them opaque per step, like hh_q: nothing is hoisted out of the tile loop.
    // Behind the barrier the step opens with its LDS reads.
    auto sync_step = [&](auto low_c) __attribute__((always_inline)) {
        constexpr bool LOW = decltype(low_c)::value;
        const unsigned r = next_region();
        in_off = LOW ? r + OFF_LIN : r;
        w_off = LOW ? r : r + OFF_SW;
        hh_q = hh;
        asm volatile("" : "+v"(hh_q));
        a_off = Lb + w_off + (unsigned)l31 * 16u + (unsigned)hh * 1024u;
        b_off = Lb + in_off + (unsigned)hh * (LOW ? PLANE_L : PLANE_S) + (LOW ? laneL : laneS);
        if constexpr (!H && !LOW) {
            // S: every fragment base of the step's fp4 units (the Q granules and scale slots of pairs 1-3 are tap_sel + a wave-uniform base)
            const unsigned hq = (unsigned)hh_q, zero = Lb + (unsigned)LDS_ZERO;
            const unsigned w0 = Lb + w_off + (unsigned)l31 * 16u;
            x_w = w0 + hq * (unsigned)(3 * 64 * 16);
            x_w4 = hq ? zero - W4_IMM : w0;
            x_sa4 = Lb + w_off + W_GRAN_S + (unsigned)l31;
            x_sa = x_sa4 + hq * 64u;
            hd_b = Lb + in_off + 2 * PLANE_S + tap_sel[0] * 4u;
            hd_sb = Lb + in_off + 3 * PLANE_S + tap_sel[0];
            x_b4 = hq ? zero : Lb + in_off + 2 * PLANE_S + tap_sel[4] * 4u;
            asm volatile("" : "+v"(a_off), "+v"(b_off), "+v"(x_w), "+v"(x_w4), "+v"(x_sa), "+v"(x_sa4), "+v"(hd_b), "+v"(hd_sb), "+v"(x_b4));
        } else if constexpr (!H) {
            // L: dy = 0, unit cls * 2 + dx with dx = the lane half
            const int u = cls * 2 + hh_q;
            const unsigned pb = (unsigned)((py * LP + px) * 16) + (unsigned)hh_q * 16u + laneL;
            hd_w = Lb + w_off + (unsigned)((u * 3 + 2) * 64 + l31) * 16u;
            hd_sa = Lb + w_off + W_GRAN_L + (unsigned)(u * 64 + l31);
            hd_b = Lb + in_off + 2 * PLANE_L + pb;
            hd_sb = Lb + in_off + 3 * PLANE_L + (pb >> 2);
            asm volatile("" : "+v"(a_off), "+v"(b_off), "+v"(hd_w), "+v"(hd_sa), "+v"(hd_b), "+v"(hd_sb));
        } else {
            asm volatile("" : "+v"(a_off), "+v"(b_off));
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    // ---- a skip chunk: the nine taps of the ordinary conv, operands of conv3x3_q.hip (f16 products per tap, both cross terms of a tap pair as one fp4 instruction)
    // FIRST: the step opens a tile -- the matrix instructions of its first unit take the literal zero for C and define the accumulators.
    // Format Q: the step is the software pipeline of conv3x3_q.hip (units_pipelined) -- 14 units in the accumulation order u = 3 tp + k (k = 0 the
    // fp4 unit of tap pair tp, k = 1 / 2 the f16 products of taps 2 tp / 2 tp + 1), the fragment reads of unit u + 1 issued before the matrix
    // instructions of unit u into the other of two fragment sets, one scheduling region per unit.  Left to the compiler a unit's reads stood
    // right in front of the wait and the matrix instructions that use them, in both waves of a SIMD at once.
    struct Frag { u32x4 a[2]; u32x4 b[2]; int sa[2]; int sb[2]; };
    auto load_unit = [&](auto u_c, Frag& f) __attribute__((always_inline)) {
        constexpr int u = decltype(u_c)::value, tp = u / 3, k = u % 3;
        if constexpr (k == 0) {
            constexpr bool single = 2 * tp + 1 >= 9;                      // the ninth tap
            constexpr unsigned wimm = (unsigned)((6 * tp + 2) * 64) * 16u;
            static_assert(!single || wimm == W4_IMM, "tap 8");
            const unsigned wb = single ? x_w4 : x_w, sab = single ? x_sa4 : x_sa;
            const unsigned bb = tp == 0 ? hd_b : (single ? x_b4 : Lb + in_off + 2 * PLANE_S + tap_sel[tp] * 4u);
            const unsigned sbb = tp == 0 ? hd_sb : Lb + in_off + 3 * PLANE_S + tap_sel[tp];
_Pragma("unroll")
            for (int m = 0; m < 2; ++m) { f.a[m] = *(lds_cu32x4*)(at(wb) + wimm + m * 512); f.sa[m] = *(lds_cuchar*)(at(sab) + 128 * tp + m * 32); }
_Pragma("unroll")
            for (int q = 0; q < 2; ++q) {
                f.b[q] = *(lds_cu32x4*)(at(bb) + q * QS);
                f.sb[q] = *(lds_cint*)(at(sbb) + q * (QS >> 2));
            }
        } else {
            constexpr int tap = 2 * tp + k - 1;
            const unsigned pb = b_off + tap_s(tap / 3, tap % 3);
_Pragma("unroll")
            for (int m = 0; m < 2; ++m) f.a[m] = *(lds_cu32x4*)(at(a_off) + ((tap * WPL) * 64) * 16 + m * 512);
_Pragma("unroll")
            for (int q = 0; q < 2; ++q) f.b[q] = *(lds_cu32x4*)(at(pb) + q * QS);
        }
    };
    auto mma_unit = [&](auto u_c, Frag& f, auto first_c) __attribute__((always_inline)) {
        constexpr int u = decltype(u_c)::value, k = u % 3;
        constexpr bool FIRST = decltype(first_c)::value && u == 0;
_Pragma("unroll")
        for (int m = 0; m < 2; ++m)
_Pragma("unroll")
            for (int q = 0; q < 2; ++q) {
                if constexpr (k != 0) wsu_mfma_f16(f.a[m], f.b[q], acc[m][q]);
                else if constexpr (FIRST) acc[m][q] = wsu_mfma_q4_z(f.a[m], f.b[q], f.sa[m], f.sb[q]);
                else wsu_mfma_q4(f.a[m], f.b[q], f.sa[m], f.sb[q], acc[m][q]);
            }
    };
    auto skip_units = [&](auto first_c) __attribute__((always_inline)) {
        constexpr bool FIRST = decltype(first_c)::value;
        if constexpr (!H) {
            constexpr int NU = 14;                                        // one unit of reads in flight, two fragment sets
            Frag fr[2];
            load_unit(std::integral_constant<int, 0>{}, fr[0]);
            WSU_STATIC_FOR(NU, u, {
                if constexpr (u + 1 < NU) load_unit(std::integral_constant<int, u + 1>{}, fr[(u + 1) % 2]);
                __builtin_amdgcn_sched_barrier(0);                        // (the reads FIRST: left to itself the scheduler sinks them behind the unit's matrix instructions)
                mma_unit(u_c, fr[u % 2], first_c);
                __builtin_amdgcn_sched_barrier(0);
            });
        } else {
            WSU_STATIC_FOR(9, tap, {
                u32x4 ah[2], bh[2];
                const unsigned pb = b_off + tap_s(tap / 3, tap % 3);
_Pragma("unroll")
                for (int m = 0; m < 2; ++m) ah[m] = *(lds_cu32x4*)(at(a_off) + ((tap * WPL) * 64) * 16 + m * 512);
_Pragma("unroll")
                for (int q = 0; q < 2; ++q) bh[q] = *(lds_cu32x4*)(at(pb) + q * QS);
_Pragma("unroll")
                for (int m = 0; m < 2; ++m)
_Pragma("unroll")
                    for (int q = 0; q < 2; ++q) {
                        if constexpr (FIRST && tap == 0) acc[m][q] = wsu_mfma_f16_z(ah[m], bh[q]);
                        else wsu_mfma_f16(ah[m], bh[q], acc[m][q]);
                    }
            });
        }
    };
    // ---- a dy slice of a low chunk: taps (dy, 0) and (dy, 1) of this wave's class -- units cls * 2 + dx of the slice [8][3 planes][64 co][16 B] + [8][64] scale bytes
    auto low_units = [&](auto dy_c) __attribute__((always_inline)) {
        constexpr int dy = decltype(dy_c)::value;
        constexpr unsigned WDY = dy ? (unsigned)(OFF_LW1) : 0u;               // the dy = 1 slice of the step's weights, relative to the dy = 0 slice
        const unsigned rowo = (unsigned)(((py + dy) * LP + px) * 16);
        if constexpr (!H) {
            const int u = cls * 2 + hh_q;                                   // lanes 32-63: dx = 1
            u32x4 a4[2], b4[2]; int sa[2], sb[2];
            const unsigned pb = rowo + (unsigned)hh_q * 16u + laneL;
            const unsigned wb = dy == 0 ? hd_w : Lb + w_off + WDY + (unsigned)((u * 3 + 2) * 64 + l31) * 16u;
            const unsigned sab = dy == 0 ? hd_sa : Lb + w_off + WDY + W_GRAN_L + (unsigned)(u * 64 + l31);
            const unsigned bb = dy == 0 ? hd_b : Lb + in_off + 2 * PLANE_L + pb;
            const unsigned sbb = dy == 0 ? hd_sb : Lb + in_off + 3 * PLANE_L + (pb >> 2);
_Pragma("unroll")
            for (int m = 0; m < 2; ++m) { a4[m] = *(lds_cu32x4*)(at(wb) + m * 512); sa[m] = *(lds_cuchar*)(at(sab) + m * 32); }
_Pragma("unroll")
            for (int q = 0; q < 2; ++q) {
                b4[q] = *(lds_cu32x4*)(at(bb) + q * QL);
                sb[q] = *(lds_cint*)(at(sbb) + q * (QL >> 2));
            }
_Pragma("unroll")
            for (int m = 0; m < 2; ++m)
_Pragma("unroll")
                for (int q = 0; q < 2; ++q) wsu_mfma_q4(a4[m], b4[q], sa[m], sb[q], acc[m][q]);
        }
        WSU_STATIC_FOR(2, dx, {
            u32x4 ah[2], bh[2];
            const unsigned wb = a_off + WDY + (unsigned)(((cls * 2 + dx) * WPL) * 64) * 16u;
            const unsigned pb = b_off + rowo + dx * 16u;
_Pragma("unroll")
            for (int m = 0; m < 2; ++m) ah[m] = *(lds_cu32x4*)(at(wb) + m * 512);
_Pragma("unroll")
            for (int q = 0; q < 2; ++q) bh[q] = *(lds_cu32x4*)(at(pb) + q * QL);
_Pragma("unroll")
            for (int m = 0; m < 2; ++m)
_Pragma("unroll")
                for (int q = 0; q < 2; ++q) wsu_mfma_f16(ah[m], bh[q], acc[m][q]);
        });
    };

    // ---- epilogue of the tile: bias, ReLU, planar Q encoding (the producing epilogue of conv3x3_q.hip), straight from the accumulators.  This
    // lane's pixels: matrix tile q -> (y0 + 2 (4 rh + 2 q + lrow) + py, x0 + 2 lcol + px)
    auto finish_tile = [&]() __attribute__((always_inline)) {
        int l31o = l31, hho = hh, lro = lrow, lco = lcol;
        asm volatile("" : "+v"(l31o), "+v"(hho), "+v"(lro), "+v"(lco));   // per-tile copies (see conv3x3_q.hip: hoisted lane values were spilled)
        const unsigned hw16 = (unsigned)(a.h * a.w) * 16u;
        const unsigned cbytes = (unsigned)wsu_q_chunk_bytes(a.h, a.w);
        const int nco = a.cout >> 4;
        const int X = cur.x0 + 2 * lco + px;
        const int Y0 = cur.y0 + 2 * (4 * rh + lro) + py, Y1 = Y0 + 4;
        const bool ok0 = Y0 < a.h && X < a.w, ok1 = Y1 < a.h && X < a.w;
        const unsigned off0 = (unsigned)(Y0 * a.w + X) * 16u, off1 = (unsigned)(Y1 * a.w + X) * 16u;
        const unsigned so0 = wsu_q_soff(Y0, X, a.tiles_x), so1 = wsu_q_soff(Y1, X, a.tiles_x);
        // the lane offsets of a piece's stores with their predicates folded in, once per tile and opaque (the four pieces change the descriptor only):
        // f16 granules of matrix tiles 0 / 1 (plane hh), the Q granule and the scale byte of tile hh
        const unsigned hpl = hho ? hw16 : 0u;
        const bool okm = hho ? ok1 : ok0;
        unsigned og0 = ok0 ? off0 + hpl : OOB, og1 = ok1 ? off1 + hpl : OOB;
        unsigned oq = okm ? (hho ? off1 : off0) + 2u * hw16 : OOB, os = okm ? 3u * hw16 + (hho ? so1 : so0) : OOB;
        asm volatile("" : "+v"(og0), "+v"(og1), "+v"(oq), "+v"(os));
        const float relu_floor = a.relu ? 0.f : -__builtin_inff();
        float vmax = 0.f;
        WSU_STATIC_FOR(2, m, {
            WSU_STATIC_FOR(2, cp, {
                const int oc = cur.cb * 4 + m * 2 + cp;
                const int co0 = oc * 16 + 4 * hho;
                const f32x4 bx = *reinterpret_cast<const f32x4*>(s_bias + co0), by = *reinterpret_cast<const f32x4*>(s_bias + co0 + 8);
                f32x4 vx[2], vy[2];
_Pragma("unroll")
                for (int q = 0; q < 2; ++q)
_Pragma("unroll")
                    for (int e = 0; e < 4; ++e) {
                        const float x = fmaxf(acc[m][q][8 * cp + e] + bx[e], relu_floor), y = fmaxf(acc[m][q][8 * cp + 4 + e] + by[e], relu_floor);
                        vx[q][e] = x; vy[q][e] = y;
                        if constexpr (H) vmax = fmaxf(fmaxf(vmax, fabsf(x)), fabsf(y));   // (format Q: the encode's maximum chain below)
                    }
                if constexpr (H) {                                              // f16 granules only: lanes 0-31 plane 0, lanes 32-63 plane 1
                    char* base = a.y + ((size_t)cur.n * nco + oc) * (2u * hw16);
                    const auto rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)(2u * hw16), 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b128(wsu_h_granule(vx[0], vy[0]), rs, (int)og0, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(wsu_h_granule(vx[1], vy[1]), rs, (int)og1, 0, 0);
                    return;                                                     // (this piece's lambda)
                }
                u32x4 g0, g1; uint32_t dh0, dr0, sb0, dh1, dr1, sb1;
                const float mx0 = wsu_q4_pre(vx[0], vy[0], g0, dh0, dr0, sb0);
                const float mx1 = wsu_q4_pre(vx[1], vy[1], g1, dh1, dr1, sb1);
                vmax = wsu_max3(vmax, mx0, mx1);
                const u32x4 qg = wsu_q4_pair(dh0, dr0, dh1, dr1);           // lanes 0-31: matrix tile 0's granule, lanes 32-63: tile 1's
                char* base = a.y + ((size_t)cur.n * nco + oc) * cbytes;
                const auto rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)cbytes, 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b128(g0, rs, (int)og0, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(g1, rs, (int)og1, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(qg, rs, (int)oq, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(hho ? sb1 : sb0), rs, (int)os, 0, 0);
            });
        });
        if (a.range_flag && __builtin_amdgcn_ballot_w64(!(vmax <= (H ? WSU_F16_RANGE : WSU_F8_RANGE))) != 0 && lane == 0) atomicOr(a.range_flag, 1u);
    };

    for (int t = 0; t < K; ++t) {
        // a tile opens with a skip chunk: no accumulator clear, its first unit writes C = 0 + products.  nchS >= 1 is what the loaders count on too
        // (one barrier per step on both sides): wsu_conv3x3_up_q_fwd / _h_fwd refuse c2 == 0 (WSU_REQUIRE) before anything is launched
        sync_step(std::false_type{});
        skip_units(std::true_type{});
        for (int c = 1; c < a.nchS; ++c) {
            sync_step(std::false_type{});
            skip_units(std::false_type{});
        }
        for (int c = 0; c < a.nchL; ++c) {                                    // one step: dy = 0 then dy = 1, the accumulation order of the two-kernel path
            sync_step(std::true_type{});
            low_units(std::integral_constant<int, 0>{});
            low_units(std::integral_constant<int, 1>{});
        }
        finish_tile();
        if (t + 1 < K) cur = tile_of(a, lw + (t + 1) * G);
    }
}

// ---- packing of the low half: one thread per (block, low chunk, dy, class, dx, co) forms its 16 combined weights in fp32 (ci outer, then ky, kx,
// fused multiply-adds) and encodes them like wsu_conv3x3_pack_f4 encodes a weight block (format H: rounds them to f16 once, like
// wsu_conv3x3_pack_h).  wc_dense (optional): the fp32 values, [cout][cl][py][px][dy][dx] -- what the tests emulate the arithmetic on.
template <int FMT>
__global__ void pack_up_low_kernel(const float* __restrict__ w3, const float* __restrict__ wt, char* __restrict__ dst, float* __restrict__ wc_dense,
                                   int cup, int c2, int cl, int cout) {
    const int nchL = cl / 16, ctot = cup + c2;
    const long long total = (long long)(cout / WSU_COB) * nchL * 2 * W_UNITS_L * WSU_COB;
    for (long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x; d < total; d += (long long)gridDim.x * blockDim.x) {
        long long t = d;
        const int co = (int)(t % WSU_COB); t /= WSU_COB;
        const int u = (int)(t % W_UNITS_L); t /= W_UNITS_L;
        const int dy = (int)(t & 1); t >>= 1;
        const int c = (int)(t % nchL); const int cb = (int)(t / nchL);
        const int cls = u >> 1, dx = u & 1, py = cls >> 1, px = cls & 1;
        // taps of the 3x3 window that fall on low row i - 1 + py + dy: py = 0: dy 0 <- ky 0; dy 1 <- ky 1, 2.  py = 1: dy 0 <- ky 0, 1; dy 1 <- ky 2
        const int ky0 = py == 0 ? (dy == 0 ? 0 : 1) : (dy == 0 ? 0 : 2), ky1 = py == 0 ? (dy == 0 ? 0 : 2) : (dy == 0 ? 1 : 2);
        const int kx0 = px == 0 ? (dx == 0 ? 0 : 1) : (dx == 0 ? 0 : 2), kx1 = px == 0 ? (dx == 0 ? 0 : 2) : (dx == 0 ? 1 : 2);
        const int cog = cb * WSU_COB + co;
        float v[16], r[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = 0.f;
        for (int ci = 0; ci < cup; ++ci)
            for (int ky = ky0; ky <= ky1; ++ky)
                for (int kx = kx0; kx <= kx1; ++kx) {
                    const float w = w3[(((size_t)cog * ctot + ci) * 3 + ky) * 3 + kx];
                    const int sy = (py + ky + 1) & 1, sx = (px + kx + 1) & 1;       // sub-position of the upsampled pixel under this tap
#pragma unroll
                    for (int e = 0; e < 16; ++e) v[e] = fmaf(w, wt[(((size_t)(c * 16 + e) * cup + ci) * 2 + sy) * 2 + sx], v[e]);
                }
        if (wc_dense)
#pragma unroll
            for (int e = 0; e < 16; ++e) wc_dense[((((size_t)cog * cl + c * 16 + e) * 2 + py) * 2 + px) * 4 + dy * 2 + dx] = v[e];
        uint32_t h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const _Float16 x = (_Float16)v[2 * e], y = (_Float16)v[2 * e + 1];
            h[e] = (uint32_t)__builtin_bit_cast(unsigned short, x) | ((uint32_t)__builtin_bit_cast(unsigned short, y) << 16);
            r[2 * e] = (v[2 * e] - (float)x) * 2048.f; r[2 * e + 1] = (v[2 * e + 1] - (float)y) * 2048.f;
        }
        const u32x4 h0 = mk_u4(h[0], h[1], h[2], h[3]), h1 = mk_u4(h[4], h[5], h[6], h[7]);
        if constexpr (FMT == WSU_PLANAR_H) {                               // slice [class 4][dx 2][plane 2][64 co][16 B]
            char* base = dst + (((size_t)cb * nchL + c) * 2 + dy) * W_L_H + (size_t)(u * 2) * (WSU_COB * 16) + co * 16;
            *reinterpret_cast<u32x4*>(base) = h0;
            *reinterpret_cast<u32x4*>(base + WSU_COB * 16) = h1;
            continue;
        }
        const int E = wsu_q4_block_exp(wsu_f16x16_max_abs_bits(h0, h1));
        const float sc = wsu_pow2f(E);
        uint32_t q[4] = {0, 0, 0, 0};
        WSU_STATIC_FOR(8, e, { q[e >> 2] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q[e >> 2], r[2 * e], r[2 * e + 1], sc, e & 3); });
        q[2] = wsu_f16x8_to_fp4(h0, sc); q[3] = wsu_f16x8_to_fp4(h1, sc);
        char* slice = dst + (((size_t)cb * nchL + c) * 2 + dy) * W_L;
        char* base = slice + (size_t)(u * 3) * (WSU_COB * 16) + co * 16;
        *reinterpret_cast<u32x4*>(base) = h0;
        *reinterpret_cast<u32x4*>(base + WSU_COB * 16) = h1;
        *reinterpret_cast<u32x4*>(base + 2 * WSU_COB * 16) = mk_u4(q[0], q[1], q[2], q[3]);
        slice[W_GRAN_L + u * 64 + co] = (char)(E + 127 - 11);
        if (u == 0 && co < 32) *reinterpret_cast<u32x4*>(slice + W_GRAN_L + 512 + co * 16) = mk_u4(0, 0, 0, 0);      // the 512 pad bytes
    }
}

// combined bias: b3[co] + sum_{ci < cup} bT[ci] * sum_{taps} w3[co][ci][tap] (reflect padding: every output pixel has all nine taps)
__global__ void up_bias_kernel(const float* __restrict__ w3, const float* __restrict__ bt, const float* __restrict__ b3, float* __restrict__ out, int cup, int c2, int cout) {
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co >= cout) return;
    float s = b3 ? b3[co] : 0.f;
    if (bt)
        for (int ci = 0; ci < cup; ++ci) {
            float t = 0.f;
            for (int k = 0; k < 9; ++k) t += w3[((size_t)co * (cup + c2) + ci) * 9 + k];
            s = fmaf(bt[ci], t, s);
        }
    out[co] = s;
}

// ---- the host side, once for both formats: what differs between Q (mode 'f16f4p') and H (mode 'f16p') is this row (the kernels are instantiated
// here, in the order the rows name them)
struct UFormat {
    const char* pack; const char* fwd;                                      // message prefixes
    void (*pack_kernel)(const float*, const float*, char*, float*, int, int, int, int); const char* pack_kernel_name;
    void (*kernel)(const UArgs); const char* kernel_name; const char* lds_name;
    int w_s, w_l;                                                           // bytes of a skip slice and of a dy slice of the low half
};
const UFormat& u_format(int fmt) {
    static const UFormat q = {"conv3x3_up_pack", "conv3x3_up_q", pack_up_low_kernel<WSU_PLANAR_Q>, "pack_up_low_kernel",
                              conv3x3_qu_kernel<WSU_PLANAR_Q>, "conv3x3_qu_kernel", "conv3x3_qu", W_S, W_L};
    static const UFormat h = {"conv3x3_up_pack_h", "conv3x3_up_h", pack_up_low_kernel<WSU_PLANAR_H>, "pack_up_low_kernel<H>",
                              conv3x3_qu_kernel<WSU_PLANAR_H>, "conv3x3_qu_kernel<H>", "conv3x3_qu<H>", W_S_H, W_L_H};
    return fmt == WSU_PLANAR_H ? h : q;
}

size_t up_packed_bytes(int fmt, int cl, int cout) {
    if (cl <= 0 || cout <= 0 || cl % 16 || cout % WSU_COB) return 0;
    return (size_t)(cout / WSU_COB) * (cl / 16) * 2 * u_format(fmt).w_l;
}

int up_pack(int fmt, const float* w3_oihw, const float* wt, const float* bt, const float* b3, void* w_low_packed, float* bias_out, float* wc_dense,
            int cl, int cup, int c2, int cout, void* stream) {
    const UFormat& f = u_format(fmt);
    WSU_REQUIRE(w3_oihw && wt && w_low_packed && bias_out, "%s: null pointer", f.pack);
    WSU_REQUIRE(cl > 0 && cl % 16 == 0 && cup > 0 && c2 >= 0 && cout > 0 && cout % WSU_COB == 0,
                "%s: cl=%d must be a multiple of 16, cout=%d of %d, cup=%d > 0", f.pack, cl, cout, WSU_COB, cup);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(f.pack_kernel, dim3(1024), dim3(128), 0, s, w3_oihw, wt, (char*)w_low_packed, wc_dense, cup, c2, cl, cout);
    int rc = wsu_check_launch(f.pack_kernel_name);
    if (rc != WSU_OK) return rc;
    hipLaunchKernelGGL(up_bias_kernel, dim3((cout + 63) / 64), dim3(64), 0, s, w3_oihw, bt, b3, bias_out, cup, c2, cout);
    return wsu_check_launch("up_bias_kernel");
}

int up_fwd(int fmt, const void* x_low, const void* x_skip, const void* w_skip_packed, const void* w_low_packed, const float* bias, void* y,
           int n, int h, int w, int cl, int c2, int cout, int relu, unsigned* range_flag, void* stream) {
    const UFormat& f = u_format(fmt);
    const char* who = f.fwd;
    WSU_REQUIRE(x_low && x_skip && w_skip_packed && w_low_packed && y, "%s: null pointer", who);
    WSU_REQUIRE(n > 0 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "%s: bad shape n=%d h=%d w=%d (the output of a stride-2 transposed conv is even)", who, n, h, w);
    WSU_REQUIRE(cl > 0 && cl % 16 == 0 && c2 > 0 && c2 % 16 == 0, "%s: cl=%d c2=%d must be positive multiples of 16", who, cl, c2);
    WSU_REQUIRE(cout > 0 && cout % WSU_COB == 0 && cout <= MAX_COUT, "%s: cout=%d must be a multiple of %d (<= %d)", who, cout, WSU_COB, MAX_COUT);
    WSU_REQUIRE((long long)h * w * 50 < 0xFFFFFFF0LL, "%s: h*w too large (a chunk must stay below 4 GiB)", who);
    UArgs a;
    a.xl = (const char*)x_low; a.xs = (const char*)x_skip; a.wps = (const char*)w_skip_packed; a.wpl = (const char*)w_low_packed; a.bias = bias;
    a.y = (char*)y;
    a.n = n; a.h = h; a.w = w; a.hl = h / 2; a.wl = w / 2; a.cl = cl; a.c2 = c2; a.cout = cout;
    a.tiles_x = (w + TW - 1) / TW; a.tiles_y = (h + TH - 1) / TH; a.ltiles_x = (a.wl + 31) / 32; a.ncb = cout / WSU_COB;
    a.nchS = c2 / 16; a.nchL = cl / 16; a.relu = relu; a.range_flag = range_flag;
    const long long nt = (long long)n * a.tiles_x * a.tiles_y * a.ncb;
    WSU_REQUIRE(nt > 0 && nt < 0x3FFFFFFFLL, "%s: %lld tiles out of range", who, nt);
    WSU_REQUIRE((long long)a.ncb * a.nchL * 2 * f.w_l < 0x7FFFFFF0LL && (long long)a.ncb * a.nchS * f.w_s < 0x7FFFFFF0LL, "%s: packed weights beyond 2 GiB", who);
    a.ntiles = (int)nt;
    const int ncu = wsu_cu_count(who);
    if (!ncu) return WSU_ERR_HIP;
    static bool raised[2] = {false, false};
    bool& done = raised[fmt == WSU_PLANAR_H];
    if (!done) {
        if (int rc = wsu_raise_lds(f.kernel, LDS_TOTAL, f.lds_name)) return rc;
        done = true;
    }
    hipLaunchKernelGGL(f.kernel, dim3(a.ntiles < ncu ? a.ntiles : ncu), dim3(NT), LDS_TOTAL, static_cast<hipStream_t>(stream), a);
    return wsu_check_launch(f.kernel_name);
}

}  // namespace

extern "C" {

// Bytes of the packed low half: per (64-co block, 16-channel chunk of x_low, dy) one 25 KB slice [class 4][dx 2][plane 3][64 co][16 B] + [8][64] scale bytes.
size_t wsu_conv3x3_up_packed_bytes(int cl, int cout) { return up_packed_bytes(WSU_PLANAR_Q, cl, cout); }

// Packs the upsampled half of a decoder block's first conv.  w3: (cout, cup + c2, 3, 3) OIHW fp32, the conv's weights (input channels
// [0, cup) = the transposed conv's output, as torch.cat([xu, skip]) orders them, unet.py:172,178,184); wt: (cl, cup, 2, 2) fp32, the
// nn.ConvTranspose2d weights; bt (cup) / b3 (cout): their biases (optional).  Out: w_low_packed (wsu_conv3x3_up_packed_bytes), bias_out (cout
// floats: the combined bias) and, optional, wc_dense (cout * cl * 16 floats [cout][cl][py][px][dy][dx]: the combined weights in fp32).
// The skip half is wsu_conv3x3_pack_f4 of w3[:, cup:].
int wsu_conv3x3_up_pack(const float* w3_oihw, const float* wt, const float* bt, const float* b3, void* w_low_packed, float* bias_out, float* wc_dense,
                        int cl, int cup, int c2, int cout, void* stream) {
    return up_pack(WSU_PLANAR_Q, w3_oihw, wt, bt, b3, w_low_packed, bias_out, wc_dense, cl, cup, c2, cout, stream);
}

// Forward of relu(conv3x3_reflect(cat[convT2x2_s2(x_low), x_skip])) in one launch (K1u above).  x_low: planar Q tensor, cl channels at (h/2) x
// (w/2); x_skip: planar Q tensor, c2 channels at h x w; w_skip_packed: wsu_conv3x3_pack_f4(w3[:, cup:], c2, cout); w_low_packed / bias: from
// wsu_conv3x3_up_pack; y: planar Q tensor, cout channels at h x w.  h, w even; cl, c2 multiples of 16 (> 0), cout of 64 (<= 512).
// range_flag as in wsu_conv3x3_q_fwd.  Asynchronous on `stream`; allocates nothing.
int wsu_conv3x3_up_q_fwd(const void* x_low, const void* x_skip, const void* w_skip_packed, const void* w_low_packed, const float* bias, void* y,
                         int n, int h, int w, int cl, int c2, int cout, int relu, unsigned* range_flag, void* stream) {
    return up_fwd(WSU_PLANAR_Q, x_low, x_skip, w_skip_packed, w_low_packed, bias, y, n, h, w, cl, c2, cout, relu, range_flag, stream);
}

// ---- format H (mode 'f16p', include/wsu.h K1h) ----------------------------------------------------------------------------------------
// Bytes of the packed low half in format H: per (64-co block, 16-channel chunk of x_low, dy) one 16 KB slice [class 4][dx 2][plane 2][64 co][16 B].
size_t wsu_conv3x3_up_packed_h_bytes(int cl, int cout) { return up_packed_bytes(WSU_PLANAR_H, cl, cout); }

// wsu_conv3x3_up_pack in format H: the combined weights rounded to f16 once (wc_dense and bias_out as there).  The skip half is
// wsu_conv3x3_pack_h of w3[:, cup:].
int wsu_conv3x3_up_pack_h(const float* w3_oihw, const float* wt, const float* bt, const float* b3, void* w_low_packed, float* bias_out, float* wc_dense,
                          int cl, int cup, int c2, int cout, void* stream) {
    return up_pack(WSU_PLANAR_H, w3_oihw, wt, bt, b3, w_low_packed, bias_out, wc_dense, cl, cup, c2, cout, stream);
}

// wsu_conv3x3_up_q_fwd on planar H tensors (x_low, x_skip, y): weights of wsu_conv3x3_pack_h (skip half) and wsu_conv3x3_up_pack_h.
int wsu_conv3x3_up_h_fwd(const void* x_low, const void* x_skip, const void* w_skip_packed, const void* w_low_packed, const float* bias, void* y,
                         int n, int h, int w, int cl, int c2, int cout, int relu, unsigned* range_flag, void* stream) {
    return up_fwd(WSU_PLANAR_H, x_low, x_skip, w_skip_packed, w_low_packed, bias, y, n, h, w, cl, c2, cout, relu, range_flag, stream);
}

}  // extern "C"
