/* wsu.h -- C ABI of the MI355X-native UNet pixel-predictor hot path (libwsu.so).
 *
 * The reference (uibk-uncover/ws-unet) is pure Python on PyTorch and has NO FFI /
 * plugin interface; the compute this library replaces is what `UNet.forward`
 * (src/unet/model/unet.py:137-189) dispatches to ATen.  Each entry point below
 * names the reference call site it stands in for.  The Python host side
 * (ws_unet_amd/model/unet.py) binds these with ctypes and keeps the reference's
 * own module / evaluate API on top.
 *
 * Conventions
 *  - plain C types only; every buffer pointer is a DEVICE pointer owned by the
 *    caller (PyTorch-ROCm caching allocator in our host code); the library
 *    allocates nothing and keeps no global mutable state (re-entrant; one host
 *    thread per GPU may call concurrently);
 *  - `stream` is a hipStream_t passed as void*; all work is asynchronous on it;
 *  - returns 0 on success, a negative code on bad arguments / HIP error, message
 *    via wsu_last_error() (thread-local);  never throws;
 *  - activations are NHWC (N*H*W*C contiguous).  With C == 1 this coincides with
 *    the reference's NCHW, so model input (N,1,H,W) and output (N,1,H,W) need no
 *    re-layout;
 *  - `mode` selects storage + arithmetic:
 *      WSU_MODE_F32    = 0  fp32 storage, exact fp32 MFMA (v_mfma_f32_32x32x2_f32)
 *      WSU_MODE_BF16X3 = 1  fp32 storage, split-bf16 (hi*hi + hi*lo + lo*hi) on
 *                           v_mfma_f32_32x32x16_bf16, fp32 accumulate (~2^-17 rel. error)
 *      WSU_MODE_BF16   = 2  bf16 storage, bf16 MFMA, fp32 accumulate
 *      WSU_MODE_BF16X3S = 3 the arithmetic of BF16X3 on activations stored ALREADY SPLIT by their producer: per pixel and 16-channel
 *                           chunk  [bf16 hi of ch 0-7][hi 8-15][lo 0-7][lo 8-15]  (4 x 16 B = the fp32 chunk size, so tensors keep
 *                           their fp32 allocation).  Staging becomes a plain copy; results are bitwise those of BF16X3.  Forward
 *                           entry points only (wsu_conv3x3_fwd / _head_fwd / _fused_first_fwd, wsu_convt2x2_fwd); weights are packed
 *                           as for BF16X3; no pool_idx, no zero padding.
 *      WSU_MODE_F16F8 = 4   two-level split on the f16 and block-scaled fp8 matrix pipes (forward inference format like BF16X3S):
 *                           w*x ~ f16(w)*f16(x) + e4m3(w)*e4m3(x - f16(x)) + e4m3(w - f16(w))*e4m3(x), fp32 accumulate.  The first
 *                           product is exact (v_mfma_f32_32x32x16_f16), the two cross terms share one
 *                           v_mfma_scale_f32_32x32x64_f8f6f4 (2x the bf16 rate; its two 32-element scale blocks carry 2^-12-sized
 *                           residuals at full e4m3 precision): ~2^-15 relative error per product at 2/3 of BF16X3's matrix cycles.
 *                           Activations take 3 bytes per element: per pixel and 16-channel chunk [f16 ch 0-7][f16 ch 8-15]
 *                           [e4m3((x - f16 x) * 2^12) ch 0-15] = 48 bytes, pixel stride C * 3 bytes (the e4m3 copy e4m3(x / 4) that
 *                           the second cross term needs is derived from the f16 part while staging); weights packed by the pack
 *                           entry points with this mode (4 bytes per weight).  Values beyond +-448 lose the residual term (plain f16 accuracy); beyond +-65504 the f16 part overflows
 *                           like any f16 pipeline (use BF16X3S for such networks).
 *      WSU_MODE_F16F8X = 5  the arithmetic of F16F8 on fp32 tensors (operands encoded while staging, fp32 results): the matrix kernels of
 *                           the training path -- wsu_conv3x3_fwd (with pool and pool_idx), wsu_convt2x2_fwd, wsu_conv3x3_bwd_data,
 *                           wsu_conv3x3_bwd_weight, wsu_convt2x2_bwd_weight; weights packed as for F16F8.  Gradient operands must be
 *                           brought into f16's range by the caller (a power-of-two scale, undone on the results).
 */
#ifndef WSU_H
#define WSU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WSU_VERSION 100

enum { WSU_MODE_F32 = 0, WSU_MODE_BF16X3 = 1, WSU_MODE_BF16 = 2, WSU_MODE_BF16X3S = 3, WSU_MODE_F16F8 = 4, WSU_MODE_F16F8X = 5 };

/* `products` of the planar BACKWARD matrix kernels (wsu_conv3x3_pl_bwd_data / _bwd_weight, wsu_convt2x2_pl_bwd_data / _bwd_weight) -- which terms of
 * (f16 a + residual a)(f16 b + residual b) are multiplied:
 *      WSU_PRODUCTS_F16F8 = 0  f16 a * f16 b on the f16 pipe + both residual cross terms on the block-scaled fp8 pipe (the forward's arithmetic,
 *                              ~2^-16 per product; 19 matrix units per 9 of plain f16 in the data gradient, 4 per 2 in the weight gradient);
 *      WSU_PRODUCTS_F16   = 1  f16 a * f16 b only (2^-11 per operand, unbiased rounding, fp32 accumulation): the residual planes are neither
 *                              fetched nor multiplied.  A weight gradient sums 10^6..10^7 such products per element and a data gradient
 *                              9 * cout of them, so the rounding noise averages out to a relative L2 of <= 2e-4 per weight gradient and
 *                              ~1e-4 per data-gradient layer (tests/test_gpu_planar_train.py) -- below the 1e-3 that ReLU-mask flips from
 *                              the FORWARD's own rounding put between any two arithmetics on these networks, and 8x finer than bf16
 *                              autocast.  The forward pass and the activations' format do not change; gradient tensors then hold f16
 *                              values (their residual plane is not used, see the K7p notes below). */
enum { WSU_PRODUCTS_F16F8 = 0, WSU_PRODUCTS_F16 = 1 };

enum {
    WSU_OK = 0,
    WSU_ERR_ARG = -1,      /* bad argument (shape, mode, null pointer) */
    WSU_ERR_HIP = -2,      /* a HIP call / launch failed */
    WSU_ERR_UNSUPPORTED = -3
};

int wsu_version(void);
const char* wsu_last_error(void);

/* Bytes per activation element for a mode (4, 4, 2, 4, 3, 4). */
int wsu_act_elem_size(int mode);

/* ---- weight packing (done once per weight update; replaces nothing in the reference:
 *      it re-lays nn.Conv2d's OIHW fp32 weight, unet.py:82-132, for the MFMA A operand) */
size_t wsu_conv3x3_packed_bytes(int cin, int cout, int mode);
int wsu_conv3x3_pack(const float* w_oihw, void* w_packed, int cin, int cout, int mode, void* stream);
/* transposed: packs w^T flipped (for the data-gradient pass), from the same OIHW source */
int wsu_conv3x3_pack_dgrad(const float* w_oihw, void* w_packed, int cin, int cout, int mode, void* stream);
size_t wsu_convt2x2_packed_bytes(int cin, int cout, int mode);
/* w is nn.ConvTranspose2d's (Cin, Cout, 2, 2) fp32 weight, unet.py:125,130 */
int wsu_convt2x2_pack(const float* w_iohw, void* w_packed, int cin, int cout, int mode, void* stream);

/* ---- K1 (+K2, K4): y = [relu](conv3x3_reflect(cat[x1, x2]) + bias), optional fused 2x2 max-pool.
 *      Replaces nn.Conv2d(k3, pad 1, reflect) + F.relu (unet.py:141-186), torch.cat (unet.py:178,184)
 *      and nn.MaxPool2d (unet.py:144,149).
 *      x1: (N,H,W,C1), x2: (N,H,W,C2) or NULL (C2 == 0); channels of x1 come first (upsampled, then skip).
 *      C1, C2 multiples of 16 (fp32 modes) / 32 (bf16); Cout multiple of 64; H, W >= 2.
 *      y: (N,H,W,Cout).  y_pool: (N,H/2,W/2,Cout) or NULL.  pool_idx: uint8 (N,H/2,W/2,Cout) argmax in
 *      row-major window order with first-max-wins ties, or NULL.  pad_zero != 0 selects zero instead of
 *      reflect padding (used by the data-gradient pass). */
int wsu_conv3x3_fwd(const void* x1, const void* x2, const void* w_packed, const float* bias,
                    void* y, void* y_pool, uint8_t* pool_idx,
                    int n, int h, int w, int c1, int c2, int cout,
                    int mode, int relu, int pad_zero, void* stream);

/* ---- K1 + K5 fused (last layer): out[n,co,y,x] = sigmoid(head_b[co] + sum_c head_w[co,c] * relu(conv3x3(cat[x1,x2]) + bias)[n,y,x,c]).
 *      Replaces d42 + outconv + F.sigmoid (unet.py:186,189) in one launch; cout must be 64, head_cout 1..4.
 *      out / logit (optional): NCHW fp32.  y (optional): also store the 64-channel conv output (NHWC). */
int wsu_conv3x3_head_fwd(const void* x1, const void* x2, const void* w_packed, const float* bias, void* y,
                         const float* head_w, const float* head_b, float* out, float* logit,
                         int n, int h, int w, int c1, int c2, int cout, int head_cout, int mode, void* stream);

/* ---- K1f: first layer fused into the conv behind it (e11 -> e12 [-> pool], unet.py:141-144) for single-plane inputs: the 64
 *      channels of e11 are computed from the image while e12 stages its input tile and never reach HBM.  Bitwise the same result
 *      as wsu_conv3x3_first_fwd followed by wsu_conv3x3_fwd.  img: (N,1,H,W) fp32; w1: (64,1,3,3) OIHW; b1: (64) or NULL;
 *      w_packed / bias: the second conv (cin = 64) as for wsu_conv3x3_fwd; y: (N,H,W,cout); y_pool / pool_idx optional. */
int wsu_conv3x3_fused_first_fwd(const float* img, const float* w1, const float* b1, const void* w_packed, const float* bias,
                                void* y, void* y_pool, uint8_t* pool_idx, int n, int h, int w, int cout, int mode, int relu, void* stream);

/* ---- K1w: the same forward conv (mode bf16x3 only: fp32 NHWC activations) through a Winograd F(2,3) kernel along x:
 *      1.5x fewer MFMAs, results equal to the direct kernel up to fp32 re-association.  Weights from wsu_conv3x3_wino_pack
 *      ([cob][chunk][12 taps][4 planes][64 co][16 B], row taps pre-multiplied by G).  Same fusions: x2 = second concat source,
 *      y_pool / pool_idx = fused 2x2 max-pool (+argmax), head_* = fused 1x1 head + sigmoid (y may then be NULL). */
size_t wsu_conv3x3_wino_packed_bytes(int cin, int cout);
int wsu_conv3x3_wino_pack(const float* w_oihw, void* w_packed, int cin, int cout, void* stream);
int wsu_conv3x3_wino_fwd(const void* x1, const void* x2, const void* w_packed, const float* bias, void* y,
                         void* y_pool, uint8_t* pool_idx,
                         const float* head_w, const float* head_b, float* head_out, float* head_logit, int head_cout,
                         int n, int h, int w, int c1, int c2, int cout, int relu, void* stream);

/* ---- K1p: the same forward conv in the f16f8 arithmetic on PLANAR activations ("F16F8P" storage, forward inference only): a tensor of C
 *      channels is [n][C/16 chunks][3 planes][H][W][16 B] with, per pixel and 16-channel chunk, plane 0 = f16 ch 0-7, plane 1 = f16 ch
 *      8-15, plane 2 = e4m3((x - f16 x) * 2^12) ch 0-15 (3 bytes per element).  The planes are three of the four LDS planes of the matrix
 *      kernel (the fourth, e4m3(x / 4), is derived from the f16 planes by the loader wave that fetched them), so staging is a pure LDS-DMA
 *      (global_load_lds) and a persistent workgroup per CU pipelines it across chunks and tiles (csrc/conv3x3_pl.hip).  Weights from wsu_conv3x3_pack(mode F16F8).  Outputs, each optional: y (planar),
 *      y_pool (2x2 max-pooled, planar), head (1x1 conv + sigmoid on cout == 64 channels; out / logit NCHW fp32).  range_flag (optional
 *      device word, all three planar entry points): bit 0 is OR-ed in when a stored activation exceeds +-448, where the e4m3 residual
 *      saturates and that value keeps only f16 accuracy (NaN / Inf set it too) -- the caller's signal to switch to BF16X3S.
 *      x_residual = 0 (plain variant only): the inputs' residual plane is neither loaded nor multiplied -- w*x ~ f16(w)*f16(x) + e4m3(w - f16 w)*e4m3(x),
 *      15 instead of 19 matrix units per chunk; the activation rounding of THIS layer's inputs then costs ~2.5e-5 MAE on the network output
 *      (profiles/r02/conv3x3_units_probe.md), so a caller spends it on at most a few layers.  Replaces the same
 *      reference lines as wsu_conv3x3_fwd / wsu_conv3x3_head_fwd (unet.py:141-189). */
/*      x_residual = 2 (round 3): both cross terms in ONE block-scaled fp4 (e2m1) MFMA per tap pair -- w*x ~ f16(w)*f16(x) + 2^(Ew+Ex-11) [fp4(rw 2^11/2^Ew)
 *      fp4(f16 x/2^Ex) + fp4(f16 w/2^Ew) fp4(rx 2^11/2^Ex)], rw / rx the residuals, 2^Ew / 2^Ex E8M0 block scales per (output channel, tap, 16 input
 *      channels) / per (pixel, 16 channels) = the smallest power of two that does not saturate fp4 (the block's largest f16 part maps into [2, 3) or [4, 6]): 14 instead of 19 matrix units per chunk.  The
 *      activations' stored format does not change (the loader waves derive the fp4 granule and scale byte of a pixel from its three stored granules);
 *      the weights come from wsu_conv3x3_pack_f4 (wsu_conv3x3_packed_f4_bytes).  MAE of the unet_2 output ~2.1e-5 instead of 4e-6. */
size_t wsu_conv3x3_packed_f4_bytes(int cin, int cout);
int wsu_conv3x3_pack_f4(const float* w_oihw, void* w_packed, int cin, int cout, void* stream);
int wsu_conv3x3_pl_fwd(const void* x1, const void* x2, const void* w_packed, const float* bias, void* y, void* y_pool,
                       const float* head_w, const float* head_b, float* head_out, float* head_logit, int head_cout,
                       int n, int h, int w, int c1, int c2, int cout, int relu, int x_residual, unsigned* range_flag,
                       unsigned char* relu_mask_out, void* stream);
/*      relu_mask planes (round 3; training): relu_mask_out (optional; plain variant: y only) receives the 1-bit ReLU mask of y --
 *      [n][cout/8][hp][wp] bytes, hp = 16 * ceil(h / 16), wp = 32 * ceil(w / 32) (wsu_relu_mask_bytes), byte (pixel, 8-channel granule),
 *      bit e = (stored f16 value of channel 8 g + e > 0).  The data gradient of the NEXT conv reads it (mask1_bits / mask2_bits of
 *      wsu_conv3x3_pl_bwd_data) instead of the 2 bytes per element of y's f16 planes.  Rows beyond h / columns beyond w are not written. */
size_t wsu_relu_mask_bytes(int n, int c, int h, int w);

/* ---- K1q (round 4): the forward conv of the DEFAULT inference mode 'f16f4p' on planar Q tensors ("F16F4P" storage; csrc/conv3x3_q.hip).
 *      The arithmetic is x_residual = 2's: w*x ~ f16(w)*f16(x) + both residual cross terms as ONE block-scaled fp4 (e2m1) MFMA per tap pair.  What changed is
 *      WHO makes the fp4 operands: a planar Q tensor stores, per image and 16-channel chunk,
 *          plane 0 = f16 ch 0-7, plane 1 = f16 ch 8-15, plane 2 = Q   as [H][W][16 B] each, then the scale plane S,
 *      Q = per pixel 32 fp4 nibbles: nibble i = fp4(f16 part of channel i / 2^E), nibble 16 + i = fp4((x - f16 x) * 2^11 / 2^E) (low nibble first, round to
 *      nearest even, saturating), 2^E = the smallest power of two with (largest |f16 part| of the 16 channels) / 2^E <= 6; S = one byte E + 127 per pixel in
 *      16 x 32-pixel tile blocks [ceil(H/16)][ceil(W/32)][16][32] (a conv tile's scale bytes are one 512-byte run; rows / columns beyond the image are
 *      padding).  A chunk is 48 H W + 512 ceil(H/16) ceil(W/32) bytes (3.06 B per element; wsu_planar_q_bytes).  The PRODUCING epilogue writes all of it
 *      from its fp32 values (residual nibbles from the exact residual; round 3's loader waves re-rounded a stored e4m3 residual), so the consumer's loader
 *      waves only issue LDS-DMA.  y_format (this entry point, wsu_convt2x2_pl_fwd, wsu_conv3x3_first_pl_fwd): WSU_PLANAR_Q, or WSU_PLANAR_A = the
 *      e4m3-residual F16F8P format above (what the transposed conv and every training kernel read).  Weights: wsu_conv3x3_pack_f4.
 *      Replaces the same reference lines as wsu_conv3x3_pl_fwd (unet.py:141-189). */
#define WSU_PLANAR_A 0
#define WSU_PLANAR_Q 1
size_t wsu_planar_q_bytes(int n, int c, int h, int w);
int wsu_conv3x3_q_fwd(const void* x1, const void* x2, const void* w_packed_f4, const float* bias, void* y, void* y_pool,
                      const float* head_w, const float* head_b, float* head_out, float* head_logit, int head_cout,
                      int n, int h, int w, int c1, int c2, int cout, int relu, int y_format, unsigned* range_flag, void* stream);

/* ---- K0p + K1q fused (round 4): e11 -> e12 -> pool of the DEFAULT mode in one launch for single-plane inputs (unet.py:141-144; kernel variant F1 of
 *      csrc/conv3x3_q.hip).  The loader waves of the persistent kernel compute e11's 64 channels from the image straight into the LDS input slots -- fp32
 *      fused multiply-adds in the tap order of wsu_conv3x3_first_pl_fwd, the same planar-Q encoding -- instead of fetching them: bitwise the result of
 *      wsu_conv3x3_first_pl_fwd(y_format Q) followed by wsu_conv3x3_q_fwd, and xe11 never reaches HBM.  img (N,1,H,W) fp32; w1_taps (9, 64) fp32 = e11's
 *      weights TAP-MAJOR (w1.reshape(64, 9).T -- a tap's 16 channels are one scalar 16-dword load of the loader waves), b1 (64); both 64-byte aligned;
 *      w_packed_f4 / bias: the second conv (cin = 64; wsu_conv3x3_pack_f4); y, y_pool: planar Q tensors (both required).  h, w even; cout % 64 == 0. */
int wsu_conv3x3_q_fused_first_fwd(const float* img, const float* w1_taps, const float* b1, const void* w_packed_f4, const float* bias, void* y, void* y_pool,
                                  int n, int h, int w, int cout, int relu, unsigned* range_flag, void* stream);

/* ---- K1u (round 4): a decoder block's transposed conv + concat + first 3x3 conv in ONE launch, default inference mode (csrc/conv3x3_qu.hip):
 *          y = relu(conv3x3_reflect(cat[conv_transpose2x2_s2(x_low), x_skip]))        (unet.py:171-173, 177-179, 183-185)
 *      There is no non-linearity between the two convs, so the upsampled half is a 2 x 2-tap conv on x_low with weights combined per PARITY CLASS of
 *      the output pixel (row parity py, column parity px): Wc[py,px][dy,dx][co][c] = sum_ci sum_{(ky,kx) -> (dy,dx)} w3[co][ci][ky][kx] wT[c][ci][sy][sx],
 *      reading x_low rows i - 1 + py + dy, columns j - 1 + px + dx of output pixel (2 i + py, 2 j + px), CLAMPED at the border (= the reflect
 *      padding of the upsampled tensor); the transposed conv's bias folds into one combined bias per output channel.  512 instead of 576
 *      multiply-adds per output and channel pair, no transposed-conv launch, and the upsampled tensor never exists.  Arithmetic and operand
 *      formats as K1q (f16 products + block-scaled fp4 cross terms, planar Q tensors in and out).
 *      wsu_conv3x3_up_pack: w3 (cout, cup + c2, 3, 3) OIHW fp32 (input channels [0, cup) = the upsampled tensor, as torch.cat([xu, skip]) orders
 *      them), wt (cl, cup, 2, 2) fp32 (nn.ConvTranspose2d), bt (cup) / b3 (cout) biases or NULL -> w_low_packed (wsu_conv3x3_up_packed_bytes: per
 *      (64-co block, 16-channel chunk of x_low, dy) a 25 KB slice [class 4][dx 2][plane 3][64 co][16 B] + [8][64] scale bytes), bias_out (cout
 *      floats), and optionally wc_dense (cout * cl * 16 floats, [cout][cl][py][px][dy][dx]).  The skip half is wsu_conv3x3_pack_f4 of w3[:, cup:].
 *      wsu_conv3x3_up_q_fwd: x_low planar Q (cl channels at h/2 x w/2), x_skip planar Q (c2 channels at h x w) -> y planar Q (cout at h x w).
 *      h, w even; cl, c2 positive multiples of 16; cout a multiple of 64, <= 512.  Asynchronous; allocates nothing. */
size_t wsu_conv3x3_up_packed_bytes(int cl, int cout);
int wsu_conv3x3_up_pack(const float* w3_oihw, const float* wt, const float* bt, const float* b3, void* w_low_packed, float* bias_out, float* wc_dense,
                        int cl, int cup, int c2, int cout, void* stream);
int wsu_conv3x3_up_q_fwd(const void* x_low, const void* x_skip, const void* w_skip_packed, const void* w_low_packed, const float* bias, void* y,
                         int n, int h, int w, int cl, int c2, int cout, int relu, unsigned* range_flag, void* stream);

/* ---- K1h: the opt-in inference mode 'f16p' -- ONE product per tap: f16(w) * f16(x) on the f16 matrix pipe, fp32 accumulation, no cross terms.
 *      A planar H tensor ("F16P" storage) holds, per image and 16-channel chunk,
 *          plane 0 = f16 ch 0-7, plane 1 = f16 ch 8-15   as [H][W][16 B] each (round to nearest even),
 *      i.e. the first two planes of a planar Q tensor without the Q plane and the scale bytes: a chunk is 32 H W bytes (2 B per element;
 *      wsu_planar_h_bytes).  The kernels are the K1q / K1u / K0p kernels instantiated for this format (csrc/conv3x3_q.hip, conv3x3_qu.hip,
 *      planar.hip); range_flag is set only when a stored value is not a finite f16 (|v| > 65504, or NaN).
 *      wsu_conv3x3_pack_h: w (cout, cin, 3, 3) OIHW fp32 -> per (64-co block, 16-channel input chunk) an 18 KB slice [tap 9][plane 2][64 co][16 B]
 *        (wsu_conv3x3_packed_h_bytes); cin a multiple of 16, cout of 64.
 *      wsu_conv3x3_h_fwd: arguments as wsu_conv3x3_q_fwd on planar H tensors (x1, x2, y, y_pool; a y beside the fused head is an H tensor too);
 *        y_format must be WSU_PLANAR_H.
 *      wsu_conv3x3_up_pack_h: as wsu_conv3x3_up_pack, the parity-class weights combined in fp32 and rounded to f16 once -> per (64-co block,
 *        16-channel chunk of x_low, dy) a 16 KB slice [class 4][dx 2][plane 2][64 co][16 B] (wsu_conv3x3_up_packed_h_bytes).  The skip half
 *        is wsu_conv3x3_pack_h of w3[:, cup:].
 *      wsu_conv3x3_up_h_fwd: as wsu_conv3x3_up_q_fwd on planar H tensors (x_low, x_skip, y).
 *      wsu_conv3x3_first_pl_fwd with y_format WSU_PLANAR_H writes the first layer as a planar H tensor. */
#define WSU_PLANAR_H 2
size_t wsu_planar_h_bytes(int n, int c, int h, int w);
size_t wsu_conv3x3_packed_h_bytes(int cin, int cout);
int wsu_conv3x3_pack_h(const float* w_oihw, void* w_packed, int cin, int cout, void* stream);
int wsu_conv3x3_h_fwd(const void* x1, const void* x2, const void* w_packed_h, const float* bias, void* y, void* y_pool,
                      const float* head_w, const float* head_b, float* head_out, float* head_logit, int head_cout,
                      int n, int h, int w, int c1, int c2, int cout, int relu, int y_format, unsigned* range_flag, void* stream);
size_t wsu_conv3x3_up_packed_h_bytes(int cl, int cout);
int wsu_conv3x3_up_pack_h(const float* w3_oihw, const float* wt, const float* bt, const float* b3, void* w_low_packed, float* bias_out, float* wc_dense,
                          int cl, int cup, int c2, int cout, void* stream);
int wsu_conv3x3_up_h_fwd(const void* x_low, const void* x_skip, const void* w_skip_packed, const void* w_low_packed, const float* bias, void* y,
                         int n, int h, int w, int cl, int c2, int cout, int relu, unsigned* range_flag, void* stream);

/* ---- K1p + K0p fused: e11 -> e12 (-> pool) of the planar path in one launch for single-plane inputs (unet.py:141-144).  The loader waves of
 *      the persistent kernel compute e11's 64 channels from the image straight into the LDS stages (instead of fetching them); bitwise the
 *      result of wsu_conv3x3_first_pl_fwd followed by wsu_conv3x3_pl_fwd, and xe11 never reaches HBM.  img (N,1,H,W) fp32, w1 (64,1,3,3),
 *      b1 (64) or NULL; w_packed / bias: the second conv (cin = 64); y / y_pool (each optional, not both NULL) planar. */
int wsu_conv3x3_pl_fused_first_fwd(const float* img, const float* w1, const float* b1, const void* w_packed, const float* bias,
                                   void* y, void* y_pool, int n, int h, int w, int cout, int relu, unsigned* range_flag, void* stream);

/* ---- K7p: data gradient of the 3x3 reflect conv on PLANAR tensors (csrc/conv3x3_pl.hip kernel variant GRAD + csrc/train_pl.hip; autograd of
 *      unet.py:141-189).  Gradients use the F16F8P layout with the gradient's residual scaling: planes f16 | f16 | e4m3((g - f16 g) * 2^14),
 *      values pre-scaled by a power of two (wsu_pow2_grad_scale).  g: pre-activation gradient (cout channels); w_packed_dgrad from
 *      wsu_conv3x3_pack_dgrad(mode F16F8); dx1 = input channels [0, csplit), dx2 (NULL iff csplit == cin) the rest (fused concat); mask1 /
 *      mask2 (optional): planar ACTIVATIONS shaped like dx1 / dx2 -- the input of this conv as the producing layer stored it -- whose sign is
 *      that layer's ReLU mask (relu'(0) = 0).  pad_zero = 0: reflect padding; the border ring of the adjoint is one more launch of the same
 *      kernel over strips of g's border rows / columns with the four 1x3 weight sets of wsu_conv3x3_pack_ring (4 x
 *      wsu_conv3x3_packed_bytes(cin, cout, F16F8) bytes) in `workspace` (>= wsu_conv3x3_pl_bwd_data_workspace_bytes).  pad_zero = 1: the
 *      adjoint of the zero-padded conv (ring arguments unused).  cin, csplit multiples of 64, cout of 16. */
size_t wsu_conv3x3_pl_bwd_data_workspace_bytes(int n, int h, int w, int cin, int cout);
int wsu_conv3x3_pack_ring(const float* w_oihw, void* w_packed, int cin, int cout, void* stream);
int wsu_conv3x3_pl_bwd_data(const void* g, const void* w_packed_dgrad, const void* w_packed_ring, void* workspace, size_t workspace_bytes,
                            void* dx1, void* dx2, int csplit, const void* mask1, const void* mask2,
                            const unsigned char* mask1_bits, const unsigned char* mask2_bits,
                            int n, int h, int w, int cin, int cout, int pad_zero, int products, void* stream);
/*      mask1_bits / mask2_bits (optional, each only together with its mask1 / mask2): the relu_mask planes of those activations; the
 *      persistent kernel then brings a tile's mask in by LDS-DMA (4 KB) instead of re-reading the activations' f16 planes (64 KB); the
 *      border fold still reads mask1 / mask2.  products: WSU_PRODUCTS_F16F8 or WSU_PRODUCTS_F16 (above). */

/* ---- K7p: weight / bias gradients on PLANAR operands (csrc/wgrad.hip wgrad_pl_kernel: the split-K MFMA GEMM over pixels of
 *      wsu_conv3x3_bwd_weight with planar staging -- one stored f16 granule + half a residual granule per (pixel, 8 channels), no split arithmetic).
 *      conv: g (cout channels, planar gradient), x1 / x2 (the layer's saved planar inputs, c1 / c2 channels), dw (cout, c1 + c2, 3, 3), db (cout) or
 *      NULL (sum of the decoded gradient values, fixed order).  Transposed conv: x (cin channels at h x w), dy (cout channels, planar gradient at
 *      2h x 2w), dw (cin, cout, 2, 2), db (cout) or NULL.  All channel counts multiples of 64; workspace >= wsu_wgrad_workspace_bytes.  Deterministic.
 *      products: WSU_PRODUCTS_F16F8 or WSU_PRODUCTS_F16 (above; db is then the sum of the gradient's f16 parts). */
int wsu_conv3x3_pl_bwd_weight(const void* g, const void* x1, const void* x2, float* dw, float* db, float* workspace, size_t workspace_bytes,
                              int n, int h, int w, int c1, int c2, int cout, int products, void* stream);
int wsu_convt2x2_pl_bwd_weight(const void* x, const void* dy, float* dw, float* db, float* workspace, size_t workspace_bytes,
                               int n, int h, int w, int cin, int cout, int products, void* stream);

/* ---- K7p: the other backward kernels of the planar training path (csrc/planar.hip, csrc/train_pl.hip; autograd of unet.py:137-189).
 *      wsu_convt2x2_pl_bwd_data: dx[n,i,j,ci] = sum dy[n,2i+a,2j+b,co] w[ci,co,a,b] times the ReLU mask of the layer below (mask: the planar
 *        ACTIVATION the transposed conv consumed, optional); dy (cout channels at 2h x 2w) and dx (cin at h x w) planar gradients; weights from
 *        wsu_convt2x2_pl_pack_dgrad (cin * cout * 16 bytes); cin a multiple of 64, cout of 16; products as above (WSU_PRODUCTS_F16: only the
 *        f16 planes of dy and of the weights travel, six LDS stages instead of three).
 *      wsu_maxpool2x2_pl_bwd: g = (skip_g + routing of dy_pool onto the first maximum of each 2x2 window) * (act > 0); act = the stored activation
 *        the pool consumed (the argmax is recomputed from it); skip_g optional; g may alias skip_g.
 *      wsu_conv1x1_sigmoid_pl_bwd: head backward (unet.py:186-188): x planar activation (c in {16..128}), w (cout <= 4, c), out / dout (N, cout, H, W)
 *        fp32 -> g (planar gradient w.r.t. the pre-activation of the layer that produced x), dw (cout, c), db (cout).
 *      wsu_colsum_pl: per-channel sums of a planar gradient (bias gradient of the transposed conv).
 *      wsu_conv3x3_first_pl_bwd_weight: first layer, single input plane: dw (c, 1, 3, 3), db (c) from the planar gradient g and img (N, 1, H, W).
 *      wsu_conv3x3_first_pl_bwd_weight_planes: the same for cin <= 8 input planes (side-information planes, wsu_pair_batch_planes_f32): x_nchw
 *        (N, cin, H, W) fp32 -> dw (c, cin, 3, 3), db (c) or NULL, dw[co,ci,u,v] = sum over n,i,j of g[n,co,i,j] * x[n,ci,reflect(i+u-1),reflect(j+v-1)];
 *        c a multiple of 16 up to 256 as above.  Planes 0-3 and the bias sum take one pass over g, planes 4-7 a second one (9 * cin + 1 sums
 *        per channel in registers: 8 planes at once do not fit a wave's register file).  Workspace: ..._workspace_bytes(cin, c).
 *      All reductions are two-stage with a fixed order (deterministic).
 *      products (every K7p entry point): with WSU_PRODUCTS_F16 a GRADIENT tensor carries no residual plane -- its producers (the data
 *        gradients, the pool and head backward) write the two f16 planes only and its consumers read only those (plane 2 of such a tensor
 *        is never touched: 2 instead of 3 bytes of traffic per gradient element); a gradient produced with one setting must be consumed
 *        with the same.  Activations are always read whole (the pool's argmax compares the stored values). */
int wsu_convt2x2_pl_pack_dgrad(const float* w_iohw, void* w_packed, int cin, int cout, void* stream);
int wsu_convt2x2_pl_bwd_data(const void* dy, const void* w_packed_dgrad, void* dx, const void* mask,
                             int n, int h, int w, int cin, int cout, int products, void* stream);
int wsu_maxpool2x2_pl_bwd(const void* skip_g, const void* dy_pool, const void* act, void* g, int n, int h, int w, int c, int products, void* stream);
size_t wsu_head_pl_bwd_workspace_bytes(int c, int cout);
int wsu_conv1x1_sigmoid_pl_bwd(const void* x, const float* w, const float* out, const float* dout, void* g, float* dw, float* db,
                               float* workspace, size_t workspace_bytes, int n, int h, int wd, int c, int cout, int products, void* stream);
size_t wsu_chansum_pl_workspace_bytes(int c);
int wsu_colsum_pl(const void* g, float* db, float* workspace, size_t workspace_bytes, int n, int h, int w, int c, int products, void* stream);
int wsu_conv3x3_first_pl_bwd_weight(const void* g, const float* img, float* dw, float* db, float* workspace, size_t workspace_bytes,
                                    int n, int h, int w, int c, int products, void* stream);
size_t wsu_conv3x3_first_pl_bwd_weight_planes_workspace_bytes(int cin, int c);
int wsu_conv3x3_first_pl_bwd_weight_planes(const void* g, const float* x_nchw, float* dw, float* db, float* workspace, size_t workspace_bytes,
                                           int n, int h, int w, int cin, int c, int products, void* stream);
/*      wsu_conv3x3_first_pl_bwd_data (round 4): the INPUT gradient of the planar training path (saliency, src/saliency.py:159-174): g (planar gradient,
 *        c channels, a multiple of 16 up to 256), w_oihw (c, cin <= 8, 3, 3) -> dx (N, cin, H, W) fp32 in g's power-of-two scale (the reflect
 *        adjoint included).  The whole range runs: the kernel's dynamic LDS (cin * 9 * c * 4 bytes, up to 73 728) is raised past 64 KB once. */
int wsu_conv3x3_first_pl_bwd_data(const void* g, const float* w_oihw, float* dx_nchw, int n, int h, int w, int cin, int c, int products, void* stream);

/* ---- K3p / K0p: the other two kernels of the planar (F16F8P) inference path (csrc/planar.hip).
 *      wsu_convt2x2_pl_fwd: nn.ConvTranspose2d(k2, s2) + bias (unet.py:125,130,177,183), x: cin channels at (h, w) planar -> y: cout channels at
 *      (2h, 2w) planar; weights from wsu_convt2x2_pack(mode F16F8); cin a multiple of 32, cout of 64.
 *      wsu_conv3x3_first_pl_fwd: the first layer e11 (unet.py:82,141), x_nchw (N, cin <= 8, H, W) fp32 -> y: cout (multiple of 16) channels planar.
 *      y_format (round 4): WSU_PLANAR_A (the format above) or WSU_PLANAR_Q (K1q; the inputs of the transposed conv stay WSU_PLANAR_A); WSU_PLANAR_H
 *      (K1h, mode 'f16p': the two f16 planes; range_flag only beyond +-65504). */
int wsu_convt2x2_pl_fwd(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w, int cin, int cout,
                        int y_format, unsigned* range_flag, void* stream);
int wsu_conv3x3_first_pl_fwd(const float* x_nchw, const float* w_oihw, const float* bias, void* y, int n, int h, int w, int cin, int cout,
                             int relu, int y_format, unsigned* range_flag, unsigned char* relu_mask_out, void* stream);

/* ---- first layer: conv3x3 reflect on a few input planes given as NCHW fp32 (the model input).
 *      Replaces e11 (unet.py:82,141).  cin 1..8; cout = 8 * 2^k (8, 16, .. 2048) with cin * cout * 36 <= 163 840: the weights live in
 *      the LDS of one compute unit (cin = 8: cout <= 512); more is an argument error that names cin and cout.  w is plain OIHW fp32.
 *      mode BF16 stores y as bf16, each value rounded ONCE from the fp32 sum, to nearest, ties to even (v_cvt_pk_bf16_f32); the other
 *      modes store fp32. */
int wsu_conv3x3_first_fwd(const float* x_nchw, const float* w_oihw, const float* bias, void* y,
                          int n, int h, int w, int cin, int cout, int mode, int relu, void* stream);

/* ---- K2 standalone 2x2/2 max-pool (used when not fused).  A last odd row / column belongs to no window.  pool_idx (optional): the window
 *      position 0..3 of the result, row-major (0,0) (0,1) (1,0) (1,1); of equal values the FIRST wins and the result carries its bits
 *      (+0 and -0 are equal).  A NaN in the window is the result, as in torch / numpy max; its index is that of the window's LAST NaN. */
int wsu_maxpool2x2_fwd(const void* x, void* y, uint8_t* pool_idx, int n, int h, int w, int c, int mode, void* stream);

/* ---- K3: y[n,2i+a,2j+b,co] = bias[co] + sum_ci x[n,i,j,ci] * w[ci,co,a,b]   (unet.py:177,183) */
int wsu_convt2x2_fwd(const void* x, const void* w_packed, const float* bias, void* y,
                     int n, int h, int w, int cin, int cout, int mode, void* stream);

/* ---- K5: out[n,co,y,x] = sigmoid(b[co] + sum_c x[n,y,x,c] * w[co,c])   (unet.py:189).
 *      w: (cout, c) fp32 (outconv.weight squeezed), out: NCHW fp32; logit: optional NCHW fp32 pre-sigmoid. */
int wsu_conv1x1_sigmoid_fwd(const void* x, const float* w, const float* bias, float* out, float* logit,
                            int n, int h, int w_, int c, int cout, int mode, void* stream);

/* ---- K6: UniformDropout (unet.py:32-42) on plane `channel` of an NCHW fp32 tensor, out of place:
 *      y = x*mask + KB(x)*(1-mask).  mask: (N,1,H,W) fp32 keep-mask, or NULL to draw it from a
 *      counter-based hash of (seed, element index) with keep probability keep_prob. */
int wsu_uniform_dropout_fwd(const float* x, float* y, const float* mask, float* mask_out,
                            int n, int c, int h, int w, int channel,
                            float keep_prob, uint64_t seed, void* stream);

/* ---- K10: per-image WS residual statistics (src/unet/evaluate.py:125-132).
 *      x_u8: (N,H,W) cover/stego pixels; y01: (N,H,W) fp32 network output in [0,1].
 *      Over the interior [1:-1,1:-1]:  xhat = y*255;  beta_hat = mean((x - (x^1)) * (x - xhat));
 *      l1 = mean|x - xhat|.  Deterministic (fixed-order fp64 tree). */
int wsu_ws_residual_stats(const uint8_t* x_u8, const float* y01, float* beta_hat, float* l1,
                          int n, int h, int w, void* stream);

/* ---- K11: weighted-stego payload estimate of the predictor's caller, src/ws/estimate.py:55-136 `attack`, batched.
 *      x_u8: (N,H,W) DEVICE pixels of the analysed plane.  The pixel prediction is either
 *        x_hat (DEVICE fp32): hat_full=1 -> (N,H,W), interior read at [r][c] (a network output; hat_scale = 255),
 *                             hat_full=0 -> (N,H-2,W-2) (what `pixel_estimator(x)` returns; hat_scale = 1), or
 *        pixel_filter (HOST, 9 floats K[a][b] of the reference's (3,3,1) kernel array, filters/evaluate.py:30-50,136-141):
 *                             x_hat = convolve(x/255, K, 'valid')*255 evaluated inside the kernel.
 *      mean_filter (HOST, 9 floats, same layout; NAMED_FILTERS['AVG'] by default, estimate.py:60,93-95) feeds the local
 *      variance for weighted = 1 (1/(5+var)) or -1 (5+var); weighted = 0 -> uniform weights (:97-110).
 *      correct_bias (:126-128) needs x_bias = pixel_estimator(x_bar - x) in x_hat's layout; with pixel_filter the kernel applies the
 *      filter to (x_bar - x)/255 itself and x_bias is not read.
 *      beta_hat: (N) fp32, clipped at 0 (:121) before the bias correction; NaN stays NaN, as np.clip: a NaN in an interior prediction
 *      (or, with correct_bias, in x_bias) gives a NaN estimate, not 0.  sums: optional (N,3) fp64 {sum w, sum w*s*(x-x_hat),
 *      sum w*s*x_bias}. */
size_t wsu_ws_attack_workspace_bytes(int n);
int wsu_ws_attack(const uint8_t* x_u8, const float* x_hat, const float* x_bias, const float* pixel_filter, const float* mean_filter,
                  int hat_full, float hat_scale, int weighted, int correct_bias, float* beta_hat, double* sums,
                  void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream);
/* K11 with one in-kernel filter per image: pixel_filters is DEVICE (N,9) fp32, row i = K[a][b] of image i's filter in pixel_filter's
 * layout.  The same kernels as wsu_ws_attack (image i's numbers are those of wsu_ws_attack on image i alone with pixel_filter = row i);
 * correct_bias uses the in-kernel filter on x_bar - x.  Workspace as for wsu_ws_attack. */
int wsu_ws_attack_taps(const uint8_t* x_u8, const float* pixel_filters, const float* mean_filter, int weighted, int correct_bias,
                       float* beta_hat, double* sums, void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream);

/* ---- K27: the WS changepoint for sequentially placed payloads (Ker, SPIE 2007; not part of the reference).  Inputs as K11's: x_u8 (N,H,W)
 *      DEVICE pixels and exactly ONE prediction source:
 *        x_hat (DEVICE fp32; hat_full = 1: (N,H,W) frames, hat_full = 0: (N,H-2,W-2) interiors; multiplied by hat_scale),
 *        pixel_filter (HOST, 9 floats K[a][b], evaluated in the kernel as in K11), or
 *        pixel_filters (DEVICE (N,9) fp32, one such filter per image, as wsu_ws_attack_taps).
 *      mean_filter (HOST, 9 floats) feeds the local variance for weighted = 1; weighted = 0 -> unit weights.  weighted = -1 and the bias
 *      correction are not defined for this statistic: weighted = -1 is an argument error (checked before any HIP call).
 *      The path visits the interior pixels [1:-1, 1:-1] row by row, left to right within a row; order = 0: rows from the top,
 *      order = 1: rows from the bottom.  M = (H-2)(W-2) positions, M <= 2^27.  Per interior pixel, in float32 with K11's operation
 *      sequence and nothing contracted (s = x - x_bar = +-1, res = x - x_hat, var as in K11):
 *        r = s * res;   d = r - 0.25f;   t = wgt * d,   wgt = 1.0f or 1.0f / (5.0f + var);
 *        q = 0 where t is NaN, otherwise llrint((double)min(max(t, -4096), 4096) * 2^24)        (round to nearest even, int64).
 *      Outputs per image, DEVICE int64 [N], with T(j) = q_1 + .. + q_j along the path and T(0) = 0:
 *        k     = the smallest k in 0..M at which T(k) is maximal (the empty prefix takes part; among equal maxima the first);
 *        t_max = T(k);   t_all = T(M);
 *        curve = optional DEVICE int64 (N,H-2) (may be null): T at the end of every interior row, in path order.
 *      All sums are exact integers (|q| <= 2^36), so the results do not depend on how the work is split, on the batch or on the run.
 *      Image i's outputs are those of a call on image i alone.  workspace: DEVICE, 8-byte aligned,
 *      wsu_ws_sequential_workspace_bytes(n, h) = 24 (H-2) bytes per image (0 for bad arguments); fully written before it is read.
 *      n <= 65535, h, w >= 3.  The payload estimate from k is host arithmetic (ws_unet_amd/ws/sequential.py). */
size_t wsu_ws_sequential_workspace_bytes(int n, int h);
int wsu_ws_sequential(const uint8_t* x_u8, const float* x_hat, const float* pixel_filter, const float* pixel_filters, const float* mean_filter,
                      int hat_full, float hat_scale, int weighted, int order, long long* k, long long* t_max, long long* t_all,
                      long long* curve, void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream);

/* ---- K33: the WS changepoint along a path given per image, for payloads placed in the order of an adaptivity criterion that the attacker
 *      recomputes from the stego image (Schoettle, Korff, Boehme, WIFS 2012; not part of the reference).  x_u8, the ONE prediction source
 *      (x_hat with hat_full and hat_scale / pixel_filter HOST / pixel_filters DEVICE (N,9)), mean_filter and weighted in {0, 1} as K27's.
 *      tau = flip rate / 2 with 0 < tau <= 0.5: a used pixel is assumed flipped with probability 2 tau (1/4: a real message, K27's term;
 *      1/2: every used pixel flipped, as HILLR does).  Per interior pixel, in float32 with K11's operation sequence, nothing contracted:
 *        r = s * res;   d = r - tau;   t = wgt * d;   q = K27's fixed-point form of t (int64, 2^24 units, 0 for NaN).
 *      path: DEVICE int32 (N,M), M = (H-2)(W-2) <= 2^27: image i's interior raster indices (r-1)(W-2) + (c-1) in the order the path
 *      visits them, meant to be a permutation of 0..M-1.  An entry outside 0..M-1 is never dereferenced and contributes a zero term.
 *      Outputs per image, DEVICE int64 [N], with T(j) = q[path[0]] + .. + q[path[j-1]] and T(0) = 0:
 *        k = the smallest k in 0..M at which T(k) is maximal;   t_max = T(k);   t_all = T(M).
 *      Exact integer sums and no atomics: the results depend on neither the split of the work, the batch nor the run.
 *      wsu_ws_ordered_terms writes the term plane `terms` (DEVICE int64 (N,M), 8-byte aligned, raster order); wsu_ws_ordered_fold reduces
 *      such a plane along `path` (workspace: wsu_ws_ordered_fold_workspace_bytes: 24 bytes per 2048 path positions of an image);
 *      wsu_ws_ordered is the two in one call with the term plane in its workspace (wsu_ws_ordered_workspace_bytes = 8 M bytes per image
 *      plus the fold's).  Workspaces: DEVICE, 8-byte aligned, fully written before they are read; the size functions give 0 for bad
 *      arguments.  n <= 65535, h, w >= 3. */
size_t wsu_ws_ordered_workspace_bytes(int n, int h, int w);
size_t wsu_ws_ordered_fold_workspace_bytes(int n, int h, int w);
int wsu_ws_ordered_terms(const uint8_t* x_u8, const float* x_hat, const float* pixel_filter, const float* pixel_filters,
                         const float* mean_filter, int hat_full, float hat_scale, int weighted, float tau, long long* terms, int n, int h, int w,
                         void* stream);
int wsu_ws_ordered_fold(const long long* terms, const int* path, long long* k, long long* t_max, long long* t_all, void* workspace,
                        size_t workspace_bytes, int n, int h, int w, void* stream);
int wsu_ws_ordered(const uint8_t* x_u8, const float* x_hat, const float* pixel_filter, const float* pixel_filters, const float* mean_filter,
                   int hat_full, float hat_scale, int weighted, float tau, const int* path, long long* k, long long* t_max, long long* t_all,
                   void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream);

/* ---- K29: per-pixel sums of the WS residual terms across images (Ker, "Locating steganographic payload via WS residuals", MM&Sec 2008;
 *      not part of the reference).  Inputs as K27's: x_u8 (N,H,W) DEVICE pixels, exactly ONE of x_hat (hat_full, hat_scale) /
 *      pixel_filter (HOST) / pixel_filters (DEVICE (N,9)), mean_filter (HOST) for weighted = 1; weighted = -1 is an argument error.
 *      num, den: DEVICE int64 (H-2,W-2), 8-byte aligned.  The call ADDS to them (the caller zeroes them before the first batch): per
 *      interior pixel and image, in float32 with K11's operation sequence and nothing contracted,
 *        r = s * res;   t = wgt * r,   wgt = 1.0f or 1.0f / (5.0f + var);
 *        where t is NaN nothing is added, otherwise
 *        num += llrint((double)min(max(t, -4096), 4096) * 2^24);      den += llrint((double)wgt * 2^32)          (round to nearest even).
 *      The weighted mean of r at a pixel is (num / 2^24) / (den / 2^32) = num * 256 / den: about 1/2 where every image carries payload,
 *      about 0 where none does.  All sums are exact integers, so the accumulators depend on neither the split of the images into calls,
 *      their order, nor `parts`: the number of workgroups that share a pixel tile's images (1: one owner per pixel and plain stores;
 *      more: 64-bit integer atomics; 0: as many as bring the grid to about 4096 workgroups, the fastest measured).  After at most 65536 images in total |num| < 2^53 and, for the
 *      weights of a non-negative mean filter (wgt <= 1), den < 2^53.  n <= 65535, h, w >= 3, (H-2)(W-2) <= 2^31. */
int wsu_ws_residual_accumulate(const uint8_t* x_u8, const float* x_hat, const float* pixel_filter, const float* pixel_filters,
                               const float* mean_filter, int hat_full, float hat_scale, int weighted, int parts, long long* num, long long* den,
                               int n, int h, int w, void* stream);

/* ---- K35: the stego-key search over K29's sums (Fridrich, Goljan, Soukal, "Searching for the stego-key", SPIE 5306, 2004; not part of
 *      the reference): masked sums of two int64 planes under many Philox keys.  num, den: DEVICE int64, `count` entries in FRAME layout
 *      (entry i = the pixel of linear index i, K30's i; the caller zero-fills the frame's border), 1 <= count <= 2^34.  The K candidate
 *      keys, 1 <= K <= 2^31-1, are EITHER `keys`, a DEVICE array of K 64-bit patterns (key_range = 0), OR the range key_first + j,
 *      j = 0..K-1, wrapping mod 2^64 (keys = NULL, key_range = 1).  thr in 0..2^32.  Pixel i is SELECTED under a key iff word i % 4 of
 *      Philox4x32-10 on counter (i / 4, 0, 0, 0) under the key (low, high word) is below thr, compared in 64 bits: K30's rule, so the
 *      selection is wsu_lsbr_key_mask(key, thr) and thresholds nest (a smaller thr selects a subset).  snum, sden: DEVICE int64 [K],
 *      zeroed on the stream by the call:
 *        snum[j] = sum of num[i] over the selected i < count;   sden[j] = the same sum of den[i];
 *      two's-complement int64 addition, wrapping, which is the definition: the result depends on neither the grid, the order of the adds
 *      nor `parts`, the number of workgroups that share a key's pixels (1: one owner per key and plain stores; more: 64-bit integer
 *      atomics; 0: as many as bring the grid to about 1024 workgroups, at least 64 quads of pixels each).  All arrays 8-byte aligned;
 *      every argument is checked before any HIP call. */
int wsu_ws_key_search(const long long* num, const long long* den, long long count, const uint64_t* keys, uint64_t key_first, int key_range,
                      int k, uint64_t thr, int parts, long long* snum, long long* sden, void* stream);

/* ---- K24: moments of the least-squares 3x3 pixel predictor.  x_u8: (N,H,W) DEVICE pixels.  At every interior pixel (r,c), with
 *      xab = x[r-1+a][c-1+b], v = [x00 x01 x02 x12 x22 x21 x20 x10 x11] (the ring order of the flattened 8-tap filters,
 *      _defs/filters.py:57-67, centre last).  moments: DEVICE (N,45) uint64, zeroed on the stream by this call:
 *      moments[i][.] = sum over image i's interior of v_p * v_q, 0 <= p <= q <= 8, row-major upper triangle -- the Gram matrix X^T X of the
 *      neighbours, X^T y (q = 8) and y^T y (last).  Exact integers (at most 255^2 (H-2)(W-2) each), the same bits on every run. */
int wsu_ols_moments(const uint8_t* x_u8, unsigned long long* moments, int n, int h, int w, void* stream);

/* ---- K56: moments of the least-squares 5x5 pixel predictor.  x_u8: (N,H,W) DEVICE pixels, H, W >= 5 (else an argument error, checked
 *      before any HIP call), N <= 65535.  The sums run over every pixel (r,c) with a full 5x5 window, 2 <= r <= H-3, 2 <= c <= W-3.  The 25
 *      variables: v[0..23] = the 24 neighbours x[r-2+a][c-2+b] in raster order of (a,b), the centre skipped; v[24] = the centre.
 *      moments: DEVICE (N,325) uint64, zeroed on the stream by this call: moments[i][.] = sum of v_p * v_q, 0 <= p <= q <= 24, row-major
 *      upper triangle -- K24's layout with 25 variables in place of 9.  Exact integers (at most 255^2 (H-4)(W-4) each), the same bits on
 *      every run, every batch and every launch split. */
int wsu_ols_moments5(const uint8_t* x_u8, unsigned long long* moments, int n, int h, int w, void* stream);

/* ---- K57: the 5x5 linear prediction as full frames.  x_u8: (N,H,W) DEVICE pixels, H, W >= 3, N <= 65535.  taps: DEVICE fp32, (N,24) with
 *      per_image != 0, else (24) for every image; taps[k] weighs v[k] of K56.  x_hat: DEVICE fp32 (N,H,W) in pixel units (hat_scale = 1
 *      for the WS statistics); x_bias: the same shape, or null.  float32 with plain operators, one rounding each, nothing fused;
 *      q(u) = (float)u / 255.0f (K11's quotient), qb(u) = (u & 1) ? -q(1) : q(1).  Per pixel:
 *        frame border (r or c the first or last)       x_hat = 0, x_bias = 0 (no statistic reads them; the plane is fully written)
 *        ring 1 (r in {1, H-2} or c in {1, W-2})       KB's 3x3 taps as K11 evaluates an in-kernel filter: acc = 0; for j = 8 .. 0:
 *                                                      acc = acc + kb[j] * q[j]; x_hat = acc * 255.0f (the 5x5 window leaves the image;
 *                                                      it is not mirrored, which would let a pixel predict itself)
 *        elsewhere                                     acc = 0; for k = 23 .. 0: acc = acc + taps[k] * q(v[k]); x_hat = acc * 255.0f
 *      x_bias is the same sequence with qb in place of q.  With KB's taps embedded in the 24, K11 on these planes with hat_scale = 1 has
 *      the bits of K11 with pixel_filter = KB.  Every argument is checked before any HIP call. */
int wsu_predict5x5(const uint8_t* x_u8, const float* taps, int per_image, float* x_hat, float* x_bias, int n, int h, int w, void* stream);

/* ---- K25: the trace-set table of Sample Pairs Analysis (Dumitrescu, Wu, Wang 2003).  x_u8: (N,H,W) DEVICE pixels, any H, W >= 1.  The
 *      pairs of an image are all horizontally adjacent (x[r][c], x[r][c+1]) and all vertically adjacent (x[r][c], x[r+1][c]):
 *      H (W-1) + (H-1) W of them.  For a pair (u,v): d = |u - v|, m = d >> 1, hi = max(u,v).  tables: DEVICE (N,3,128) uint64, zeroed on the
 *      stream by this call:
 *        tables[i][0][m] (E) = pairs with d even (d = 2m);
 *        tables[i][1][m] (X) = pairs with d odd and hi even (their halves u >> 1, v >> 1 differ by m + 1);
 *        tables[i][2][m] (Y) = pairs with d odd and hi odd (their halves differ by m).
 *      With C_m = pairs whose halves differ by m and D_n = pairs with d = n: D_2m = E[m], D_2m+1 = X[m] + Y[m],
 *      C_m = E[m] + Y[m] + X[m-1] (X[-1] = 0).  An image without a pair has an all-zero table.  Exact integers, the same bits on every run. */
int wsu_spa_tables(const uint8_t* x_u8, unsigned long long* tables, int n, int h, int w, void* stream);

/* ---- K26: the regular / singular group counts of RS analysis (Fridrich, Goljan, Du 2001).  x_u8: (N,H,W) DEVICE pixels, any H, W >= 1.
 *      Groups are the non-overlapping runs of 4 consecutive pixels of every row from column 0: G = x[r][4g .. 4g+3], g < W / 4 (the trailing
 *      W % 4 columns are ignored; W < 4 gives zeros).  f(G) = |g1-g0| + |g2-g1| + |g3-g2| in integers; F1(v) = v ^ 1;
 *      F-1(v) = ((v + 1) ^ 1) - 1 in integers (0 -> -1, 255 -> 256, not clamped).  Mask M = (0,1,1,0): G_M applies F1 to g1 and g2,
 *      G_-M applies F-1 to g1 and g2.  counts: DEVICE (N,8) uint64, zeroed on the stream by this call, per image in this order:
 *        R_M = #{f(G_M) > f(G)}, S_M = #{f(G_M) < f(G)}, R_-M = #{f(G_-M) > f(G)}, S_-M = #{f(G_-M) < f(G)},
 *      then the same four on the plane with every LSB flipped (G ^ 1 element-wise in the place of G).  Exact integers. */
int wsu_rs_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream);

/* ---- K58: the histograms of the segments of a path (the chi-square attack of Westfeld, Pfitzmann, IH 1999, along the file order; not part
 *      of the reference).  x_u8: (N,H,W) DEVICE pixels, any H, W >= 1 with H W < 2^32.  segments = S in 1..4096.  The path position of pixel
 *      (r,c) is t = r W + c for order 0 ('rows') and t = (H-1-r) W + c for order 1 ('rows_up'), as in K27 / K28; the pixel belongs to
 *      segment s = floor(t S / (H W)), the product in 64 bits, so segment s holds the positions ceil(s H W / S) .. ceil((s+1) H W / S) - 1
 *      (none of them where S > H W leaves it empty).  table: DEVICE (N,S,256) uint64, zeroed on the stream by this call:
 *        table[i][s][v] = pixels of image i in segment s with the value v.
 *      S = 1 is the plain histogram; a prefix histogram is a cumulative sum over s, which the caller takes.  Exact integers, the same bits
 *      on every run.  n in 1..65535; every argument is checked before any HIP call. */
int wsu_hist_segments(const uint8_t* x_u8, unsigned long long* table, int n, int h, int w, int segments, int order, void* stream);

/* ---- K59: the horizontal adjacency histogram (Ker, IEEE SPL 12(6), 2005; not part of the reference).  x_u8: (N,H,W) DEVICE pixels, any
 *      H, W >= 1.  table: DEVICE (N,256,256) uint64, zeroed on the stream by this call:
 *        table[i][u][v] = #{(r,c): c + 1 < W, x[r][c] = u, x[r][c+1] = v},
 *      H (W - 1) pairs per image; W = 1 gives an all-zero table.  Exact integers, the same bits on every run.  n in 1..65535; every
 *      argument is checked before any HIP call. */
int wsu_adjacency_hist(const uint8_t* x_u8, unsigned long long* table, int n, int h, int w, void* stream);

/* ---- K60: the 2 x 2 block mean, rounded down (Ker's calibration image; not part of the reference).  x_u8: (N,H,W) DEVICE pixels, H, W >= 2.
 *      y_u8: DEVICE (N, H/2, W/2) uint8 in integer division (an odd last row or column is dropped):
 *        y[i][r][c] = (x[i][2r][2c] + x[i][2r][2c+1] + x[i][2r+1][2c] + x[i][2r+1][2c+1]) >> 2.
 *      n in 1..65535; every argument is checked before any HIP call. */
int wsu_downsample2x2(const uint8_t* x_u8, uint8_t* y_u8, int n, int h, int w, void* stream);

/* ---- K36: the co-occurrence counts of the subtractive pixel adjacency matrix (SPAM; Pevny, Bas, Fridrich, IEEE TIFS 5(2), 2010; not part
 *      of the reference).  x_u8: (N,H,W) DEVICE pixels, any H, W >= 1.  order in {1,2}; T in 1..8 at order 1, 1..4 at order 2; B = 2T + 1.
 *      A direction is a step (dr,dc); the four counted ones, in this index order: 0 (0,+1), 1 (+1,0), 2 (+1,+1), 3 (+1,-1).  In integers
 *        D_k(r,c) = clip(x[r + k dr][c + k dc] - x[r + (k+1) dr][c + (k+1) dc], -T, T),   k = 0 .. order
 *      (a difference beyond +-T is clipped into the border bins, not dropped).  A position (r,c) counts for a direction when all order + 2
 *      pixels x[r + k dr][c + k dc], k = 0 .. order + 1, lie in the image; it adds 1 to bin sum_k (D_k + T) B^(order - k) (D_0 is the most
 *      significant digit).  counts: DEVICE (N, 4, B^(order+1)) uint64, zeroed on the stream by this call.  An image too small for a direction
 *      has zero counts there; otherwise counts[i][d] sums to H (W - order - 1), (H - order - 1) W and, for both diagonals,
 *      (H - order - 1)(W - order - 1).  The counts of the opposite step are C_opp[d_0, .., d_order] = C[-d_order, .., -d_0] (the same runs
 *      walked backwards), so they are not counted.  order 2, T 3: 343 bins per direction (SPAM-686); order 1, T 4: 81 (SPAM-162).  Exact
 *      integers, the same bits on every run.  n in 1..65535; every argument is checked before any HIP call. */
int wsu_spam_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, int order, int T, void* stream);

/* ---- K49: the co-occurrence counts of the linear ("spam"-type) submodels of the spatial rich model (SRM; Fridrich, Kodovsky, IEEE TIFS
 *      7(3), 2012; not part of the reference; only these submodels, the min/max ones are K50's; not compared with the authors' extractor).
 *      x_u8: (N,H,W) DEVICE pixels X[r][c], any H, W >= 1.  All arithmetic is exact integer arithmetic.  Eight residuals per pixel:
 *        S1   h: X[r][c+1] - X[r][c]                                  v: X[r+1][c] - X[r][c]                      q2 = 2, 4
 *        S2   h: X[r][c-1] - 2 X[r][c] + X[r][c+1]                    v: the same down a column                   q2 = 4, 6, 8
 *        S3   h: X[r][c-1] - 3 X[r][c] + 3 X[r][c+1] - X[r][c+2]      v: the same down a column                   q2 = 6, 9, 12
 *        S3x3 n: [[-1,2,-1],[2,-4,2],[-1,2,-1]] centred on (r,c)                                                  q2 = 8, 12, 16
 *        S5x5 n: [[-1,2,-2,2,-1],[2,-6,8,-6,2],[-2,8,-12,8,-2],[2,-6,8,-6,2],[-1,2,-2,2,-1]] centred on (r,c)    q2 = 24, 36, 48
 *      The digit of a residual R at the step q = q2 / 2 is d = sign(R) min((4|R| + q2) / (2 q2), 2) in integer division: R / q rounded
 *      with halves away from zero, then cut to -2 .. 2.  A table takes one residual at one q and scans it h (the four digits at columns
 *      c .. c+3 of a row) or v (at rows r .. r+3 of a column); a run counts when every pixel that its four residuals read lies in the image
 *      (no padding) and adds 1 to bin sum_k (d_k + 2) 5^(3-k), the leftmost or topmost digit the most significant: 625 bins, centre 312.
 *      The 44 tables in order: for class in S1, S2, S3, S3x3, S5x5; for q ascending; for residual in (h, v) or the one n; for scan in
 *      (h, v): S1 is 0..7, S2 8..19, S3 20..31, S3x3 32..37, S5x5 38..43.  A table sums to max(H - a, 0) max(W - b, 0) with (a,b) =
 *        S1: hh (0,4) hv (3,1) vh (1,3) vv (4,0);  S2: (0,5) (3,2) (2,3) (5,0);  S3: (0,6) (3,3) (3,3) (6,0);  S3x3: nh (2,5) nv (5,2);
 *        S5x5: nh (4,7) nv (7,4).
 *      counts: DEVICE (N, 44, 625) uint64, zeroed on the stream by this call.  Exact integers, the same bits on every run.  n in
 *      1..65535; every argument is checked before any HIP call. */
int wsu_srm_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream);

/* ---- K50: the co-occurrence counts of the min/max submodels of the spatial rich model built on the directional first-, second- and
 *      third-order residuals (the paper's minmax22h/v, minmax24, minmax34h/v of the 1st and 3rd order and minmax21, 41, 32, 24h/v of the
 *      2nd; stated as remembered, not compared with the authors' extractor; the other 1st/3rd-order submodels are K54's and the EDGE3x3 and
 *      EDGE5x5 classes K55's; by the paper's naming rule the set WENS below is its minmax41 and its minmax24 is K54's).  x_u8, the digit d(R, q2), a run (four digits at columns
 *      c..c+3, scan h, or rows r..r+3, scan v) and its bin are K49's.  The directional residuals at a pixel (r,c):
 *        S1  q2 = 2, 4       E = X[r][c+1] - X[r][c]   W = X[r][c-1] - X[r][c]   S = X[r+1][c] - X[r][c]   N = X[r-1][c] - X[r][c]
 *        S2  q2 = 4, 6, 8    h = X[r][c-1] - 2 X[r][c] + X[r][c+1]               v = X[r-1][c] - 2 X[r][c] + X[r+1][c]
 *                            d = X[r-1][c-1] - 2 X[r][c] + X[r+1][c+1]           m = X[r-1][c+1] - 2 X[r][c] + X[r+1][c-1]
 *        S3  q2 = 6, 9, 12   E = X[r][c-1] - 3 X[r][c] + 3 X[r][c+1] - X[r][c+2]   W = X[r][c+1] - 3 X[r][c] + 3 X[r][c-1] - X[r][c-2]
 *                            S = X[r-1][c] - 3 X[r][c] + 3 X[r+1][c] - X[r+2][c]   N = X[r+1][c] - 3 X[r][c] + 3 X[r-1][c] - X[r-2][c]
 *      A set is a list of residuals of one class taken at the same pixel; its digits are lo = the minimum and hi = the maximum of its
 *      members' digits (the digit is monotone: the digit of the smallest / largest residual).  The sets in order:
 *        S1 and S3: WE, NS, WENS, WNE, ESW, SWN, NES          S2: hv, hvdm, hvd, hvm, hd, hm, vd, vm
 *      One table per (class, q2, set, scan), and TWO updates per run: the run of four lo digits adds 1 at its bin, the run of four hi
 *      digits adds 1 at the bin of the NEGATED digits, 624 - bin (the rich model's min/max symmetrisation, done at the source).  A run
 *      counts when every pixel that any member of the set reads at any of its four positions lies in the image (no padding).  With
 *      (u, dn, l, rt) how far the set's taps reach up, down, left and right, a scan-h table sums to 2 max(H - u - dn, 0) max(W - l - rt - 3, 0)
 *      and a scan-v table to 2 max(H - u - dn - 3, 0) max(W - l - rt, 0):
 *        S1: WE (0,0,1,1) NS (1,1,0,0) WENS (1,1,1,1) WNE (1,0,1,1) ESW (0,1,1,1) SWN (1,1,1,0) NES (1,1,0,1);   S2: every set (1,1,1,1);
 *        S3: WE (0,0,2,2) NS (2,2,0,0) WENS (2,2,2,2) WNE (2,1,2,2) ESW (1,2,2,2) SWN (2,2,2,1) NES (2,2,1,2).
 *      The 118 tables in order: for class in S1, S2, S3; for q2 ascending; for set as listed; for scan in (h, v): S1 is 0..27, S2 28..75,
 *      S3 76..117.  counts: DEVICE (N, 118, 625) uint64, zeroed on the stream by this call; an image too small for a table leaves it zero.
 *      Exact integers, the same bits on every run, independent of the batch split.  n in 1..65535; every argument is checked before any
 *      HIP call. */
int wsu_srm_minmax_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream);

/* ---- K54: the co-occurrence counts of the remaining first- and third-order min/max submodels of the spatial rich model, over "fans" of
 *      the eight directional residuals (stated as remembered, not compared with the authors' extractor; by the rich model's rule
 *      minmax<number of residuals><symmetry index> the sets below are its minmax24, 34, 48h/v and 54, and K50's set WENS is its minmax41:
 *      DESIGN.md 4-srmfull has the mapping).  x_u8, the digit d(R, q2), lo / hi, a run, its bin, the two updates per run (the lo digits at
 *      their bin, the negated hi digits at theirs) and the condition for a run to count are K50's.  The directions counter-clockwise and
 *      their steps d = (dr, dc):  E (0,1)  NE (-1,1)  N (-1,0)  NW (-1,-1)  W (0,-1)  SW (1,-1)  S (1,0)  SE (1,1);  the residual of a
 *      direction at the pixel p:
 *        S1  q2 = 2, 4       X[p+d] - X[p]
 *        S3  q2 = 6, 9, 12   X[p-d] - 3 X[p] + 3 X[p+d] - X[p+2d]                 (E, W, S, N are K50's)
 *      The 20 sets in order, named by their members:
 *        pairs (perpendicular)                    E+N  N+W  W+S  S+E
 *        3-fans centred on a diagonal             E+NE+N  N+NW+W  W+SW+S  S+SE+E
 *        4-fans with N or S and both neighbours   E+NE+N+NW  NE+N+NW+W  W+SW+S+SE  SW+S+SE+E          ("vertical")
 *        4-fans with E or W and both neighbours   N+NW+W+SW  NW+W+SW+S  S+SE+E+NE  SE+E+NE+N          ("horizontal")
 *        5-fans centred on a diagonal             SE+E+NE+N+NW  NE+N+NW+W+SW  NW+W+SW+S+SE  SW+S+SE+E+NE
 *      A first-order residual reaches 1 pixel along its direction, a third-order one 2 along it and 1 against it; with (u, dn, l, rt) the
 *      largest reach of a set's members up, down, left and right, a scan-h table sums to 2 max(H - u - dn, 0) max(W - l - rt - 3, 0) and a
 *      scan-v table to 2 max(H - u - dn - 3, 0) max(W - l - rt, 0).  The 200 tables in order: for (class, q2) in S1 2, S1 4, S3 6, S3 9,
 *      S3 12; for set as listed; for scan in (h, v).  counts: DEVICE (N, 200, 625) uint64, zeroed on the stream by this call; an image too
 *      small for a table leaves it zero.  Exact integers, the same bits on every run, independent of the batch split.  n in 1..65535;
 *      every argument is checked before any HIP call. */
int wsu_srm_fan_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream);

/* ---- K55: the co-occurrence counts of the EDGE3x3 and EDGE5x5 classes of the spatial rich model (stated as remembered, not compared with
 *      the authors' extractor).  Everything but the residuals and the sets is K50's.  Four residuals per class at a pixel (r,c):
 *        E3  q2 = 8, 12, 16     U = -X[r-1][c-1] + 2 X[r-1][c] - X[r-1][c+1] + 2 X[r][c-1] - 4 X[r][c] + 2 X[r][c+1]: the top two rows of
 *                               K49's 3x3 kernel with the centre on its -4
 *        E5  q2 = 24, 36, 48    U = the top three rows of K49's 5x5 kernel with the centre on its -12 (rows r-2 .. r, columns c-2 .. c+2)
 *        D = U flipped top to bottom, L = U transposed, R = L mirrored left to right.
 *      The eleven sets in order: U, D, L, R, UL, UR, DL, DR, UD, LR, UDLR.  A singleton has lo = hi = its digit and takes the same two
 *      updates: its table is the residual's plain co-occurrence table plus the same with every digit negated.  With k = 1 (E3) or 2 (E5)
 *      the reach (u, dn, l, rt) is U (k,0,k,k), D (0,k,k,k), L (k,k,k,0), R (k,k,0,k) and (k,k,k,k) for every other set; the sums are K54's.
 *      The 132 tables in order: for (class, q2) in E3 8, 12, 16, E5 24, 36, 48; for set as listed; for scan in (h, v).  counts: DEVICE
 *      (N, 132, 625) uint64, zeroed on the stream by this call.  Exact integers, the same bits on every run, independent of the batch
 *      split.  n in 1..65535; every argument is checked before any HIP call. */
int wsu_srm_edge_counts(const uint8_t* x_u8, unsigned long long* counts, int n, int h, int w, void* stream);

/* ---- K52: the weighted co-occurrence sums of K49's tables, the integer half of the selection-channel-aware rich model (maxSRM: Denemark,
 *      Sedighi, Holub, Cogranne, Fridrich, WIFS 2014; not part of the reference; the h and v scans of the linear submodels only, not the
 *      oblique d2 scan of maxSRMd2 and not the min/max submodels; not compared with the authors' extractor).  x_u8, the residuals, the digit,
 *      a run, its bin, the condition for a run to count and the order of the 44 tables are K49's, unchanged.  weights_u16: DEVICE uint16
 *      (N,H,W), any plane of that shape (K51 makes the sender's change probabilities).  The position of a residual is the (r,c) of K49's
 *      list (the pixel whose coefficient is written at X[r][c]; the centre of S3x3 and S5x5), whatever pixels it reads.  A counted run
 *      whose four residuals sit at (r, c+k), scan h, or (r+k, c), scan v, k = 0..3, adds  max_k weights[r][c+k]  or  max_k weights[r+k][c]
 *      to its bin instead of 1.  With weights all 1 the sums are K49's counts.  sums: DEVICE (N, 44, 625) uint64, zeroed on the stream by
 *      this call.  Exact integers, the same bits on every run and in every batch.  n in 1..65535; every argument is checked before any
 *      HIP call. */
int wsu_srm_weighted_counts(const uint8_t* x_u8, const uint16_t* weights_u16, unsigned long long* sums, int n, int h, int w, void* stream);

/* ---- K53: the bootstrap-weighted scatter matrices of the base learners of the FLD ensemble (Kodovsky, Fridrich, Holub, "Ensemble
 *      classifiers for steganalysis of digital media", IEEE TIFS 7(2), 2012; not part of the reference; ws_unet_amd.ensemble fits it).
 *      zt: DEVICE (d, n_rows) float64, FEATURE-major (a feature is one contiguous row), finite.  idx: DEVICE (L, d_sub) int32, every entry
 *      in [0, d): THE CALLER CHECKS THAT, this entry does not read idx on the host (ops.subspace_gram checks it with one reduction on
 *      the device); any order, repeats allowed.  weights: DEVICE (L, n_rows) int32 >= 0, the bootstrap multiplicity of row i in learner l.
 *        G[l][a][b] = sum_i weights[l][i] * zt[idx[l][a]][i] * zt[idx[l][b]][i]         G: DEVICE (L, d_sub, d_sub) float64
 *      Products and sums are float64 on v_mfma_f64_16x16x4_f64.  The weight is multiplied into the a-operand where it is staged, so a
 *      term is fl(fl(w z_a) z_b + partial sum): at most one rounding more than a plain product sum, and
 *      |G - exact| <= (n_rows + 2) 2^-53 sum_i w_i |z_a z_b|.  Only entries with a >= b are computed; each is written at [a][b] and at
 *      [b][a], so G[l] is symmetric bit for bit.  An entry is accumulated in one accumulator over i ascending in steps of 4: its bits
 *      depend on n_rows and the data alone, not on L, on the other learners of the launch or on how a caller splits L.  Tails of n_rows
 *      and d_sub are zero-filled operands: nothing is read outside zt's rows.  Every entry of G is written; nothing needs zeroing.
 *      L in 1..65535, d_sub in 1..2^20; null pointers and non-positive sizes return -1 before any HIP call. */
int wsu_subspace_gram_f64(const double* zt, const int32_t* idx, const int32_t* weights, double* G, int n_rows, int d, int d_sub, int L,
                          void* stream);

/* A register-only loop of v_mfma_f64_16x16x4_f64 (4 independent accumulators per wave, 4 waves per workgroup, `iters` x 4 instructions per
 * wave, no memory access in the loop): the measured ceiling that tools/bench_ensemble.py quotes K53's rate against, since no FP64
 * matrix peak is on record.  sink: DEVICE (blocks * 256) float64, written once.  2048 flops per instruction and wave. */
int wsu_mfma_f64_loop(double* sink, int blocks, int iters, void* stream);

/* ---- K12-K14: HILL-cost weighted prediction error (wMAE) of src/filters/evaluate.py:79-115 `get_filter_residuals_cover` and
 *      src/predictor_error.py:19-76 `attack`.  Both reference callers take HILL from a library (conseal.hill._costmap.compute_cost,
 *      stegolab2.hill.compute_rho); here both are the textbook cost, the one pinned by results/prediction/filters.csv:
 *        R = x (*) [[-1,2,-1],[2,-4,2],[-1,2,-1]];  rho0 = 1 / (box3x3(|R|)/9);  cost = box15x15(rho0)/225   ('same', boundary 'symm')
 *        cost[isinf | isnan | cost > 1e10] = 1e10                                  (filters/evaluate.py:104, predictor_error.py:66)
 *
 * K12: x_u8 (N,H,W) DEVICE -> cost (N,H,W) DEVICE fp32 with cost[inf | nan | > clamp] = clamp (the reference's clamp is 1e10;
 *      q and wMAE below need a positive finite clamp). */
int wsu_hill_cost(const uint8_t* x_u8, float* cost, float clamp, int n, int h, int w, void* stream);

/* K13: per-image threshold q = numpy.quantile(cost[1:-1,1:-1], quantile) ('linear', filters/evaluate.py:106) by an exact radix select.
 *      (k, g) = floor / fraction of (count-1)*quantile with count = (H-2)(W-2) (host helper ws_unet_amd.hill.quantile_index);
 *      q: (N) DEVICE fp64 = a + (b-a)*g  (b - (b-a)*(1-g) when g >= 0.5), a = c_(k), b = c_(min(k+1, count-1)).
 *      The workspace (DEVICE, wsu_hill_threshold_workspace_bytes(n)) is zeroed on the stream by every call; deterministic. */
size_t wsu_hill_threshold_workspace_bytes(int n);
int wsu_hill_threshold(const float* cost, long long k, double g, double* q, void* workspace, size_t workspace_bytes,
                       int n, int h, int w, void* stream);

/* K14: per-image mae = mean|x - x_hat| and wmae = mean|x - x_hat| over cost <= q on the interior [1:-1,1:-1]
 *      (filters/evaluate.py:101-107, predictor_error.py:60-67).  The prediction is either
 *        x_hat (DEVICE fp32): hat_full=1 -> (N,H,W) read at [r][c] (a network output; hat_scale = 255), hat_full=0 -> (N,H-2,W-2);
 *                             the residual is K10's float32 x - x_hat*hat_scale, or
 *        pixel_filter (HOST, 9 doubles, weight of x[r-1+a][c-1+b] at [a*3+b]): get_filter_residuals' float64 y - x @ filter
 *                             (filters/evaluate.py:53-76), evaluated inside the kernel.
 *      mae, wmae: (N) DEVICE fp64 (fixed-order fp64 sums, deterministic); selected: optional (N) DEVICE int64 count of cost <= q. */
size_t wsu_prediction_error_workspace_bytes(int n);
int wsu_prediction_error(const uint8_t* x_u8, const float* x_hat, const double* pixel_filter, int hat_full, float hat_scale,
                         const float* cost, const double* q, double* mae, double* wmae, long long* selected,
                         void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream);

/* ---- K15: correlation of a predictor's cover estimate, made from the stego image, with the embedding change,
 *      src/correlation.py:22-59 `run` (results/estimation/correlation.csv), per cover/stego pair on the interior [1:-1,1:-1]:
 *        d = x_s - x_c;  dhat = xhat - x_c;  cor = (sum((dhat - mean dhat)(d - mean d)) / (n-1)) / std(xhat) / std(d)
 *      with n = (H-2)(W-2) and both stds ddof 0 -- the reference's quirks, restated: std of xhat (not dhat), so the identity
 *      filter gives ~0.013 and |cor| can exceed 1; IEEE division (x_s == x_c -> NaN, constant prediction -> +-inf or NaN).
 *      xc_u8, xs_u8: (N,H,W) DEVICE cover / stego pixels.  The prediction xhat of the STEGO plane is either
 *        x_hat (DEVICE fp32): hat_full=1 -> (N,H,W) read at [r][c], xhat = float32(x_hat*hat_scale) (a network output, hat_scale = 255),
 *                             hat_full=0 -> (N,H-2,W-2) (what a host `predictor(x)` returns; hat_scale = 1), or
 *        pixel_filter (HOST, 9 doubles K[a][b] of the reference's (3,3,1) kernel array, K11's layout): the 'valid' convolution
 *                             sum_ab K[a][b] * x_s[r+1-a][c+1-b], evaluated inside the kernel in fp64.
 *      Two passes (means, then centred fp64 sums), fixed-order and free of float atomics: deterministic and batch-independent.
 *      cor: (N) DEVICE fp64; moments: optional (N,6) DEVICE fp64 {mean xhat, mean dhat, mean d, S_hd, S_hh, S_dd} (centred sums).
 *      workspace: DEVICE, wsu_pair_correlation_workspace_bytes(n). */
size_t wsu_pair_correlation_workspace_bytes(int n);
int wsu_pair_correlation(const uint8_t* xc_u8, const uint8_t* xs_u8, const float* x_hat, const double* pixel_filter, int hat_full,
                         float hat_scale, double* cor, double* moments, void* workspace, size_t workspace_bytes,
                         int n, int h, int w, void* stream);

/* ---- K16-K18: the KB-stratified absolute-error box table, src/error_boxes.py `plot_error` (results/prediction/ae_boxes_3.csv):
 *      per predictor the absolute error (AE) of every interior pixel [1:-1,1:-1] of the split, image-major; the pixels are cut into
 *      slices by the anchor predictor's AE (the reference sorts by it and slices at argmin(sorted <= e_j) - 1, defs.py:77-92 for
 *      the statistics), and each (predictor, slice) reports min, q25, q50, q75, max.
 *
 * K16 wsu_ae_values: the float32 AE of one predictor for N (N,H,W) DEVICE u8 planes, written to keys[key_offset + i*per + j]
 *      (per = num_idx, or (H-2)(W-2) for all pixels, row-major); key_capacity bounds the write.  The predictor is either
 *        pixel_filter (HOST, 9 doubles, the weight of x[r-1+a][c-1+b] at [a*3+b]: K14's layout): |y - x @ f| in fp64
 *                     (filters/evaluate.py:53-76), exact in float32 for the dyadic taps the Python layer admits, or
 *        x_hat (DEVICE fp32 (N,H,W) network output): |x - float32(x_hat*hat_scale)|, K10's float32 residual.
 *      idx: optional DEVICE int64 (N,num_idx) interior indices (`subset_residual`'s draws, with replacement, in draw order).
 *      flag: DEVICE u32, OR-ed with 1 on a NaN / infinite AE and with 2 on an index outside the interior (that key is not written).
 * K17 wsu_ae_slices: over `count` anchor keys (DEVICE fp32, non-negative) and HOST edges e_j (1..5 of them), writes DEVICE u64
 *      out[num_edges + 1][3]: row j < num_edges {#(a <= e_j), bits of max{a <= e_j}, largest index holding it + 1} -- the key at
 *      rank c_j - 1 of the stable sort by (a, index) -- and row num_edges {-, bits of max a, largest index holding it + 1}, the
 *      key at rank N - 1 (0 = no such key).  The host turns them into the slices' boundary keys.
 * K18 wsu_ae_select: exact order statistics per (predictor, slice) by a radix select over the float32 bit patterns (11/11/10-bit
 *      digits, one pass over all predictors' keys per level, then one for c_(k+1)).  keys: DEVICE fp32 [num_pred][stride], the first
 *      `count` of each row used; anchor: the row that defines the slices.  slices: HOST int64 [num_slices][10] = {size, has_lo,
 *      lo_bits, lo_idx, has_hi, hi_bits, hi_idx, k0, k1, k2}: a pixel at index i with anchor bits a is in the slice iff
 *      (lo_bits, lo_idx) <= (a, i) < (hi_bits, hi_idx) lexicographically (an absent bound always holds); size = its pixel count
 *      (0 = empty); k_t < size are the ranks to select.  out: DEVICE u32 [num_pred][num_slices][8] float32 bits {min, max,
 *      c_(k0), c_(k0+1), c_(k1), c_(k1+1), c_(k2), c_(k2+1)} (c_(k+1) clamped to the last rank; NaN for an empty slice).
 *      flags: DEVICE u32 [num_pred], 1 where a key is negative, NaN or infinite.  Integer atomics only: deterministic.
 *      workspace: DEVICE, wsu_ae_select_workspace_bytes(num_pred); num_pred <= 16, num_slices <= 6. */
int wsu_ae_values(const uint8_t* x_u8, const float* x_hat, const double* pixel_filter, float hat_scale, const long long* idx, int num_idx,
                  float* keys, size_t key_offset, size_t key_capacity, uint32_t* flag, int n, int h, int w, void* stream);
int wsu_ae_slices(const float* anchor_keys, long long count, const double* edges, int num_edges, unsigned long long* out, void* stream);
size_t wsu_ae_select_workspace_bytes(int num_pred);
int wsu_ae_select(const float* keys, size_t stride, int num_pred, int anchor, long long count, const long long* slices, int num_slices,
                  uint32_t* out, uint32_t* flags, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K19: exact confusion counts of a threshold sweep, src/ws/roc.py `produce_roc` (results/detection/auc_*.csv, roc_*.csv),
 *      for `groups` groups of scores in one call.  numpy's semantics, as the reference computes (y_hat > tau) & (y > 0.):
 *        TP_j = #{pos: s > tau_j}   FP_j = #{neg: s > tau_j}   TN_j = #{neg: s <= tau_j}   FN_j = #{pos: s <= tau_j}
 *      compared in float64 (a float32 score widened exactly: NumPy 2 / NEP 50 compares a float32 array with an np.float64 tau in
 *      float64; numpy 1.x rounded tau to float32 first).  A NaN score or a label other than 0 / 1 is in none of the four counts;
 *      +-inf are ordinary scores.
 *      scores: DEVICE fp64 [offsets[groups]]; labels: DEVICE int8, one per score: 1 = positive (y > 0), 0 = negative (y <= 0),
 *      -1 = neither (y is NaN); offsets: HOST int64 [groups + 1], offsets[0] = 0, non-decreasing -- group g is
 *      [offsets[g], offsets[g+1]) (empty groups allowed; scores / labels may be NULL when every group is); taus: HOST fp64 [t],
 *      finite, strictly ascending, 1 <= t <= 4096; groups <= 65535.  taus and offsets are copied into the workspace on `stream`.
 *      counts: DEVICE int64 [groups][t][4] = {TP, FP, TN, FN} at taus[j].  Two passes: a (label, bin) histogram per group with
 *      bin = #{tau_j < s} (LDS, 64-bit global integer atomics), then a fixed-order prefix scan -- deterministic and independent of
 *      how the scores are split into calls.  workspace: DEVICE, wsu_roc_counts_workspace_bytes(groups, t) (0 for bad arguments),
 *      zeroed on the stream by every call. */
size_t wsu_roc_counts_workspace_bytes(int groups, int t);
int wsu_roc_counts(const double* scores, const signed char* labels, const long long* offsets, int groups, const double* taus, int t,
                   long long* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K20-K23, K28, K30, K34: the stego simulators HILLR, LSBR, LSBRS, LSBRK and HILLRM.  The reference's stego twins were made by a library outside its tree; HILLR is
 *      pinned to them bit for bit (tests/golden/stego_HILLR_*), LSBR's realisation is defined here.  Every plane is DEVICE (N,H,W) and
 *      contiguous; H, W >= 1, H*W < 2^32, N <= 65535.  stego may alias cover.  Deterministic: integer atomics only, two calls give the
 *      same bits, and an image's result does not depend on its position in the batch or on the batch size.
 *
 * K20: the HILL cost of K12 in float64 with the operation order of numpy's float64 restatement (exact integer S, 1.0 / (S / 9.0) as
 *      two divisions, +inf where S == 0, 15 horizontal then 15 vertical taps each added in order from 0, / 225.0, then
 *      inf | nan | > clamp -> clamp): bit-identical to it.  This is the ranking key of HILLR; the float32 cost of K12 cannot be (two
 *      keys of a reference cover are 9.4e-8 apart, relatively).  0 < clamp < inf. */
int wsu_hill_cost_f64(const uint8_t* x_u8, double* key, double clamp, int n, int h, int w, void* stream);
/* K21: bits[i] = the uint64 pattern of the key of rank k[i] (0-based, ascending) among the H*W keys of image i, by an exact radix
 *      select.  Keys must be positive and finite (K20's are, after the clamp), so their patterns order as the values do.  k: DEVICE
 *      int64 [N]; a negative rank gives the pattern 0, which is below every key (K22 then changes nothing); a rank >= H*W is taken as
 *      H*W - 1.  workspace: DEVICE, 8-byte aligned, wsu_rank_select_f64_workspace_bytes(n) (0 for n <= 0), zeroed on the stream by
 *      every call. */
size_t wsu_rank_select_f64_workspace_bytes(int n);
int wsu_rank_select_f64(const double* key, const long long* k, uint64_t* bits, void* workspace, size_t workspace_bytes,
                        int n, int h, int w, void* stream);
/* K22: stego = cover ^ (key <= c) with c = the key whose pattern is bits[i]; changes[i] (DEVICE int64 [N], zeroed on the stream) =
 *      the number of flipped pixels.  With bits from K21 at k = floor((H*W - 1) * alpha / 2) this is HILLR: the k + 1 cheapest pixels
 *      change.  TIES at the threshold are ALL flipped, so changes[i] can exceed k + 1; a flat image, whose keys all equal the clamp, is
 *      flipped entirely.  The reference does not pin that case (its 25 files have a single pixel at the threshold); flipping every tie
 *      is the choice that does not depend on any order among equal keys.  Loads and stores of the planes are 16 bytes wide where cover
 *      and stego share their alignment, single bytes at an image's unaligned ends. */
int wsu_embed_threshold(const uint8_t* cover, const double* key, const uint64_t* bits, uint8_t* stego, long long* changes,
                        int n, int h, int w, void* stream);
/* K23: LSB replacement at change rate alpha / 2 with a counter-based generator: pixel i (linear index in its image) flips iff
 *      word < thresholds[image], word = output word i % 4 of Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments
 *      0x9E3779B9 / 0xBB67AE85) on the counter (i / 4, 0, 0, 0) under the key (low, high word of seeds[image]).  seeds: DEVICE uint64
 *      [N]; thresholds: DEVICE uint32 [N], each from wsu_lsbr_threshold (HOST: *threshold = floor(alpha / 2 * 2^32) in float64, alpha in
 *      [0, 1]; 0 copies the cover); changes as in K22. */
int wsu_lsbr_threshold(double alpha, uint32_t* threshold);
int wsu_embed_lsbr(const uint8_t* cover, const uint64_t* seeds, const uint32_t* thresholds, uint8_t* stego, long long* changes,
                   int n, int h, int w, void* stream);
/* K28: LSBRS, sequential LSB replacement: the message occupies the first counts[image] pixels of the path over the WHOLE plane (row by
 *      row, left to right within a row; order = 0: rows from the top, order = 1: rows from the bottom).  Pixel i (linear index) flips iff
 *      its path position (order 0: i; order 1: (H - 1 - i / W) * W + i % W) is < counts[image] AND it flips under K23 at alpha = 1 with the
 *      same seed (word i % 4 of Philox4x32-10 on counter (i / 4, 0, 0, 0) < 2^31).  So at counts = H*W the twin is K23's alpha = 1 twin bit
 *      for bit in both orders, every pixel at a path position >= counts is the cover's, and a twin at a smaller count is a prefix of one at
 *      a larger count.  counts: DEVICE int64 [N], for a payload alpha the HOST value floor(alpha * H * W) in float64 (clamped to 0..H*W
 *      here); seeds, changes, limits and aliasing as in K23. */
int wsu_embed_lsbr_seq(const uint8_t* cover, const uint64_t* seeds, const long long* counts, int order, uint8_t* stego, long long* changes,
                       int n, int h, int w, void* stream);

/* K30: LSBRK, LSB replacement at the positions a stego key selects, the same in every image: pixel i (linear index) is USED iff
 *      key word < alpha_threshold, compared in 64 bits, key word = word i % 4 of Philox4x32-10 on counter (i / 4, 0, 0, 0) under the key
 *      (low, high word of key_seed); alpha_threshold = floor(alpha * 2^32) in 0..2^32, so alpha = 1 uses every pixel.  A used pixel flips
 *      iff it flips under K23 at alpha = 1 with its image's seed (the same word under seeds[image] < 2^31).  So at alpha_threshold = 2^32
 *      the twin is K23's alpha = 1 twin bit for bit, at 0 it is the cover, and the flips are a subset of the used positions, which depend
 *      on (key_seed, alpha_threshold, H, W) alone.  seeds, changes, limits and aliasing as in K23.
 *      wsu_lsbr_key_mask writes those used positions as a DEVICE (H,W) uint8 plane of 1 / 0. */
int wsu_embed_lsbr_keyed(const uint8_t* cover, const uint64_t* seeds, uint64_t key_seed, uint64_t alpha_threshold, uint8_t* stego,
                         long long* changes, int n, int h, int w, void* stream);
int wsu_lsbr_key_mask(uint64_t key_seed, uint64_t alpha_threshold, uint8_t* mask, int h, int w, void* stream);
/* K34: HILLRM, HILLR's pixel selection carrying a real message: a pixel whose key (K20) is <= the key whose pattern is bits[image] (K21,
 *      for a payload alpha at the HOST rank floor((H*W - 1) * alpha), -1 for alpha = 0) is USED, ties included as in K22; a used pixel
 *      flips iff it flips under K23 at alpha = 1 with its image's seed.  So the flips are a subset of K22's at the same threshold, and a
 *      negative rank leaves the cover.  seeds, changes, limits and aliasing as in K23. */
int wsu_embed_threshold_lsbr(const uint8_t* cover, const double* key, const uint64_t* bits, const uint64_t* seeds, uint8_t* stego,
                             long long* changes, int n, int h, int w, void* stream);

/* ---- K37-K39: the +-1 embedding simulators LSBM and HILL (LSB matching: Sharp, IH 2001; the payload-limited sender: Filler & Fridrich, IEEE TIFS
 *      5(4), 2010; not part of the reference).  Planes, limits, aliasing, seeds, the generator word of pixel i and `changes` as in K23.  For a
 *      multiplier lambda > 0 and a cost rho > 0 (+inf: a wet pixel), in float64 with one rounding per operation:
 *        a = lambda * rho;   a+ = +inf where x == 255, else a;   a- = +inf where x == 0, else a;   e+- = exp(-a+-), exp(-inf) = 0;
 *        Z = (1 + e+) + e-;   p+- = e+- / Z:  the probabilities of the changes +1 and -1, never out of 0..255.
 *
 * K37: entropy[i][l] = the sum over image i's pixels of h = log2(Z) + (t+ + t-) / (Z ln 2), t+- = a e+- where e+- > 0 else 0, at
 *      lambda = lambdas[i][l]: the bits a sender with these change probabilities embeds.  One pass over rho serves all l multipliers,
 *      1 <= l <= 16.  x_u8: (N,H,W); rho: DEVICE float64 (N,H,W); lambdas: DEVICE float64 [N][l]; entropy: DEVICE float64 [N][l].  Sums
 *      are taken in a fixed order (no float atomics): two calls give the same bits, whatever the batch.  workspace: DEVICE, 8-byte aligned,
 *      wsu_ternary_entropy_workspace_bytes(n) (0 for n <= 0), written before it is read by every call. */
size_t wsu_ternary_entropy_workspace_bytes(int n);
int wsu_ternary_entropy(const uint8_t* x_u8, const double* rho, const double* lambdas, int l, double* entropy, void* workspace,
                        size_t workspace_bytes, int n, int h, int w, void* stream);
/* K38: HILL when rho is K20's cost: with T+- = floor(p+- * 2^32) at lambda = lambdas[image] (DEVICE float64 [N]; +inf leaves the cover) and
 *      u the generator word of pixel i, stego = cover + 1 where u < T+, cover - 1 where T+ <= u < T+ + T-, else cover. */
int wsu_embed_ternary(const uint8_t* cover, const double* rho, const double* lambdas, const uint64_t* seeds, uint8_t* stego,
                      long long* changes, int n, int h, int w, void* stream);
/* K39: LSBM, the same draw with constant thresholds: T+ = T- = T = thresholds[image] inside the range, (2T, 0) at x == 0 and (0, 2T) at
 *      x == 255, so a fraction alpha / 2 of the pixels changes by +-1 with a random sign, inwards at the ends of the range.  thresholds:
 *      DEVICE uint32 [N], each from wsu_lsbm_threshold (HOST: *threshold = floor(alpha / 4 * 2^32) in float64, alpha in [0, 1]; 0 copies
 *      the cover). */
int wsu_lsbm_threshold(double alpha, uint32_t* threshold);
int wsu_embed_lsbm(const uint8_t* cover, const uint64_t* seeds, const uint32_t* thresholds, uint8_t* stego, long long* changes,
                   int n, int h, int w, void* stream);
/* K51: the change probability of K38's sender per pixel, as a 16-bit fixed-point weight: with a, e+-, Z as above at lambda =
 *      lambdas[image] (DEVICE float64 [N], given by the caller: nothing is solved here),  beta = (e+ + e-) / Z  and
 *      weights[i] = floor(beta * 65536) in float64.  beta <= 2/3, so a weight is at most 43 690 and nothing is clipped; rho = +inf or
 *      lambda = +inf gives 0; a beta below 2^-16 = 1.5e-5 gives 0.  weights_u16: DEVICE uint16 (N,H,W), the selection channel that K52
 *      takes.  H * W < 2^32, N <= 65535; every argument is checked before any HIP call. */
int wsu_change_weights(const uint8_t* x_u8, const double* rho, const double* lambdas, uint16_t* weights_u16, int n, int h, int w, void* stream);

/* ---- K40-K42: binary syndrome-trellis codes (Filler, Judas, Fridrich, IEEE TIFS 6(3), 2011; not part of the reference): a message that is
 *      really carried, embedded with near-minimal additive cost and read back.  Planes, limits and seeds as in K23, but H * W < 2^31.
 *      Per image, over the LSBs x[0..n) along a pixel path (n = H * W), costs rho[0..n) >= 0 (+inf: wet, NaN: not allowed), a message
 *      m[0..k) of bytes 0 / 1, 1 <= k <= n, a constraint height 1 <= height <= 10, S = 2^height states and a column table
 *      cols[0..ceil(n / k)) of height-bit integers:
 *        block i owns the path positions [floor(i n / k), floor((i + 1) n / k));  its position t has the column
 *        cols[t] & ((1 << min(height, k - i)) - 1), whose bit r reaches message bit i + r;
 *        forward:  W[0] = 0, W[s > 0] = +inf;  per position j with column c:  a = W[s] + (x_j ? rho_j : 0),  b = W[s ^ c] + (x_j ? 0 : rho_j),
 *                  take[j][s] = b < a (a tie keeps y_j = 0),  W[s] = take ? b : a;  after block i: W[s] = W[2 s + m_i] for s < S / 2, +inf above;
 *        cost = W[0] after the last block: the least sum of rho_j over y_j != x_j among all y with syndrome m;  ok = cost < +inf;
 *        backward: s = 0;  for i = k - 1 .. 0:  s = 2 s + m_i, then down the block's positions  y_j = take[j][s],  s ^= c_j where y_j is set;
 *        extract:  m_b = XOR of y_j over the blocks i in (b - height, b] and their positions t whose column has bit b - i set.
 *      Only float64 additions and comparisons touch a cost: the results are bit for bit those of a numpy restatement.
 *      path: DEVICE int32 [N][n], per image a permutation of the raster indices (position -> pixel), or NULL for raster order; an entry
 *      outside [0, n) is never dereferenced (the position counts as wet and its pixel is not written).  cols: DEVICE uint32.
 *
 * K40: words[i][p] = the generator word of pixel p under seeds[i] (word p % 4 of Philox4x32-10 on counter (p / 4, 0, 0, 0), K23's): the
 *      sort key of the keyed path and the sign bit of K41's +-1 change.  words: DEVICE uint32 (N,H,W); H * W < 2^32. */
int wsu_philox_words(const uint64_t* seeds, uint32_t* words, int n, int h, int w, void* stream);
/* K41: phases 1: forward (writes cost, ok and the workspace), 2: backward (reads them, writes stego and changes), 3: both.  Where y_j differs
 *      from the cover's LSB the pixel becomes x ^ 1 (change 0) or x + d, d = +1 / -1 as bit 0 of its generator word is 1 / 0, inwards at 0
 *      and 255 (change 1); every other pixel, and every pixel of an image that is not ok, is copied.  cost: DEVICE float64 [N]; changes:
 *      DEVICE int64 [N]; ok: DEVICE uint8 [N]; stego may alias cover.  workspace: DEVICE, 8-byte aligned, n * wsu_stc_workspace_bytes(H * W,
 *      height) bytes (pixels * max(2^height, 64) / 8 each: the take bits; 0 for bad arguments), written by phase 1 before phase 2 reads it. */
size_t wsu_stc_workspace_bytes(long long pixels, int height);
int wsu_stc_embed(const uint8_t* cover, const double* rho, const uint8_t* message, const uint32_t* cols, const int32_t* path,
                  const uint64_t* seeds, int change, int height, int k, int phases, uint8_t* stego, double* cost, long long* changes,
                  uint8_t* ok, void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream);
/* K42: message[i][b] = m_b of stego image i, one thread per message bit.  message: DEVICE uint8 [N][k]. */
int wsu_stc_extract(const uint8_t* stego, const uint32_t* cols, const int32_t* path, int height, int k, uint8_t* message, int n, int h,
                    int w, void* stream);
/* K43, K44: K41 (both phases) and K42 with a message length per image, for messages of unequal length in one batch: image i embeds / reads
 *      the ks[i] bits message[i * message_stride + first[i] ..].  ks, first: DEVICE int32 [N], 0 <= ks[i] <= H * W, first[i] >= 0,
 *      first[i] + ks[i] <= max_bits <= message_stride (max_bits: HOST, the most bits of a row any image may touch).  cols: DEVICE uint32
 *      [cols_len], cols_len >= ceil(H * W / ks[i]) for every positive ks[i].  ks[i] == 0: no block exists; K43 gives stego = cover, cost 0,
 *      changes 0, ok 1, and K44 writes nothing for that image.  A workgroup reads its image's ks and first once at entry; what they hold
 *      is only known on the device, so an image whose values break a condition above is treated as ks[i] = 0 and K43 reports cost +inf and
 *      ok 0 for it (stego = cover): no access leaves the buffers on its account.  Everything else, and every bit of the results, as K41 /
 *      K42 with k = ks[i]; wsu_stc_embed / wsu_stc_extract are these kernels with one k for all.
 *      K44's `bit` (0..7) names the bit of the stego byte that is the code's bit (K42 reads bit 0); rows of `message` are written only in
 *      [first[i], first[i] + ks[i]). */
int wsu_stc_embed_ragged(const uint8_t* cover, const double* rho, const uint8_t* message, long long message_stride, const int32_t* ks,
                         const int32_t* first, int max_bits, const uint32_t* cols, int cols_len, const int32_t* path, const uint64_t* seeds,
                         int change, int height, uint8_t* stego, double* cost, long long* changes, uint8_t* ok, void* workspace,
                         size_t workspace_bytes, int n, int h, int w, void* stream);
int wsu_stc_extract_ragged(const uint8_t* stego, const uint32_t* cols, int cols_len, const int32_t* path, int height, int bit,
                           const int32_t* ks, const int32_t* first, int max_bits, uint8_t* message, long long message_stride, int n, int h,
                           int w, void* stream);

/* ---- K45-K47: the planes of the ternary two-layer syndrome-trellis embedder (Filler, Judas, Fridrich 2011, sections V-VI, for +-1 changes; not
 *      part of the reference; ws_unet_amd.stc_ml drives them).  Two binary codes (K43) run along one keyed path with one column table:
 *      first over bit 1 of the pixels, then over bit 0.  Per image: cover x in 0..255, n = H * W pixels, one cost rho >= 0 per pixel for both
 *      directions (+inf: wet), a message m[0..k), k >= 2, and the multiplier lambda of K37's search for k bits (its lower bracket end).
 *      With K37's text unchanged:  a = lambda * rho;  a+ = +inf where x == 255, else a;  a- = +inf where x == 0, else a;  e+- = exp(-a+-);
 *      Z = (1 + e+) + e-.   d = the direction that changes bit 1 of x: +1 for odd x, -1 for even x;  o = the other direction.
 *        high layer:  cover bit u1 = (x >> 1) & 1;  cost rho1 = a_d + log1p(e_o)  (= ln((1 - q1) / q1) for q1 = e_d / Z without overflow or
 *                     cancellation; +inf where a_d is);  H1 = the sum over the pixels of the binary entropy of q1 in bits, each term
 *                     h1 = (r log1p(t)) / ln 2 - q1 log2(q1) where e_d > 0 and 0 elsewhere, r = (1 + e_o) / Z, t = e_d / (1 + e_o);
 *                     k1 = min(floor(H1), k - 1);  k1 == 0: the layer is not run, y1 = u1;  else y1 = K43's solution for (u1, rho1, m[0..k1));
 *        low layer:   k0 = k - k1 >= 1;  where y1 != u1 the pixel is decided (it becomes x + d): u0 = 1 - (x & 1), rho0 = +inf;  elsewhere
 *                     u0 = x & 1, rho0 = a_o (the product lambda * rho itself, +inf at the range's end);  y0 = K43's solution for
 *                     (u0, rho0, m[k1..k));
 *        stego:       x + d where y1 != u1;  x + o where bit 1 was kept and y0 != (x & 1);  x otherwise.  Then (y >> 1) & 1 == y1 and
 *                     y & 1 == y0, the stego stays in 0..255 and a wet pixel never changes.  ok = ok1 and ok0; an image that is not ok is
 *                     copied.  The receiver reads m[0..k1) from bit 1 and m[k1..k) from bit 0 (K44), knowing (seed, H, W, height, k1, k0).
 *      The first layer is sized by its entropy, the last takes the rest; no smaller payload is tried when a layer has no solution.
 *      Planes (N,H,W), H * W < 2^31, N <= 65535; lambdas: DEVICE float64 [N]; k1: DEVICE int32 [N].  Sums are taken in K37's fixed order (no
 *      float atomics): the same bits whatever the batch.  workspace: DEVICE, 8-byte aligned, wsu_stc_layer_workspace_bytes(n) bytes (0 for
 *      n <= 0), written before it is read by every call.
 *
 * K45: u1 (DEVICE uint8 plane of 0 / 1), rho1 (DEVICE float64 plane) and entropy[i] = H1 of image i (DEVICE float64 [N]) in one pass. */
size_t wsu_stc_layer_workspace_bytes(int n);
int wsu_stc_layer_high(const uint8_t* x_u8, const double* rho, const double* lambdas, uint8_t* u1, double* rho1, double* entropy,
                       void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream);
/* K46: u0 and rho0 from bit 0 of the plane y1 (K43's output over u1); where k1[i] <= 0, y1 is not read. */
int wsu_stc_layer_low(const uint8_t* x_u8, const double* rho, const double* lambdas, const uint8_t* y1, const int32_t* k1, uint8_t* u0,
                      double* rho0, int n, int h, int w, void* stream);
/* K47: the stego plane from bit 0 of y1 (ignored where k1[i] <= 0) and of y0;  ok[i] = ok1[i] and ok0[i] (DEVICE uint8 [N] each), else image i
 *      is copied;  changes[i] (DEVICE int64) = its changed pixels, distortion[i] (DEVICE float64) = the sum of rho over them.  A pixel whose
 *      planes ask for a step out of 0..255 (they cannot, when they are K43's over K45 / K46's costs) is not changed.  stego may alias cover. */
int wsu_stc_layer_compose(const uint8_t* cover, const double* rho, const uint8_t* y1, const uint8_t* y0, const int32_t* k1,
                          const uint8_t* ok1, const uint8_t* ok0, uint8_t* stego, long long* changes, double* distortion, uint8_t* ok,
                          void* workspace, size_t workspace_bytes, int n, int h, int w, void* stream);

/* ---- K48: the directional wavelet cost map of S-UNIWARD (Holub, Fridrich, Denemark, "Universal distortion function for steganography in
 *      an arbitrary domain", EURASIP JIS 2014) and of WOW (Holub, Fridrich, "Designing steganographic distortion using directional
 *      filters", WIFS 2012); not part of the reference; ws_unet_amd.costs drives it, tests/costs_np.py restates it.  All float64.
 *        filter:   p[0..15] = the Daubechies-8 orthonormal scaling filter, minimum phase, sum p = sqrt 2 (p[0] = 0.0544158422...; the
 *                  literals of ws_unet_amd.costs.DB8, derived by tools/db8_taps.py);  l[j] = p[15 - j];  h[j] = (-1)^(j+1) p[j].
 *        bands:    F_k[u,v] = a_k[u] b_k[v], u down the rows, v along the columns:  (a,b)_1 = (l,h),  (a,b)_2 = (h,l),  (a,b)_3 = (h,h).
 *        padding:  X~ = the cover as float64 under numpy.pad(mode='symmetric'), the periodic fold of K20 (planes smaller than the pad
 *                  are defined).  Indices are unpadded coordinates.
 *        forward:  r_b[y,n]  = sum_{v=0..15} b[v] X~[y, n+8-v]          for b in {l, h},  n in [-8, W+6],  y in [-15, H+14]
 *                  W_k[m,n]  = sum_{u=0..15} a_k[u] r_bk[m+8-u, n]      m in [-8, H+6]
 *        g_k:      S-UNIWARD  1 / (|W_k| + sigma), sigma > 0;     WOW  |W_k|
 *        back:     t_k[m,j]  = sum_v |b_k[v]| g_k[m, j-8+v]             xi_k[i,j] = sum_u |a_k[u]| t_k[i-8+u, j],   i < H, j < W
 *        merge:    S-UNIWARD  rho = (xi_1 + xi_2) + xi_3;         WOW  rho = (1/xi_1 + 1/xi_2) + 1/xi_3  (a flat neighbourhood has xi = 0,
 *                  1/0 = +inf);     both, as K20:  rho <= clamp ? rho : clamp  (inf | nan | > clamp -> clamp).
 *      Every sum starts at +0.0 and adds its taps in ascending order; a product and its addition round separately; the divisions are
 *      IEEE divisions; no library function is called: the plane equals the numpy restatement bit for bit, and an image's plane does not
 *      depend on the batch.  rho[i,j] sums |F_k[u,v]| g over exactly the 3 * 256 coefficients that pixel (i,j) enters with weight
 *      F_k[u,v]: for S-UNIWARD that is the authors' D(X, X +- e_ij) wherever the pixel does not meet its own mirror image in the padding
 *      (tests/test_costs_host.py).  The published codes' clamps (1e8, 1e10), their pad of 16, sigma = 1 and this alignment are as
 *      remembered; no run was compared with them.
 *      x_u8: DEVICE (N,H,W) uint8; rho: DEVICE (N,H,W) float64, 8-byte aligned; H, W >= 1, H*W < 2^32, N <= 65535.  sigma is ignored
 *      by WOW.  0 < clamp < inf.  Every argument is checked before any HIP call. */
#define WSU_COST_SUNIWARD 0
#define WSU_COST_WOW 1
int wsu_wavelet_cost_f64(const uint8_t* x_u8, double* rho, int kind, double sigma, double clamp, int n, int h, int w, void* stream);

/* ---- K31, K32: the JPEG history of a bitmap (Boehme, "Weighted stego-image steganalysis for JPEG covers", IH 2008; not part of the
 *      reference): which quantisation table an image was compressed with, and the image after a round trip through a table -- the WS
 *      predictor for covers that were a JPEG once (the quantiser rounds the +-1 embedding noise away).  All arithmetic is exact integers:
 *        blocks of 8 x 8 on the grid at the plane's origin; H and W multiples of 8, H*W <= 2^24, N <= 65535;
 *        C[k][n] = rint(2^13 c_k cos((2n+1) k pi / 16)) as int64, c_0 = sqrt(1/8), c_k = sqrt(2/8);
 *        Y = C (X - 128) C^T at scale 2^26;   for a table entry Q in 1..255, D = Q 2^26:   k = sign(Y) ((|Y| + D/2) / D), half away from zero.
 *      x_u8: DEVICE (N,H,W), 8-byte aligned.  tables: HOST int32, entries in 1..255 (checked with every other argument before any HIP
 *      call); the kernels know nothing of JPEG qualities (ws_unet_amd.ops.jpeg_tables builds the IJG luminance tables).
 *
 * K31: tables (m,64), m >= 1, row-major 8 x 8 by frequency [u][v].  energies: DEVICE int64 (N,m), 8-byte aligned, zeroed on the stream by
 *      this call:  energies[i][j] = sum over image i's coefficients of r'^2,  r = Y - k D,  r' = (r + 2^15) >> 16 (arithmetic shift; scale 2^10).
 *      energies / 2^20 / (H W) is the residual energy per pixel.  Integer sums (64-bit atomics): the same bits on every run. */
int wsu_jpeg_energies(const uint8_t* x_u8, const int* tables, int m, long long* energies, int n, int h, int w, void* stream);
/* K32: tables (N,64), one per image; use: HOST uint8 [N].  Where use[i] != 0, with Z = C^T (k Q) C + 128 2^26 (int64):
 *        x_hat[i]    = float32(clamp(Z, 0, 255 2^26) / 2^26)       (the quotient in float64, rounded once to float32)
 *        x_u8_out[i] = clamp((Z + 2^25) >> 26, 0, 255)             (the recompressed image)
 *      Where use[i] == 0 the table is not read: x_hat[i] is the KB filter's prediction in K11's float32 operation sequence
 *      (convolve(x / 255.f, KB) summed K00 .. K22, times 255.f) on the interior and the pixel itself on the border (the statistics ignore
 *      it), so K11 with this plane and hat_scale = 1 has the bits of K11 with pixel_filter = KB; x_u8_out[i] is the input.
 *      x_hat: DEVICE fp32 (N,H,W), 16-byte aligned, or null; x_u8_out: DEVICE (N,H,W), 8-byte aligned, not aliasing x_u8, or null; one
 *      of the two must be given.  Plain vector stores; every output element is written. */
int wsu_jpeg_predict(const uint8_t* x_u8, const int* tables, const uint8_t* use, float* x_hat, uint8_t* x_u8_out, int n, int h, int w,
                     void* stream);

/* Linear pixel predictor on its own (filters/evaluate.py:136-141): y (N,H-2,W-2) = convolve(x/255., K, 'valid')*255.
 * x: DEVICE (N,H,W) fp32; filter: HOST 9 floats K[a][b]. */
int wsu_filter3x3_valid_f32(const float* x, const float* filter, float* y, int n, int h, int w, void* stream);

/* (x ^ 1 - x) / 255. as fp32: the network input of the bias term `pixel_estimator(x_bar - x)` (estimate.py:127, evaluate.py:45) */
int wsu_lsb_delta_unit_f32(const uint8_t* x, float* y, size_t count, void* stream);

/* Epoch meter of the training loop (src/_defs/metrics.py:122-142 WSMeter.update): per-image fp64 beta_hat over the interior from the
 * FLOAT inputs x01 and outputs y01, both (N,H,W) single-plane fp32 in [0,1]; the caller clips and averages |beta - alpha/2|. */
int wsu_ws_meter_beta(const float* x01, const float* y01, double* beta_hat, int n, int h, int w, void* stream);

/* ---- u8 -> [0,1] fp32, numpy float32 division semantics of evaluate.py:45 (x / 255.) */
int wsu_u8_to_unit_f32(const uint8_t* x, float* y, size_t count, void* stream);

/* ---- one training batch in one launch (data/pairs.py): gather + dihedral transform + u8 -> [0,1] fp32, inputs and targets together:
 *        inputs[s] = D(op[s])(planes[idx_in[s]]) / 255.0f        covers[s] = D(op[s])(planes[idx_cov[s]]) / 255.0f
 * planes: DEVICE (files,H,W) uint8; idx_in, idx_cov (int32) and op (uint8): DEVICE arrays of n entries; inputs, covers: DEVICE (n,1,H,W)
 * fp32.  The division is that of wsu_u8_to_unit_f32, so op = 0 gives the bits of that kernel followed by a gather.
 * op holds the eight elements of D4 as three bits, applied in this order: bit 0 mirrors the columns (x[:, ::-1]), bit 1 mirrors the rows
 * (x[::-1, :]), bit 2 transposes last.  Output pixel (i, j) reads source (r, c):
 *        (r, c) = (j, i) if bit 2 else (i, j);   r = H-1-r if bit 1;   c = W-1-c if bit 0
 *        op   0         1          2          3           4       5            6            7
 *             identity  x[:,::-1]  x[::-1,:]  rot90(x,2)  x.T     rot90(x,1)   rot90(x,3)   x[::-1,::-1].T      (numpy)
 * allow_transpose: 1 admits ops 4-7 and then requires H == W ("transposing ops need square planes"); 0 admits ops 0-3 on any H, W.
 * A sample whose index is outside [0, files) or whose op is not admitted writes NOTHING (the Python wrapper validates before the launch).
 * Any H, W >= 1; loads are 4 and stores 16 bytes wide when W % 4 == 0 and the pointers are aligned.  n == 0 is a no-op. */
int wsu_pair_batch_f32(const uint8_t* planes, int files, int h, int w, const int32_t* idx_in, const int32_t* idx_cov, const uint8_t* op,
                       int n, int allow_transpose, float* inputs, float* covers, void* stream);
/* The same batch with side-information planes behind the image (the reference's ParityOracle / DemosaicOracle, src/_defs/loader.py:73-103),
 * still one launch.  side: bit 0 appends the parity plane, bit 1 the three demosaic planes; inputs is (n,P,H,W), P = 1 + (side&1) +
 * 3*((side>>1)&1); covers stays (n,1,H,W), or is NULL together with idx_cov (inference: the inputs alone).  With (r, c) the SOURCE coordinate
 * of output pixel (i, j) under op[s] as defined above and v = planes[idx_in[s]][r][c], the planes are, in the reference's transform order:
 *        image    float(v) / 255.0f                      (the bits wsu_pair_batch_f32 writes; so are covers)
 *        parity   float(v & 1)
 *        R site   1.0f where r%2==0 && c%2==0, else 0.0f
 *        G site   1.0f where (r+c)%2==1
 *        B site   1.0f where r%2==1 && c%2==1
 * The reference appends these planes BEFORE its random flips and rotation, so the Bayer grid is transformed with the image: it is a function
 * of the source coordinate, and a mirror of an even side moves its phase.  side outside 0..3 is an argument error (-1) before any HIP call;
 * a sample with a bad index or a non-admitted op writes nothing; vector widths and the n == 0 rule are those of wsu_pair_batch_f32. */
int wsu_pair_batch_planes_f32(const uint8_t* planes, int files, int h, int w, const int32_t* idx_in, const int32_t* idx_cov, const uint8_t* op,
                              int n, int allow_transpose, int side, float* inputs, float* covers, void* stream);

/* ======================= backward / train step (K7, K8, K9) =======================
 * The reference publishes no UNet training script; these entry points are the autograd of
 * UNet.forward (unet.py:137-189) + the loss classes (src/_defs/losses.py:28-121) + torch.optim.AdamW as used
 * by the detector loop (src/detector/train.py:55-95,228).  Gradients are exact-fp32 / split-bf16 on fp32 storage;
 * every reduction is two-stage in a fixed order (bitwise reproducible, no float atomics).
 * "g" always denotes a PRE-activation gradient (dLoss/d(conv output before ReLU)). */

/* dx of conv3x3-reflect: zero-padded transposed conv on the matrix cores + reflect-adjoint border fold.
 * g: (N,H,W,Cout) fp32.  dx1: (N,H,W,csplit), dx2: (N,H,W,cin-csplit) or NULL (the two inputs of a fused concat).
 * relu_mask1/2 (optional, shapes of dx1/dx2): saved post-ReLU activations; where they are <= 0 the gradient is zeroed,
 * which makes dx the pre-activation gradient of the producing layers.  mode: WSU_MODE_F32 or WSU_MODE_BF16X3. */
size_t wsu_conv3x3_bwd_data_workspace_bytes(int n, int h, int w, int cin, int cout, int mode);
int wsu_conv3x3_bwd_data(const void* g, const void* w_packed_dgrad, const float* w_oihw, void* workspace, size_t workspace_bytes,
                         void* dx1, void* dx2, int csplit, const void* relu_mask1, const void* relu_mask2,
                         int n, int h, int w, int cin, int cout, int mode, void* stream);

/* dW (OIHW, Cout x (c1+c2) x 3 x 3) and db (Cout, optional) of conv3x3-reflect on cat[x1, x2]: exact fp32 MFMA (mode F32) or
 * split-bf16 MFMA fed by transposing LDS reads (mode BF16X3); db is always an exact fp32 sum. */
size_t wsu_wgrad_workspace_bytes(int cm, int cn, int ntaps);
int wsu_conv3x3_bwd_weight(const float* g, const float* x1, const float* x2, float* dw, float* db,
                           float* workspace, size_t workspace_bytes,
                           int n, int h, int w, int c1, int c2, int cout, int mode /* F32 exact | BF16X3 */, void* stream);

/* first layer: dW (Cout x cin x 3 x 3), db from g (N,H,W,Cout) and the NCHW fp32 input planes. */
size_t wsu_first_bwd_workspace_bytes(int n, int h, int w, int cin, int cout);
int wsu_conv3x3_first_bwd_weight(const float* g, const float* x_nchw, float* dw, float* db,
                                 float* workspace, size_t workspace_bytes, int n, int h, int w, int cin, int cout, void* stream);

/* first layer: dx (N,cin,H,W) NCHW fp32 -- the input saliency gradient (src/saliency.py:159-174).  cin 1..8, cout a multiple of 4 with
 * cin * cout * 36 <= 163 840 (the weights live in the LDS of one compute unit); more is an argument error that names cin and cout. */
int wsu_conv3x3_first_bwd_data(const float* g, const float* w_oihw, float* dx_nchw, int n, int h, int w, int cin, int cout, void* stream);

/* transposed conv: dW (Cin x Cout x 2 x 2), db (Cout, optional) from x (N,h,w,Cin) and dy (N,2h,2w,Cout) ... */
int wsu_convt2x2_bwd_weight(const float* x, const float* dy, float* dw, float* db,
                            float* workspace, size_t workspace_bytes,
                            int n, int h, int w, int cin, int cout, int mode, void* stream);
/* ... and dx (N,h,w,Cin), optionally masked by the saved post-ReLU activation of the producing layer. */
size_t wsu_convt2x2_packed_dgrad_bytes(int cin, int cout, int mode);
int wsu_convt2x2_pack_dgrad(const float* w_iohw, void* w_packed, int cin, int cout, int mode, void* stream);
int wsu_convt2x2_bwd_data(const void* dy, const void* w_packed_dgrad, void* dx, const void* relu_mask,
                          int n, int h, int w, int cin, int cout, int mode, void* stream);

/* 2x2 max-pool backward into the full-resolution gradient buffer (accumulate != 0: add to what the skip path
 * already stored there).  pool_idx from the forward; xp_relu_mask: pooled activation (gradient only where > 0). */
int wsu_maxpool2x2_bwd(float* g_full, const float* dy_pool, const uint8_t* pool_idx, const float* xp_relu_mask,
                       int n, int h, int w, int c, int accumulate, void* stream);

/* head: gx (N,H,W,C) = relu_mask(x) * W^T (dout * out * (1-out)); dw (cout x C), db (cout); cout <= 4. */
size_t wsu_head_bwd_workspace_bytes(int c, int cout);
int wsu_conv1x1_sigmoid_bwd(const float* x, const float* w, const float* out, const float* dout,
                            float* gx, float* dw, float* db, float* workspace, size_t workspace_bytes,
                            int n, int h, int w_, int c, int cout, int apply_relu_mask, void* stream);

/* K8: L1 + WS loss and dLoss/dout in one call (losses.py:33-36,47-89,99-116).
 * use_l1: 0 = off, 1 = mean |covers - out| (L1Loss), 2 = mean (covers - out)^2 (L2Loss, losses.py:39-42). */
size_t wsu_l1ws_loss_workspace_bytes(int n);
int wsu_l1ws_loss_fwd_bwd(const float* out, const float* covers, const float* inputs, const float* alphas,
                          float* loss, float* loss_parts, float* dout, float* beta_hat, void* workspace, size_t workspace_bytes,
                          int n, long long per_image, int use_l1, int use_ws, void* stream);

/* K9: multi-tensor AdamW (decoupled weight decay), one launch for all parameters.
 * table: DEVICE array of ntensors records {float* p; const float* g; float* m; float* v; int64 n; int64 first_block}.
 * skip_flag: optional device int; non-zero = the launch changes nothing. */
int wsu_adamw_multi_tensor(const void* table, int ntensors, long long total_blocks,
                           float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                           const int* skip_flag, void* stream);

/* Helpers of the train step that keep its scalar arithmetic on the device and inside libwsu (reference: there is none -- PyTorch's
 * GradScaler plays this role for fp16 training; pattern src/detector/train.py:88-95):
 *   wsu_pow2_grad_scale     scale2 = {2^floor(2 - log2 max|x|), its reciprocal}: the power-of-two scale of the f16f8x backward chain
 *   wsu_scale_f32           y = x * factor[0]
 *   wsu_scale_multi_tensor  in-place, many tensors, one launch; table records {float* p; int64 n; int64 first_block}
 *   wsu_nonfinite_flag      flag[0] = bucket holds inf / NaN, flag[1] += flag[0]; feed flag to wsu_adamw_multi_tensor(skip_flag) */
int wsu_pow2_grad_scale(const float* x, long long n, float* scale2, void* workspace, void* stream);
int wsu_scale_f32(const float* x, float* y, long long n, const float* factor, void* stream);
int wsu_scale_multi_tensor(const void* table, int ntensors, long long total_blocks, const float* factor, void* stream);
int wsu_nonfinite_flag(const float* g, long long n, int* flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WSU_H */
