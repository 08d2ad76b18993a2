"""MI355X-native UNet pixel predictor behind the reference's module interface.

Mirrors /root/reference/src/unet/model/unet.py (class UniformDropout :15-51, class UNet :54-199):
same constructor arguments, same parameter names / shapes / init (the layers are
held as never-called ``nn.Conv2d`` / ``nn.ConvTranspose2d`` parameter holders, so
``state_dict()`` keys, default initialisation and RNG consumption are identical and
reference checkpoints load unchanged), same ``forward(x: (N,C,H,W) float) -> (N,out,H,W)``.
The arithmetic is libwsu (hand-written gfx950 kernels, include/wsu.h); there is no
CPU / eager fallback: calling the model with CPU tensors raises.

Precision modes (``mode=`` or env ``WSU_MODE``):
  'f32'     exact fp32 MFMA                     -- parity anchor (also trains in exact fp32)
  'bf16x3'  split-bf16 MFMA, fp32 storage       -- meets the 1e-4 MAE gate (~2e-6)
  'bf16'    bf16 storage + MFMA                 -- fastest; MAE ~1e-3 on full-range weights
  'bf16x3s' bf16x3 with producer-side split     -- bitwise the results of 'bf16x3', activations stored as hi/lo halves
                                                   between the fused first layer and the fused head (keep= / autograd use 'bf16x3')
  'f16f8p'  the 'f16f8' arithmetic on PLANAR storage -- [n][C/16][4 planes][H][W][16 B], the LDS image of the matrix kernels: staging is a
                                                   pure LDS-DMA and one persistent workgroup per CU pipelines it across chunks and tiles
                                                   (csrc/conv3x3_pl.hip, planar.hip); same values as 'f16f8' up to the accumulation order
  'f16f4p'  (DEFAULT since round 3) the 3x3 convs multiply both cross terms as ONE block-scaled fp4 (e2m1) operand pair per tap pair (14 instead of
            19 matrix units per chunk): MAE 2.1e-5 (the gate is 1e-4) instead of 4e-6.  Since round 4 on planar Q storage (ops.PlanarQ, include/wsu.h
            K1q): every producer's epilogue writes the fp4 granule + scale byte its consumer multiplies, the consumers' loader waves are pure DMA
            (csrc/conv3x3_q.hip); training forwards and the transposed convs keep the e4m3 arithmetic and format (profiles/r03/f16f4p.md, profiles/r04)
  'f16p'    (opt-in) ONE product per tap: f16(w) * f16(x) on the f16 matrix pipe, fp32 accumulation, no cross terms (9 instead of 14 matrix
            units per chunk), activations as two f16 planes (ops.PlanarH, include/wsu.h K1h: 2 bytes per element).  The K1q / K1u kernels
            instantiated for that format; e11 -> 3x3 convs with fused pool and head -> the fused decoder entry for every decoder block (there is
            no two-kernel decoder path: WSU_FUSE_UP and WSU_FUSE_FIRST_Q do not apply).  Its own MAE: meant for trained
            checkpoints; range flag only beyond +-65504.  Trains in 'f16f8p' like 'f16f4p'
  'f16f8q'  'f16f8p' with ONE cross term (the weights' residual) on the first conv of every decoder block: MAE ~4e-5 instead of 4e-6
  'f16f8'   f16 products + fp8 cross terms      -- f16(w)*f16(x) exactly, the two residual cross terms on the block-scaled fp8
                                                   matrix pipe (0.70 of bf16x3's matrix cycles, ~2^-15 relative error per product, MAE
                                                   4e-6 on the full-range test weights); same storage discipline as 'bf16x3s'.
                                                   Activations beyond +-448 fall back to plain f16 accuracy (include/wsu.h): networks
                                                   without the reference's [0,1] inputs can select 'bf16x3s'
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from .. import ops
from .._lib import WsuError

ENC = [("e11", "e12"), ("e21", "e22"), ("e31", "e32"), ("e41", "e42"), ("e51", "e52")]
ENC_CH = [64, 128, 256, 512, 1024]


def dec_names(depth: int):
    """Decoder block that exists iff nsteps >= depth (unet.py:112-132): upconv{5-d}, d{5-d}1, d{5-d}2."""
    k = 5 - depth
    return f"upconv{k}", f"d{k}1", f"d{k}2"


class UniformDropout(nn.Module):
    """Reference unet.py:15-51.  ``p`` is the DROP probability (self.p keeps 1-p like the reference).
    Not gated on ``self.training`` and active even at p == 0 (identity that still rewrites the input
    in place) -- both reference behaviours are kept.  The Bernoulli keep-mask comes from libwsu's
    counter-based hash of (seed, call number, pixel); assign ``next_mask`` to supply one explicitly."""

    def __init__(self, p: float, drop_channel: Sequence[int], seed: int = 0):
        super().__init__()
        self.p = 1 - p
        self.drop_channel = drop_channel
        self.mask = None
        self.next_mask: Optional[torch.Tensor] = None
        self.seed = seed
        self.calls = 0

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        c = list(self.drop_channel)
        mask = self.next_mask
        self.next_mask = None
        if mask is None and self.p >= 1.0:
            # drop probability 0 (what get_pretrained builds, evaluate.py:180): the reference still draws an all-ones mask and rewrites x
            # with itself; here that identity costs no launch (the mask attribute keeps its all-ones value, allocated once per shape)
            shape = (x.shape[0], len(c), x.shape[2], x.shape[3])
            if self.mask is None or tuple(self.mask.shape) != shape or self.mask.device != x.device or not getattr(self, "_mask_is_ones", False):
                self.mask = torch.ones(shape, dtype=torch.float32, device=x.device)
                self._mask_is_ones = True
            self.calls += 1
            return x
        self._mask_is_ones = False
        if mask is not None:
            mask = mask.to(device=x.device, dtype=torch.float32).contiguous()
        src = x if x.is_contiguous() else x.contiguous()
        for ch in c:
            seed = (self.seed * 0x9E3779B97F4A7C15 + self.calls) & 0xFFFFFFFFFFFFFFFF
            y, mask = ops.uniform_dropout(src, mask, channel=ch, keep_prob=self.p, seed=seed, want_mask=True)
            src = y
        self.calls += 1
        self.mask = mask.repeat((1, len(c), 1, 1)) if len(c) > 1 else mask
        x.copy_(src)                      # the reference writes x[:, c] in place (unet.py:41)
        return x


PLANAR_MODES = (ops.MODE_F16F8P, ops.MODE_F16F8Q, ops.MODE_F16F4P, ops.MODE_F16P)
W = ops.MODE_F16F8                                               # the planar paths' weights are packed as for 'f16f8'


def _no_tag(name):
    pass


class _NHWC:
    """What UNet._walk calls to run its layers on NHWC tensors ('f32', 'bf16', 'bf16x3', 'bf16x3s', 'f16f8', 'f16f8x'): the matrix layers in mode
    `m`, e11 and the 1x1 head in `m0` (training: the train mode beside `train_fwd_mode`).  Keep policy: `t` (a dict, or None) receives the
    reference's intermediates; `train` also keeps the 2-bit pool argmax `idx*`, fuses nothing and sets no layer tag."""

    def __init__(self, net, m, m0=None, t=None, train=False, want_logit=False):
        self.net, self.m, self.m0, self.t, self.train, self.want_logit = net, m, m if m0 is None else m0, t, train, want_logit
        self.tag = _no_tag if train else ops.set_layer           # per-layer labels for bench.py's KernelTimer (a global assignment)
        # e11 is folded into e12's input staging unless its output is asked for (xe11 then never reaches HBM)
        self.fold_first = t is None and net.fuse_first and net._single_plane()
        # last layer: d42 + outconv + sigmoid in one launch, xd42 never touches HBM
        self.fused_head = t is None and net.nsteps >= 1 and net.fuse_head and net.outconv.out_channels <= 4

    def first(self, x):
        if self.fold_first:
            return None
        e11 = self.net.e11
        self.tag("e11")
        return ops.conv3x3_first(x, e11.weight.detach(), e11.bias.detach(), self.m0, relu=True)

    def fused_first(self, x):
        net, m = self.net, self.m
        return ops.conv3x3_fused_first(x, net.e11.weight, net.e11.bias.detach(), net._packed("conv", ops.first_layer_weight_mode(m), net.e12),
                                       net.e12.bias.detach(), net.e12.out_channels, m, pool=net.nsteps > 0)

    def conv(self, name, xa, xb=None, pool=0, feeds=None, mask=False):
        layer, m = getattr(self.net, name), self.m
        res = ops.conv3x3(xa, xb, self.net._packed("conv", m, layer), layer.bias.detach(), layer.out_channels, m, pool=bool(pool), pool_idx=self.train)
        if pool and self.train:
            *res, self.t[f"idx{pool}"] = res
        return res

    def enter(self, depth, up, c1, cur, skip):
        lu, m = getattr(self.net, up), self.m
        self.tag(up)
        xu = ops.convt2x2(cur, self.net._packed("convt", m, lu), lu.bias.detach(), lu.out_channels, m)
        self.tag(c1)
        return xu, self.conv(c1, xu, skip)

    def head(self, name, cur):
        layer, oc = getattr(self.net, name), self.net.outconv
        self.tag(name + "+outconv")
        return ops.conv3x3_head(cur, None, self.net._packed("conv", self.m, layer), layer.bias.detach(), oc.weight.detach(), oc.bias.detach(), self.m,
                                want_logit=self.want_logit)

    def outconv(self, cur):
        oc, save = self.net.outconv, self.t is not None and not self.train
        self.tag("outconv")
        res = ops.conv1x1_sigmoid(cur, oc.weight.detach(), oc.bias.detach(), self.m0, want_logit=self.want_logit or save)
        if save:
            self.t["logit"] = res[1]
        return res if self.want_logit or not save else res[0]


class _Planar:
    """What UNet._walk calls to run its layers on planar tensors of ONE storage format `S`, all persistent LDS-DMA kernels; no intermediate leaves
    the format: ops.PLANAR_A ('f16f8p', 'f16f8q' and training: f16 + e4m3 residual), PLANAR_Q ('f16f4p': block-scaled fp4 cross terms, every
    producer's epilogue writes the fp4 granule and scale byte its consumer multiplies) or PLANAR_H ('f16p': two f16 planes, one product per tap).
    The head is always fused into the last 3x3 conv.  Keep policy: `train` keeps in `t` every activation the backward needs, the 1-bit ReLU
    masks `m_x*` of those whose mask a data gradient applies (written by the producing kernel's epilogue, read by the consumer's loaders by
    LDS-DMA: 1/8 byte per element instead of 2) and the last conv's output beside the head's; it fuses nothing else and sets no layer tag."""
    CONV = {ops.PLANAR_A: ("conv3x3_pl", "conv"), ops.PLANAR_Q: ("conv3x3_q", "conv_f4"), ops.PLANAR_H: ("conv3x3_h", "conv_h")}
    UP = {ops.PLANAR_Q: "conv3x3_up_q", ops.PLANAR_H: "conv3x3_up_h"}

    def __init__(self, net, x, t=None, train=False, want_logit=False):
        mode = "f16f8p" if train else net.mode
        self.net, self.t, self.train, self.want_logit = net, t, train, want_logit
        self.S = S = ops.PLANAR_H if mode == "f16p" else ops.PLANAR_Q if mode == "f16f4p" else ops.PLANAR_A
        # 'f16f8q': the first conv of every decoder block (the two most expensive layers of unet_2) multiplies without the activations'
        # residual term: 15 instead of 19 matrix units there, MAE 4e-6 -> ~4e-5 on the gate's weights (still 2.5x inside 1e-4)
        self.quick = mode == "f16f8q"
        self.rf = net._range_flag_tensor(x.device)               # OR-ed by every epilogue that stores an activation beyond the format's range
        self.tag = _no_tag if train else ops.set_layer
        self.fused_head = True
        # e11 folded into e12's launch (its 64 channels are computed by the loader waves of the persistent kernel) for single-plane inputs: an
        # experiment switch of the e4m3 modes (wsu_conv3x3_pl_fused_first_fwd) and of 'f16f4p' (ops.conv3x3_q_fused_first); 'f16p' has none
        switch = {ops.PLANAR_A: net.fuse_first_planar, ops.PLANAR_Q: net.fuse_first_q, ops.PLANAR_H: False}[S]
        self.fold_first = switch and not train and net._single_plane() and net.nsteps >= 1

    def fused_up(self, depth):
        """Decoder block `depth` runs upconv + concat + first conv as one launch: always in format H (it has no two-kernel decoder path), in
        format Q unless switched off (WSU_FUSE_UP=0) or the block is wider than the kernel, never in format A."""
        co = ENC_CH[depth - 1]                                   # the block's width (d*1.out_channels)
        return self.S == ops.PLANAR_H or (self.S == ops.PLANAR_Q and self.net.fuse_up_planar and co <= 512 and co % 64 == 0)

    def first(self, x):
        if self.fold_first:
            return None
        e11 = self.net.e11
        self.tag("e11")
        res = ops.conv3x3_first_pl(x, e11.weight, e11.bias.detach(), range_flag=self.rf, want_mask=self.train, y_format=self.S)
        if self.train:
            res, self.t["m_xe11"] = res
        return res

    def fused_first(self, x):
        net = self.net
        e11, e12 = net.e11, net.e12
        if self.S == ops.PLANAR_Q:                               # e11's weights tap-major: the kernel's scalar loads
            return ops.conv3x3_q_fused_first(x, net._packed("taps", W, e11), None if e11.bias is None else e11.bias.detach(),
                                             net._packed("conv_f4", W, e12), e12.bias.detach(), e12.out_channels, range_flag=self.rf)
        return ops.conv3x3_pl_fused_first(x, e11.weight, e11.bias.detach(), net._packed("conv", W, e12), e12.bias.detach(), e12.out_channels,
                                          pool=True, range_flag=self.rf)

    def conv(self, name, xa, xb=None, pool=0, feeds=None, mask=False, **kw):
        """One 3x3 conv in the format's arithmetic.  feeds: the decoder depth whose transposed conv reads the result (None: a 3x3 conv does);
        mask: training keeps the result's ReLU mask; kw: the fused head's arguments."""
        S, layer = self.S, getattr(self.net, name)
        fn, kind = self.CONV[S]
        if kw.get("want_y", True):                               # a head that stores no y stores no activation
            kw["range_flag"] = self.rf
        if S == ops.PLANAR_Q:                                    # only the tensor a transposed conv of its own reads stays in the e4m3-residual format
            kw["y_format"] = S if feeds is None or self.fused_up(feeds) else ops.PLANAR_A
        elif S == ops.PLANAR_A:
            kw["x_residual"] = xb is None or not self.quick
            kw["want_mask"] = mask and self.train
        res = getattr(ops, fn)(xa, xb, self.net._packed(kind, W, layer), layer.bias.detach(), layer.out_channels, pool=bool(pool), **kw)
        if kw.get("want_mask"):
            res, self.t["m_x" + name] = res
        return res

    def enter(self, depth, up, c1, cur, skip):
        net, lu, l1 = self.net, getattr(self.net, up), getattr(self.net, c1)
        if self.fused_up(depth):
            self.tag(up + "+" + c1)
            return None, getattr(ops, self.UP[self.S])(cur, skip, *net._packed("up", self.S, lu, l1), l1.out_channels, range_flag=self.rf)
        self.tag(up)
        xu = ops.convt2x2_pl(cur, net._packed("convt", W, lu), lu.bias.detach(), lu.out_channels, range_flag=self.rf, y_format=self.S)
        self.tag(c1)
        return xu, self.conv(c1, xu, skip, mask=True)

    def head(self, name, cur):
        oc = self.net.outconv
        self.tag(name + "+outconv")
        res = self.conv(name, cur, want_y=self.train, head_w=oc.weight.detach(), head_b=oc.bias.detach(), want_logit=self.want_logit)
        if self.train:
            res, self.t["x" + name] = res
        return res


class UNet(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, nsteps: int, drop_rate: float,
                 drop_channel: Sequence[int], mode: Optional[str] = None):
        super().__init__()
        assert nsteps >= 0
        if nsteps > 4:
            raise NotImplementedError("the reference defines at most 4 pooling steps (unet.py:85-132)")
        self.nsteps = nsteps
        # DEFAULT MODE POLICY (round 4, VERDICT r03 next #2b).  The library default is the fastest arithmetic that keeps >= 3x margin to the north
        # star's gate (MAE <= 1e-4 of the [0,1] output against the fp32 CPU path) on BOTH weight sets the repository can pin: the full-range 'he'
        # formula weights (tests/test_gpu_forward.py::test_mae_gate_512_batch, bench.py `mae_vs_cpu_oracle`: 2.1e-5) and weights trained by this
        # package's own loop (tests/test_gpu_round4.py::test_mae_gate_on_trained_weights, bench.py `mae_vs_cpu_oracle_trained`: <= 3e-5).  Parity on
        # the PUBLISHED checkpoints is unpinned -- the reference ships none (.MISSING_LARGE_BLOBS:7-12); mode='f16f8p' (MAE 4e-6, ~12 % slower) is
        # the conservative setting one argument away, 'f32' the exact one.  A mode that misses the margin on either set must not become the default.
        self.mode = mode or os.environ.get("WSU_MODE", "f16f4p")
        self.fuse_head = os.environ.get("WSU_FUSE_HEAD", "1") != "0"  # fold outconv + sigmoid into the last 3x3 conv
        self.fuse_first = os.environ.get("WSU_FUSE_FIRST", "1") != "0"  # fold e11 into e12's input staging
        # planar path: e11 computed by the loader waves of e12's kernel (wsu_conv3x3_pl_fused_first_fwd).  Off by default: xe11 never
        # reaches HBM (-2.1 GB at batch 32) but the loaders' VALU work makes them the critical path -- e11 + e12 1.82 -> 1.60 ms, +0.8 % images/s
        self.fuse_first_planar = os.environ.get("WSU_FUSE_FIRST_PL", "0") != "0"
        # default mode: every decoder block's transposed conv + concat + first conv is ONE launch (ops.conv3x3_up_q, csrc/conv3x3_qu.hip); 0 = the
        # two-kernel path (convt2x2_pl -> conv3x3_q), kept as the A/B reference
        self.fuse_up_planar = os.environ.get("WSU_FUSE_UP", "1") != "0"
        # default mode, single-plane inputs, optional (WSU_FUSE_FIRST_Q=1): e11 folded into e12's launch (its 64 channels are computed by the loader
        # waves, bitwise the two-kernel result; ops.conv3x3_q_fused_first).  Measured a tie in time (profiles/r04/ab_fused_first_q.md); it frees
        # xe11's memory (1.4 GB at batch 32 @ 512x512, 5.5 GB at 1024x1024) -- a switch for memory-bound callers, off by default
        self.fuse_first_q = os.environ.get("WSU_FUSE_FIRST_Q", "0") != "0"
        # arithmetic of the autograd path: exact fp32 MFMA for an 'f32' model; 'f16f8p' for a planar model -- the f16f8 arithmetic on planar
        # activations AND gradients (3 bytes per element, model/autograd.py; single-plane inputs, or 2..8 planes with train_planes_planar; falls back to 'bf16x3' otherwise, the input gradient
        # included); else split-bf16 on fp32 tensors (~2^-16 relative per product -- finer than the TF32 convs PyTorch
        # trains with by default on the reference's GPUs)
        self.train_mode = os.environ.get("WSU_TRAIN_MODE") or ("f32" if self.mode == "f32" else "f16f8p" if self.mode in ("f16f8p", "f16f8q", "f16f4p", "f16p") else "bf16x3")
        # train_mode 'f16f8p': the terms the BACKWARD matrix kernels (3x3 data and weight gradients) multiply -- 'f16' (default: exact products of
        # the operands' f16 parts, fp32 accumulation; include/wsu.h WSU_PRODUCTS_*) or 'f16f8' (+ both residual cross terms, the forward's
        # arithmetic).  The forward -- loss, predictions, ReLU masks -- is the same.  Why 'f16' is enough (profiles/r03/
        # train_products.md): a gradient element is a sum of 10^3 .. 10^7 products whose operand roundings (2^-12 relative, unbiased) average
        # out -- <= 2e-4 relative L2 per kernel on zero-mean random operands, the worst case -- while the forward's own rounding already puts
        # ~1e-3 between any two arithmetics through ReLU-mask flips; 300 AdamW steps track exact fp32 as closely as 'f16f8' does.
        # train_mode 'f16f8p' with 2..8 input planes (side-information planes): True trains on the planar path too (first-layer weight gradient:
        # ops.conv3x3_first_pl_bwd_weight_planes), False (default) on the fp32-storage fallback, as every multi-plane model did before the
        # planar path took them.  ws_unet_amd.train decides for its own models.
        self.train_planes_planar = False
        # (parity_oracle, demosaic_oracle): the side-information planes this network's input carries behind the image (ops.side_planes);
        # set by evaluate.get_pretrained and ws_unet_amd.train from the run's config, read by unet_run.unet_plane / evaluate.infere_single
        self.side_planes = (False, False)
        self.train_products = os.environ.get("WSU_TRAIN_PRODUCTS") or "f16"
        ops.products_id(self.train_products)
        # matrix layers of the training FORWARD when train_mode is 'bf16x3': 'f16f8x' (default) or 'bf16x3'
        self.train_fwd_mode = os.environ.get("WSU_TRAIN_FWD_MODE") or "f16f8x"
        self.train_bwd_mode = os.environ.get("WSU_TRAIN_BWD_MODE") or "f16f8x"     # data-gradient 3x3 convs: 'f16f8x' or 'bf16x3'
        ops.mode_id(self.mode)                                    # validate early
        if self.mode == "f16f8x":
            raise ValueError("'f16f8x' is the arithmetic of the training forward (fp32 tensors); the inference mode is 'f16f8'")
        conv_kw = {"kernel_size": 3, "padding": 1, "padding_mode": "reflect"}
        ups_kw = {"kernel_size": 2, "stride": 2}
        if drop_rate is not None:
            self.input_dropout = UniformDropout(p=drop_rate, drop_channel=drop_channel)
        else:
            self.input_dropout = None
        # registration order == reference (unet.py:82-135) so that state_dict order and default-init RNG
        # consumption match: encoder levels first, then decoder from the deepest block up, then outconv
        cin = in_channels
        for lvl in range(nsteps + 1):
            a, b = ENC[lvl]
            if lvl >= 1:
                setattr(self, f"pool{lvl}", nn.MaxPool2d(kernel_size=2, stride=2))
            setattr(self, a, nn.Conv2d(cin, ENC_CH[lvl], **conv_kw))
            setattr(self, b, nn.Conv2d(ENC_CH[lvl], ENC_CH[lvl], **conv_kw))
            cin = ENC_CH[lvl]
        for depth in range(4, 0, -1):
            if nsteps >= depth:
                up, c1, c2 = dec_names(depth)
                hi, lo = ENC_CH[depth], ENC_CH[depth - 1]
                setattr(self, up, nn.ConvTranspose2d(hi, lo, **ups_kw))
                setattr(self, c1, nn.Conv2d(hi, lo, **conv_kw))
                setattr(self, c2, nn.Conv2d(lo, lo, **conv_kw))
        self.outconv = nn.Conv2d(64, out_channels, kernel_size=1, padding_mode="reflect")
        self._pack_cache: Dict[tuple, tuple] = {}

    # ---- packed-weight cache (re-packed only when a parameter was modified) -------------------------
    _PACKERS = {
        "conv_f4": lambda mode, w: ops.pack_conv3x3_f4(w),
        "conv_h": lambda mode, w: ops.pack_conv3x3_h(w),
        "conv": lambda mode, w: ops.pack_conv3x3(w, mode),
        "dgrad": lambda mode, w: ops.pack_conv3x3(w, mode, dgrad=True),
        "ring": lambda mode, w: ops.pack_conv3x3_ring(w),
        # e11's weights tap-major (9, 64): the scalar loads of ops.conv3x3_q_fused_first
        "taps": lambda mode, w: w.detach().reshape(w.shape[0], 9).t().contiguous(),
        "convt_dgrad_pl": lambda mode, w: ops.pack_convt2x2_pl_dgrad(w),
        "convt_dgrad": lambda mode, w: ops.pack_convt2x2_dgrad(w, mode),
        "convt": lambda mode, w: ops.pack_convt2x2(w, mode),
        # (w_skip_packed, w_low_packed, bias) of the fused decoder-block entry; `mode` is the planar format
        "up": lambda fmt, wu, bu, w1, b1: (ops.pack_conv3x3_up_h if fmt == ops.PLANAR_H else ops.pack_conv3x3_up)(w1, wu, bu, b1),
    }

    def _packed(self, kind: str, mode: int, *layers):
        """The `kind` packing (_PACKERS) in `mode` of one layer's weight or, kind 'up', of a decoder block's transposed conv and first conv, biases
        included.  Cached on (version, address, device) of every parameter it reads."""
        if kind == "up":
            params = (layers[0].weight, layers[0].bias, layers[1].weight, layers[1].bias)
        else:
            params = (layers[0].weight,)
        tag = []
        for p in params:
            tag += (p._version, p.data_ptr(), p.device)
        key = (kind, mode) + layers
        hit = self._pack_cache.get(key)
        if hit is None or hit[0] != tag:
            hit = self._pack_cache[key] = (tag, self._PACKERS[kind](mode, *params))
        return hit[1]

    def _check_input(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda or not self.outconv.weight.is_cuda:
            raise WsuError("ws_unet_amd.UNet runs on an MI355X only: move the model and its input to 'cuda' "
                           "(there is deliberately no CPU fallback)")
        if x.dim() != 4 or x.shape[1] != self.e11.weight.shape[1]:
            raise ValueError(f"expected input (N,{self.e11.weight.shape[1]},H,W), got {tuple(x.shape)}")
        div = 2 ** self.nsteps
        if x.shape[2] % div or x.shape[3] % div:
            raise ValueError(f"H and W must be divisible by {div} for unet_{self.nsteps} (skip concat, unet.py:178,184)")
        if min(x.shape[2], x.shape[3]) // div < 2:
            raise ValueError("input too small: reflect padding needs every level to be at least 2x2")
        return x

    def forward_features(self, x: torch.Tensor, keep: Optional[dict] = None, want_logit: bool = False):
        """Inference forward.  ``keep`` (optional dict) receives every intermediate as an NHWC tensor,
        named as in the reference's forward (xe11 ... xd42, xp*, xu*)."""
        m = ops.mode_id(self.mode)
        save = keep is not None
        if m in PLANAR_MODES and not save and self._planar_ok():
            res = self._walk(x, _Planar(self, x, want_logit=want_logit))
            if not getattr(self, "_range_checked", False):
                # first planar forward of this model: one synchronising look at the range flag.  Weights whose activations leave
                # the format's full-accuracy range (nobody knows that of a foreign checkpoint) fall back LOUDLY to fp32-range storage.
                self._range_checked = True
                if self.range_exceeded():
                    import logging
                    if self.mode == "f16p":
                        logging.warning("ws_unet_amd.UNet: activations beyond +-65504 in mode 'f16p' (not a finite f16); "
                                        "switching this model to mode 'bf16x3s'")
                    else:
                        logging.warning("ws_unet_amd.UNet: activations beyond +-448 in mode 'f16f8p' (the e4m3 residual saturates there); "
                                        "switching this model to mode 'bf16x3s'")
                    self.mode = "bf16x3s"
                    self._range_switched = True                # (a sharded pass tells the other ranks: unet_run.range_fallback)
                    return self.forward_features(x, keep, want_logit)
            return res
        if m in PLANAR_MODES:
            m = ops.MODE_BF16X3                 # intermediates are only kept in fp32 NHWC; odd channel counts take the general path
        if m in (ops.MODE_BF16X3S, ops.MODE_F16F8) and (save or self.nsteps < 1 or not (self.fuse_first and self.fuse_head)
                                                       or not self._single_plane() or self.outconv.out_channels > 4):
            m = ops.MODE_BF16X3                 # the split formats live only between the fused first layer and the fused head
        return self._walk(x, _NHWC(self, m, t=keep, want_logit=want_logit))

    def _walk(self, x: torch.Tensor, A):
        """The reference's forward (unet.py:137-189), written once for every arithmetic and for training: `A` (_NHWC or _Planar above) runs each
        layer, decides what is fused and keeps in `A.t` what its keep policy adds; the reference's intermediates are kept here, under the
        reference's names.  Returns what the head returns."""
        ns, tag, t = self.nsteps, A.tag, A.t
        skips: List = []
        cur = A.first(x)                                           # None: e11 runs inside e12's launch
        if t is not None:
            t["xe11"] = cur
        for lvl in range(ns + 1):
            a, b = ENC[lvl]
            if lvl == 0 and cur is None:
                tag("e11+e12")
                res = A.fused_first(x)
                if ns > 0:
                    skips.append(res[0])
                    cur = res[1]
                else:
                    cur = res
                continue
            if lvl >= 1:
                tag(a)
                cur = A.conv(a, cur, mask=True)
                if t is not None:
                    t["x" + a] = cur
            tag(b)
            if lvl < ns:
                full, cur = A.conv(b, cur, pool=lvl + 1)
                skips.append(full)
            elif ns == 0 and A.fused_head:
                return A.head(b, cur)
            else:
                full = cur = A.conv(b, cur, feeds=ns)              # feeds the transposed conv
            if t is not None:
                t["x" + b] = full
                if lvl < ns:
                    t[f"xp{lvl + 1}"] = cur
        for depth in range(ns, 0, -1):
            up, c1, c2 = dec_names(depth)
            xu, cur = A.enter(depth, up, c1, cur, skips[depth - 1])  # transposed conv + first conv, or the fused entry (xu is None)
            if t is not None:
                t["xu" + up[-1]], t["x" + c1] = xu, cur
            if depth == 1 and A.fused_head:
                return A.head(c2, cur)
            tag(c2)
            cur = A.conv(c2, cur, feeds=depth - 1)                 # feeds the next transposed conv
            if t is not None:
                t["x" + c2] = cur
        return A.outconv(cur)

    def _range_flag_tensor(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:           # 'cuda' and 'cuda:0' name the same card: do not replace a live flag word
            device = torch.device("cuda", torch.cuda.current_device())
        rf = getattr(self, "_range_flag", None)
        if rf is None or rf.device != device:
            rf = self._range_flag = torch.zeros(1, dtype=torch.int32, device=device)
        return rf

    def range_exceeded(self, clear: bool = True) -> bool:
        """True if, since the last call, a planar ('f16f8p') forward stored an activation beyond +-448 -- where the format's e4m3 residual
        saturates and that value keeps only f16 accuracy (NaN / Inf count too); in mode 'f16p' only beyond +-65504 (not a finite f16).  One device word OR-ed by the kernels' epilogues; reading
        it synchronises.  A network that trips it should run in mode 'bf16x3s' (fp32-range storage)."""
        rf = getattr(self, "_range_flag", None)
        if rf is None:
            return False
        hit = bool(rf.item())
        if clear and hit:
            rf.zero_()
        return hit

    def _single_plane(self) -> bool:
        return self.e11.in_channels == 1 and self.e11.out_channels == 64

    def _planar_ok(self) -> bool:
        """The planar path needs <= 8 input planes, at most 4 head planes and the reference's channel ladder (multiples of 64)."""
        e11, oc = self.e11, self.outconv
        return e11.in_channels <= 8 and oc.out_channels <= 4 and oc.in_channels == 64 and e11.out_channels % 16 == 0

    def forward(self, x_in: torch.Tensor) -> torch.Tensor:
        x_in = self._check_input(x_in)
        if x_in.shape[0] == 0:                                     # empty batch: nothing to launch (torch returns an empty tensor too)
            return x_in.new_zeros((0, self.outconv.out_channels) + tuple(x_in.shape[2:]), dtype=torch.float32)
        if self.input_dropout is not None:
            x_in = self.input_dropout(x_in)
        x = x_in if (x_in.dtype == torch.float32 and x_in.is_contiguous()) else x_in.float().contiguous()
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if needs_grad:
            from .autograd import unet_apply           # training path: the same walk, keeping what the backward reads
            return unet_apply(self, x)
        return self.forward_features(x)

    def to(self, *args, **kw):
        # the reference's override (unet.py:191-194) dereferences input_dropout unconditionally and crashes when it
        # is None; that accident is not reproduced.
        super().to(*args, **kw)
        return self

    def disable_center_pixels(self):
        """unet.py:196-199."""
        self.e11.weight.data[:, :, 1, 1] = 0.
        if self.e11.weight.grad is not None:
            self.e11.weight.grad[:, :, 1, 1] = 0.
        self.invalidate_packed()

    def invalidate_packed(self, recheck_range: bool = True):
        """Drop cached packed weights.  Needed only after writing through ``param.data`` (which bypasses
        the tensor version counter the cache keys on); optimizer steps and load_state_dict are detected.
        New weights also mean a new activation range: the planar modes' one-time look at the +-448 range flag is re-armed
        (``recheck_range=False``: the optimiser's per-step call -- the trainer reads the flag once per epoch instead)."""
        self._pack_cache.clear()
        if recheck_range:
            self._range_checked = False
            self._range_checked_train = False

    def load_state_dict(self, *args, **kw):
        res = super().load_state_dict(*args, **kw)
        self.invalidate_packed()                                   # a foreign checkpoint: nobody knows its activation range
        return res
