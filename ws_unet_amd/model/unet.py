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
        # activations AND gradients (3 bytes per element, model/autograd.py; single-plane inputs, falls back to 'bf16x3' otherwise and when the
        # input gradient is asked for); else split-bf16 on fp32 tensors (~2^-16 relative per product -- finer than the TF32 convs PyTorch
        # trains with by default on the reference's GPUs)
        self.train_mode = os.environ.get("WSU_TRAIN_MODE") or ("f32" if self.mode == "f32" else "f16f8p" if self.mode in ("f16f8p", "f16f8q", "f16f4p", "f16p") else "bf16x3")
        # train_mode 'f16f8p': the terms the BACKWARD matrix kernels (3x3 data and weight gradients) multiply -- 'f16' (default: exact products of
        # the operands' f16 parts, fp32 accumulation; include/wsu.h WSU_PRODUCTS_*) or 'f16f8' (+ both residual cross terms, the forward's
        # arithmetic).  The forward -- loss, predictions, ReLU masks -- is the same.  Why 'f16' is enough (profiles/r03/
        # train_products.md): a gradient element is a sum of 10^3 .. 10^7 products whose operand roundings (2^-12 relative, unbiased) average
        # out -- <= 2e-4 relative L2 per kernel on zero-mean random operands, the worst case -- while the forward's own rounding already puts
        # ~1e-3 between any two arithmetics through ReLU-mask flips; 300 AdamW steps track exact fp32 as closely as 'f16f8' does.
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
        "conv_f4": lambda p, mode: ops.pack_conv3x3_f4(p),
        "conv_h": lambda p, mode: ops.pack_conv3x3_h(p),
        "conv": ops.pack_conv3x3,
        "dgrad": lambda p, mode: ops.pack_conv3x3(p, mode, dgrad=True),
        "ring": lambda p, mode: ops.pack_conv3x3_ring(p),
        # e11's weights tap-major (9, 64): the scalar loads of ops.conv3x3_q_fused_first
        "taps": lambda p, mode: p.detach().reshape(p.shape[0], 9).t().contiguous(),
        "convt_dgrad_pl": lambda p, mode: ops.pack_convt2x2_pl_dgrad(p),
        "convt_dgrad": ops.pack_convt2x2_dgrad,
        "convt": ops.pack_convt2x2,
    }
    _UP_PACKERS = {ops.PLANAR_Q: ops.pack_conv3x3_up, ops.PLANAR_H: ops.pack_conv3x3_up_h}

    def _packed(self, name: str, mode: int, kind: str) -> torch.Tensor:
        p = getattr(self, name).weight
        key = (name, mode, kind)
        tag = (p._version, p.data_ptr(), p.device)
        hit = self._pack_cache.get(key)
        if hit is not None and hit[0] == tag:
            return hit[1]
        packed = self._PACKERS[kind](p, mode)
        self._pack_cache[key] = (tag, packed)
        return packed

    def _packed_up(self, up: str, c1: str, fmt: int = ops.PLANAR_Q):
        """(w_skip_packed, w_low_packed, bias) of the fused decoder-block entry (ops.pack_conv3x3_up; fmt PLANAR_H: ops.pack_conv3x3_up_h), cached
        on all four parameters' versions."""
        lu, l1 = getattr(self, up), getattr(self, c1)
        ps = (lu.weight, lu.bias, l1.weight, l1.bias)
        key = (up, c1, "up", fmt)
        tag = tuple((p._version, p.data_ptr(), p.device) for p in ps)
        hit = self._pack_cache.get(key)
        if hit is not None and hit[0] == tag:
            return hit[1]
        packed = self._UP_PACKERS[fmt](l1.weight, lu.weight, lu.bias, l1.bias)
        self._pack_cache[key] = (tag, packed)
        return packed

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
        t = keep if keep is not None else {}
        save = keep is not None
        e11 = self.e11
        if m in (ops.MODE_F16F8P, ops.MODE_F16F8Q, ops.MODE_F16F4P, ops.MODE_F16P):
            if save or not self._planar_ok():
                m = ops.MODE_BF16X3             # intermediates are only kept in fp32 NHWC; odd channel counts take the general path
            else:
                res = self._forward_planar(x, want_logit)
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
                        self._range_switched = True                # (a sharded pass tells the other ranks: evaluate.range_fallback)
                        return self.forward_features(x, keep, want_logit)
                return res
        if m in (ops.MODE_BF16X3S, ops.MODE_F16F8) and (save or self.nsteps < 1 or not (self.fuse_first and self.fuse_head)
                                     or e11.in_channels != 1 or e11.out_channels != 64 or self.outconv.out_channels > 4):
            m = ops.MODE_BF16X3             # the split formats live only between the fused first layer and the fused head
        # e11 is folded into e12's input staging unless its output is asked for (xe11 then never reaches HBM)
        fuse_first = self.fuse_first and not save and e11.in_channels == 1 and e11.out_channels == 64
        cur = None
        tag = ops.set_layer                                        # per-layer labels for bench.py's KernelTimer (a global assignment)
        if not fuse_first:
            tag("e11")
            cur = ops.conv3x3_first(x, e11.weight.detach(), e11.bias.detach(), m, relu=True)
        if save:
            t["xe11"] = cur
        skips: List[torch.Tensor] = []
        oc_fusable = self.fuse_head and self.outconv.out_channels <= 4
        for lvl in range(self.nsteps + 1):
            a, b = ENC[lvl]
            if lvl == 0 and fuse_first:
                lb = self.e12
                tag("e11+e12")
                res = ops.conv3x3_fused_first(x, e11.weight, e11.bias.detach(), self._packed("e12", ops.first_layer_weight_mode(m), "conv"), lb.bias.detach(),
                                              lb.out_channels, m, pool=self.nsteps > 0)
                if self.nsteps > 0:
                    skips.append(res[0])
                    cur = res[1]
                else:
                    cur = res
                continue
            if lvl >= 1:
                la = getattr(self, a)
                tag(a)
                cur = ops.conv3x3(cur, None, self._packed(a, m, "conv"), la.bias.detach(), la.out_channels, m)
                if save:
                    t["x" + a] = cur
            lb = getattr(self, b)
            tag(b)
            if lvl < self.nsteps:
                full, cur = ops.conv3x3(cur, None, self._packed(b, m, "conv"), lb.bias.detach(), lb.out_channels, m, pool=True)
                skips.append(full)
                if save:
                    t["x" + b] = full
                    t[f"xp{lvl + 1}"] = cur
            else:
                cur = ops.conv3x3(cur, None, self._packed(b, m, "conv"), lb.bias.detach(), lb.out_channels, m)
                if save:
                    t["x" + b] = cur
        for depth in range(self.nsteps, 0, -1):
            up, c1, c2 = dec_names(depth)
            lu, l1, l2 = getattr(self, up), getattr(self, c1), getattr(self, c2)
            tag(up)
            xu = ops.convt2x2(cur, self._packed(up, m, "convt"), lu.bias.detach(), lu.out_channels, m)
            skip = skips[depth - 1]
            tag(c1)
            cur = ops.conv3x3(xu, skip, self._packed(c1, m, "conv"), l1.bias.detach(), l1.out_channels, m)
            if save:
                t["xu" + up[-1]] = xu
                t["x" + c1] = cur
            if depth == 1 and not save and oc_fusable:
                # last layer: d42 + outconv + sigmoid in one launch, xd42 never touches HBM
                tag(c2 + "+outconv")
                return ops.conv3x3_head(cur, None, self._packed(c2, m, "conv"), l2.bias.detach(),
                                        self.outconv.weight.detach(), self.outconv.bias.detach(), m, want_logit=want_logit)
            tag(c2)
            cur = ops.conv3x3(cur, None, self._packed(c2, m, "conv"), l2.bias.detach(), l2.out_channels, m)
            if save:
                t["x" + c2] = cur
        oc = self.outconv
        tag("outconv")
        res = ops.conv1x1_sigmoid(cur, oc.weight.detach(), oc.bias.detach(), m, want_logit=want_logit or save)
        if want_logit or save:
            out, logit = res
            if save:
                t["logit"] = logit
            return (out, logit) if want_logit else out
        return res

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

    def _planar_ok(self) -> bool:
        """The planar path needs <= 8 input planes, at most 4 head planes and the reference's channel ladder (multiples of 64)."""
        return self.e11.in_channels <= 8 and self.outconv.out_channels <= 4 and self.outconv.in_channels == 64 and self.e11.out_channels % 16 == 0

    def _forward_planar(self, x: torch.Tensor, want_logit: bool = False):
        """unet.py:137-189 on planar F16F8P activations: e11 (VALU) -> 3x3 convs with fused pool / concat / head and transposed convs, all
        persistent LDS-DMA kernels; no intermediate leaves the format.  Mode 'f16p': planar H tensors throughout, every decoder block through
        the fused entry ops.conv3x3_up_h (WSU_FUSE_UP and WSU_FUSE_FIRST_Q are ignored: the mode has no two-kernel decoder path)."""
        W = ops.MODE_F16F8                                           # weights are packed as for 'f16f8'
        # 'f16f8q': the first conv of every decoder block (the two most expensive layers of unet_2) multiplies without the activations'
        # residual term: 15 instead of 19 matrix units there, MAE 4e-6 -> ~4e-5 on the gate's weights (still 2.5x inside 1e-4)
        quick = self.mode == "f16f8q"
        # 'f16f4p' (default): block-scaled fp4 cross terms on planar Q tensors (ops.PlanarQ; csrc/conv3x3_q.hip): every producer's epilogue writes
        # the fp4 granule and scale byte its consumer multiplies; only the two tensors the transposed convs read stay in the e4m3-residual format
        q4 = self.mode == "f16f4p"
        # 'f16p': the walk of 'f16f4p' on planar H tensors (ops.PlanarH), the fused entry for every decoder block, no format-A tensor anywhere
        h16 = self.mode == "f16p"
        CK = "conv_h" if h16 else "conv_f4" if q4 else "conv"
        A = ops.PLANAR_A
        S = ops.PLANAR_H if h16 else ops.PLANAR_Q                    # the storage format between the layers of the 'f16f4p' / 'f16p' walk
        tag = ops.set_layer
        e11 = self.e11
        rf = self._range_flag_tensor(x.device)

        def conv(xa, xb, name, layer, fmt=S, xres=True, **kw):       # one 3x3 conv of the planar path in this mode's arithmetic
            if h16:
                return ops.conv3x3_h(xa, xb, self._packed(name, W, CK), layer.bias.detach(), layer.out_channels, **kw)
            if q4:
                return ops.conv3x3_q(xa, xb, self._packed(name, W, CK), layer.bias.detach(), layer.out_channels, y_format=fmt, **kw)
            return ops.conv3x3_pl(xa, xb, self._packed(name, W, CK), layer.bias.detach(), layer.out_channels, x_residual=xres, **kw)

        def fuse_up(depth):                                          # decoder block `depth` runs upconv + concat + first conv as one launch
            l1 = getattr(self, dec_names(depth)[1])
            return h16 or (q4 and self.fuse_up_planar and l1.out_channels <= 512 and l1.out_channels % 64 == 0)

        # e11 is folded into e12 (its 64 channels are computed by the loader waves of the persistent kernel) for single-plane inputs -- an
        # experiment switch of the e4m3 modes (the fused kernel multiplies e4m3 cross terms and writes the e4m3-residual format)
        fuse_first = self.fuse_first_planar and not (q4 or h16) and e11.in_channels == 1 and e11.out_channels == 64 and self.nsteps >= 1
        fuse_first_q = q4 and self.fuse_first_q and e11.in_channels == 1 and e11.out_channels == 64 and self.nsteps >= 1 and self.e12.in_channels == 64
        cur = None
        if not fuse_first and not fuse_first_q:
            tag("e11")
            cur = ops.conv3x3_first_pl(x, e11.weight, e11.bias.detach(), range_flag=rf, y_format=S if (q4 or h16) else A)
        skips: List = []
        for lvl in range(self.nsteps + 1):
            a, b = ENC[lvl]
            if lvl == 0 and fuse_first_q:
                lb = self.e12
                tag("e11+e12")
                full, cur = ops.conv3x3_q_fused_first(x, self._packed("e11", W, "taps"), None if e11.bias is None else e11.bias.detach(),
                                                      self._packed("e12", W, CK), lb.bias.detach(), lb.out_channels, range_flag=rf)
                skips.append(full)
                continue
            if lvl == 0 and fuse_first:
                lb = self.e12
                tag("e11+e12")
                full, cur = ops.conv3x3_pl_fused_first(x, e11.weight, e11.bias.detach(), self._packed("e12", W, "conv"), lb.bias.detach(),
                                                       lb.out_channels, pool=True, range_flag=rf)
                skips.append(full)
                continue
            if lvl >= 1:
                la = getattr(self, a)
                tag(a)
                cur = conv(cur, None, a, la, range_flag=rf)
            lb = getattr(self, b)
            tag(b)
            last = lvl == self.nsteps
            if last and self.nsteps == 0:
                tag(b + "+outconv")
                return conv(cur, None, b, lb, want_y=False, head_w=self.outconv.weight.detach(), head_b=self.outconv.bias.detach(), want_logit=want_logit)
            if not last:
                full, cur = conv(cur, None, b, lb, pool=True, range_flag=rf)
                skips.append(full)
            else:
                cur = conv(cur, None, b, lb, fmt=S if fuse_up(self.nsteps) else A, range_flag=rf)        # feeds the transposed conv
        for depth in range(self.nsteps, 0, -1):
            up, c1, c2 = dec_names(depth)
            lu, l1, l2 = getattr(self, up), getattr(self, c1), getattr(self, c2)
            if fuse_up(depth):
                tag(up + "+" + c1)
                cur = (ops.conv3x3_up_h if h16 else ops.conv3x3_up_q)(cur, skips[depth - 1], *self._packed_up(up, c1, S), l1.out_channels, range_flag=rf)
            else:
                tag(up)
                xu = ops.convt2x2_pl(cur, self._packed(up, W, "convt"), lu.bias.detach(), lu.out_channels, range_flag=rf, y_format=S if q4 else A)
                tag(c1)
                cur = conv(xu, skips[depth - 1], c1, l1, xres=not quick, range_flag=rf)
            if depth == 1:
                tag(c2 + "+outconv")
                return conv(cur, None, c2, l2, want_y=False, head_w=self.outconv.weight.detach(), head_b=self.outconv.bias.detach(), want_logit=want_logit)
            tag(c2)
            cur = conv(cur, None, c2, l2, fmt=S if fuse_up(depth - 1) else A, range_flag=rf)           # feeds the next transposed conv
        raise AssertionError("unreachable")

    def forward(self, x_in: torch.Tensor) -> torch.Tensor:
        x_in = self._check_input(x_in)
        if x_in.shape[0] == 0:                                     # empty batch: nothing to launch (torch returns an empty tensor too)
            return x_in.new_zeros((0, self.outconv.out_channels) + tuple(x_in.shape[2:]), dtype=torch.float32)
        if self.input_dropout is not None:
            x_in = self.input_dropout(x_in)
        x = x_in if (x_in.dtype == torch.float32 and x_in.is_contiguous()) else x_in.float().contiguous()
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if needs_grad:
            from .autograd import unet_apply           # training path (exact fp32 kernels + saved activations)
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
