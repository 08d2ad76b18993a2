"""Training path of the UNet: one torch.autograd.Function whose forward and backward are libwsu kernels.

The reference has no hand-written backward -- it relies on autograd through
src/unet/model/unet.py:137-189.  Here the whole network is ONE autograd node: the forward is UNet._walk keeping the activations, the backward
(_backward below) walks the layers in reverse calling the K7 kernels (include/wsu.h).  `model.train_mode` picks the path:
  'f16f8p'  (default for planar models) activations AND gradients in the planar three-plane layout (3 bytes per element), the f16f8
            arithmetic in forward, data gradient and weight gradient (unet._Planar / _PlanarBwd); single-plane inputs, and inputs of 2..8
            planes (side-information planes) when the model carries `train_planes_planar = True` -- other multi-plane inputs fall
            back to 'bf16x3';
  'bf16x3'  fp32 NHWC tensors; the matrix kernels run the f16f8 arithmetic on them (`train_fwd_mode` / `train_bwd_mode` = 'f16f8x', default:
            exact f16 products + fp8 cross terms, ~2^-15 relative, 0.7 of bf16x3's matrix cycles) or split-bf16; 2-bit pool argmax saved by
            the forward;
  'f32'     exact fp32 on the matrix cores.
Bias gradients are fp32 sums in every mode.  The gradient w.r.t. the network input (saliency, src/saliency.py:159-174) is produced when
`x.requires_grad`, in every mode.

Conventions inside backward: `g` is the PRE-activation gradient of the layer being processed; every kernel
that produces the gradient w.r.t. a post-ReLU activation applies that activation's ReLU mask itself
(relu'(0) = 0 as in PyTorch), so `g` can be fed straight to the next weight / data gradient.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from .. import ops
from .unet import ENC, W, _NHWC, _Planar, dec_names


def _param_list(model) -> List[torch.nn.Parameter]:
    return [p for _, p in model.named_parameters()]


class _NHWCBwd:
    """The eight kernels of _backward on fp32 NHWC operands.  Weight gradients and the 3x3 data gradients run in `mb`: train_bwd_mode 'f16f8x'
    for a split-bf16 run (the f16f8 arithmetic on the fp32 tensors), else the train mode `m`; the transposed conv's data gradient runs in `m`.
    Gradients of a mean-reduced loss sit far below f16's normal range, so an 'f16f8x' backward runs on gradients scaled by a power of two
    (`scaled`).  The concat's skip half is masked by the data gradient (mask2); the pool routes through the saved argmax."""

    def __init__(self, net, m):
        self.net, self.m = net, m
        self.scaled = m == ops.MODE_BF16X3 and (getattr(net, "train_bwd_mode", None) or "f16f8x") == "f16f8x"
        self.mb = ops.MODE_F16F8X if self.scaled else m

    def head(self, t, dout):
        return ops.conv1x1_sigmoid_bwd(t["last"], self.net.outconv.weight, t["out"], dout)

    def conv_w(self, g, x1, x2):
        return ops.conv3x3_bwd_weight(g, x1, x2, mode=self.mb)

    def conv_d(self, name, g, x1, mask1, mask2, bits):
        layer = getattr(self.net, name)
        return ops.conv3x3_bwd_data(g, self.net._packed("dgrad", self.mb, layer), layer.weight, x1.shape[3], mask1, mask2, self.mb)

    def convt_w(self, below, dxu):
        return ops.convt2x2_bwd_weight(below, dxu, mode=self.mb)

    def convt_d(self, up, dxu, below):
        lu = getattr(self.net, up)
        return ops.convt2x2_bwd_data(dxu, self.net._packed("convt_dgrad", self.m, lu), lu.in_channels, below, self.m)

    def pool(self, skip_g, g, t, lvl):       # g: the gradient w.r.t. the pooled tensor xp{lvl+1}, routed onto the argmax and added to the skip path
        return ops.maxpool2x2_bwd(skip_g, g, t[f"idx{lvl + 1}"], t[f"xp{lvl + 1}"])

    def first_w(self, g, x):
        return ops.conv3x3_first_bwd_weight(g, x)

    def first_d(self, g, w):
        return ops.conv3x3_first_bwd_data(g, w)


class _PlanarBwd:
    """The eight kernels of _backward for train_mode 'f16f8p': every gradient tensor planar (f16 + e4m3 residual), ALWAYS pre-scaled by a power of
    two; data gradients through the persistent LDS-DMA conv kernel (packed kinds 'dgrad' + 'ring'), weight gradients from planar operands, all
    multiplying the terms `train_products` names (wsu.h WSU_PRODUCTS_*).  The 3x3 data gradient takes the 1-bit mask plane of its input
    (mask1_bits) and masks neither half of the concat: the skip's mask meets the pool routing in maxpool2x2_pl_bwd."""
    scaled = True

    def __init__(self, net):
        self.net, self.kw = net, {"products": getattr(net, "train_products", "f16f8")}

    def head(self, t, dout):
        return ops.conv1x1_sigmoid_pl_bwd(t["last"], self.net.outconv.weight, t["out"], dout, **self.kw)

    def conv_w(self, g, x1, x2):
        return ops.conv3x3_pl_bwd_weight(g, x1, x2, **self.kw)

    def conv_d(self, name, g, x1, mask1, mask2, bits):
        net, layer = self.net, getattr(self.net, name)
        return ops.conv3x3_pl_bwd_data(g, net._packed("dgrad", W, layer), net._packed("ring", W, layer), layer.in_channels,
                                       x1.shape[1] * 16, mask1, None, mask1_bits=bits, **self.kw)

    def convt_w(self, below, dxu):
        return ops.convt2x2_pl_bwd_weight(below, dxu, **self.kw)

    def convt_d(self, up, dxu, below):
        lu = getattr(self.net, up)
        return ops.convt2x2_pl_bwd_data(dxu, self.net._packed("convt_dgrad_pl", W, lu), lu.in_channels, below, **self.kw)

    def pool(self, skip_g, g, t, lvl):
        return ops.maxpool2x2_pl_bwd(skip_g, g, t["x" + ENC[lvl][1]], **self.kw)

    def first_w(self, g, x):
        if x.shape[1] > 1:
            return ops.conv3x3_first_pl_bwd_weight_planes(g, x, **self.kw)
        return ops.conv3x3_first_pl_bwd_weight(g, x, **self.kw)

    def first_d(self, g, w):
        return ops.conv3x3_first_pl_bwd_data(g, w, **self.kw)


def _backward(B, model, t: Dict[str, torch.Tensor], x: torch.Tensor, dout: torch.Tensor, want_dx: bool) -> Dict[str, torch.Tensor]:
    """The reverse walk, once for both tables (B: _NHWCBwd or _PlanarBwd): head, decoder blocks from depth 1 upward, encoder levels downward
    with pool routing and skip gradients.  Returns the parameter gradients by name and the input gradient as '__dx__'."""
    grads: Dict[str, torch.Tensor] = {}
    scale = None
    if B.scaled:
        # max |dout| * scale in (2, 4]: 2^14 of headroom below f16's largest value for gradients that grow on the way down, while values
        # 2^-27 of that maximum still keep an absolute error below theirs (f16 subnormal spacing 2^-24 + the e4m3 residual).  Every kernel on
        # the way is linear in the gradient; ReLU masks and pool routing ignore the scale.  Computed on the device: no host synchronisation
        scale = ops.pow2_grad_scale(dout)                          # device {scale, 1 / scale}
        dout = ops.scale_by(dout, scale[0:1])

    def conv_bwd(name, g, x1, x2, mask1, mask2=None, bits=None):
        grads[name + ".weight"], grads[name + ".bias"] = B.conv_w(g, x1, x2)
        return B.conv_d(name, g, x1, mask1, mask2, bits)

    ns = model.nsteps
    g, grads["outconv.weight"], grads["outconv.bias"] = B.head(t, dout)
    skip_g: Dict[int, torch.Tensor] = {}
    for depth in range(1, ns + 1):
        up, c1, c2 = dec_names(depth)
        xc1, xu, skip = t["x" + c1], t["xu" + up[-1]], t["x" + ENC[depth - 1][1]]
        g, _ = conv_bwd(c2, g, xc1, None, xc1, bits=t.get("m_x" + c1))             # -> pre-activation grad of c1
        dxu, skip_g[depth] = conv_bwd(c1, g, xu, skip, None, mask2=skip)            # the upconv output has no ReLU
        below = t["x" + (dec_names(depth + 1)[2] if depth < ns else ENC[ns][1])]
        grads[up + ".weight"], grads[up + ".bias"] = B.convt_w(below, dxu)
        g = B.convt_d(up, dxu, below)
    for lvl in range(ns, -1, -1):
        a, b = ENC[lvl]
        if lvl < ns:
            g = B.pool(skip_g[lvl + 1], g, t, lvl)
        xa = t["x" + a]
        g, _ = conv_bwd(b, g, xa, None, xa, bits=t.get("m_x" + a))                 # -> pre-activation grad of conv a
        if lvl == 0:
            grads[a + ".weight"], grads[a + ".bias"] = B.first_w(g, x)
            grads["__dx__"] = B.first_d(g, getattr(model, a).weight) if want_dx else None    # saliency: src/saliency.py:159-174
        else:
            g, _ = conv_bwd(a, g, t[f"xp{lvl}"], None, None)                        # pooled tensor: no ReLU of its own
    if scale is not None:
        ops.scale_many_(list(grads.values()), scale[1:2])    # every parameter / input gradient back to its true scale: ONE launch, exact
    return grads


def planar_range_fallback(model) -> bool:
    """True (after switching the model to train_mode 'bf16x3', loudly) if a planar forward stored activations beyond +-448 since the last look:
    there the e4m3 residual saturates and the planar format keeps only f16 accuracy; fp32 storage has fp32's range."""
    # collective: in a data-parallel job the ranks must not train in different arithmetics (one MAX all-reduce of one word, first forward only)
    from .. import parallel
    rf = getattr(model, "_range_flag", None)
    if rf is None or not parallel.any_rank_flag(rf):
        return False
    rf.zero_()
    import logging
    logging.warning("ws_unet_amd.UNet: activations beyond +-448 while training in train_mode 'f16f8p' (the planar format's e4m3 residual "
                    "saturates there); switching this model to train_mode 'bf16x3' (fp32 storage)")
    model.train_mode = "bf16x3"
    return True


def _save(ctx, model, x, t, out, m):
    t["out"], t["last"] = out, t["x" + (dec_names(1)[2] if model.nsteps else ENC[0][1])]
    ctx.model, ctx.t, ctx.x, ctx.m = model, t, x, m
    return out


class _UNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, *params):
        """UNet._walk with the training keep policy: the reference's intermediates plus idx* (NHWC) or m_x* (planar), `last` and `out`."""
        tm = getattr(model, "train_mode", "f32")
        if tm == "f16f8p":
            # what the planar inference path covers: for single-plane inputs, and for 2..8 planes where the model asks for it
            cin = model.e11.in_channels
            if model._planar_ok() and (cin == 1 or (cin <= 8 and getattr(model, "train_planes_planar", False))):
                t: Dict[str, torch.Tensor] = {}
                out = model._walk(x, _Planar(model, x, t=t, train=True))
                ok = True
                if not getattr(model, "_range_checked_train", False):
                    # first planar training forward of this model: one synchronising look at the range flag, as the inference path does.  The
                    # trainer looks again after every epoch (Trainer._run_epoch): weights move.
                    model._range_checked_train = True
                    ok = not planar_range_fallback(model)
                if ok:
                    return _save(ctx, model, x, t, out, ops.MODE_F16F8P)
            tm = model.train_mode if model.train_mode != "f16f8p" else "bf16x3"   # multi-plane inputs, odd shapes, range fallback: fp32 storage
        m = ops.mode_id(tm)
        if m == ops.MODE_BF16:
            raise ValueError("train_mode must be 'f32' or 'bf16x3' (activations are kept in fp32 for the backward pass)")
        # e11 and outconv run in the train mode, the matrix layers of a split-bf16 run in train_fwd_mode (WSU_TRAIN_FWD_MODE='bf16x3' keeps them there)
        mf = ops.mode_id(getattr(model, "train_fwd_mode", None) or "f16f8x") if m == ops.MODE_BF16X3 else m
        t = {}
        return _save(ctx, model, x, t, model._walk(x, _NHWC(model, mf, m0=m, t=t, train=True)), m)

    @staticmethod
    def backward(ctx, dout):
        model, m = ctx.model, ctx.m
        B = _PlanarBwd(model) if m == ops.MODE_F16F8P else _NHWCBwd(model, m)
        grads = _backward(B, model, ctx.t, ctx.x, dout.contiguous().float(), ctx.needs_input_grad[1])
        ctx.t = None
        return (None, grads["__dx__"]) + tuple(grads[name] if p.requires_grad else None for name, p in model.named_parameters())


def unet_apply(model, x: torch.Tensor) -> torch.Tensor:
    return _UNetFn.apply(model, x, *_param_list(model))
