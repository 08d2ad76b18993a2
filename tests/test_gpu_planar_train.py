"""Parity of the PLANAR training kernels (gradients in the F16F8P layout) against torch-CPU autograd of the reference's layers
(src/unet/model/unet.py:82-132,141-189 under autograd; oracle: torch.nn.functional on the CPU, fp32).

Tolerances: the band against the fp32 oracle is REL_L2 = 3e-4 (relative L2 of a whole tensor), the band of tests/test_gpu_backward_large.py
for the NHWC f16f8x kernels.  What it can tell apart: a wrong tap, channel, mask, tile edge or accumulation -- errors of the size of the
result.  What it cannot: the f16f8 arithmetic (f16 a * f16 b plus the two residual cross terms) sits ~1e-5 from the oracle on these
operands, but the f16 products ALONE sit at ~2e-4 .. 3e-4 (the products 'f16' tests below state it), inside the same band -- a kernel that
dropped, mis-scaled or misread its cross terms would still pass here.  tests/test_gpu_f16f8_terms.py holds the six matrix kernels to their
own three-term arithmetic instead (bit for bit on crafted operands, and to a quarter of the f16-only distance on realistic ones).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import math

from gpu_util import DEV, GRAD_LO, gpu_model, planar_decode, planar_encode
from ws_unet_amd import formula, losses

pytestmark = pytest.mark.gpu

REL_L2 = 3e-4


def _ops():
    from ws_unet_amd import ops
    return ops


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _h(t):
    """what the f16 planes of a planar tensor hold for t"""
    return t.half().float()


def _q(t, lo):
    """the values a planar tensor holds for t"""
    return planar_decode(planar_encode(t, lo), lo)


@pytest.mark.parametrize("n,h,w,cin,csplit,cout,masked", [
    (2, 16, 32, 64, 64, 64, False),
    (1, 40, 72, 64, 64, 64, True),          # partial tiles in both directions
    (2, 32, 64, 128, 64, 64, False),        # fused concat: two gradients
    (1, 24, 40, 128, 128, 32, True),
    (1, 3, 5, 64, 64, 64, True),            # rows 1 and h-2 coincide
    (2, 2, 2, 64, 64, 32, False),
])
@pytest.mark.parametrize("pad_zero", [True, False])
def test_conv3x3_pl_bwd_data(n, h, w, cin, csplit, cout, masked, pad_zero):
    ops = _ops()
    wgt = _rand((cout, cin, 3, 3), 1, (2.0 / (9 * cin)) ** 0.5)
    g = _q(_rand((n, cout, h, w), 2), GRAD_LO)
    act = torch.relu(_rand((n, cin, h, w), 3)) if masked else None
    x = torch.zeros((n, cin, h, w), requires_grad=True)
    xp = F.pad(x, (1, 1, 1, 1), mode="constant" if pad_zero else "reflect")
    F.conv2d(xp, wgt).backward(g)
    ref = x.grad.clone()
    if masked:
        ref = ref * (act > 0)
    wd = wgt.to(DEV)
    wp = ops.pack_conv3x3(wd, ops.MODE_F16F8, dgrad=True)
    wr = None if pad_zero else ops.pack_conv3x3_ring(wd)
    m1 = planar_encode(act[:, :csplit]) if masked else None
    m2 = planar_encode(act[:, csplit:]) if (masked and csplit < cin) else None
    dx1, dx2 = ops.conv3x3_pl_bwd_data(planar_encode(g, GRAD_LO), wp, wr, cin, csplit, m1, m2, pad_zero=pad_zero)
    torch.cuda.synchronize()
    got = planar_decode(dx1, GRAD_LO)
    if dx2 is not None:
        got = torch.cat([got, planar_decode(dx2, GRAD_LO)], dim=1)
    assert got.shape == ref.shape
    assert rel_l2(got, ref) < REL_L2, rel_l2(got, ref)
    assert float((got - ref).abs().max()) < 2e-3 * float(ref.abs().max())
    if masked:
        assert float(got[(act <= 0)].abs().max()) == 0.0


def _mask_bits_ref(y_planar):
    """relu_mask plane of a planar activation, restated on the host (include/wsu.h): byte (pixel, 8-channel granule), bit e = stored f16 value
    of channel 8 g + e > 0; rows / columns padded to the 16 x 32 tile grid with zeros."""
    raw = y_planar.detach().contiguous().view(torch.uint8)                        # (n, chunk, 3, h, w, 16)
    n, nch, _, h, w, _ = raw.shape
    f16 = torch.stack([raw[:, :, 0], raw[:, :, 1]], dim=2).contiguous().view(torch.float16).reshape(n, nch * 2, h, w, 8)   # granule planes
    bits = ((f16 > 0).to(torch.int32) << torch.arange(8, device=raw.device, dtype=torch.int32)).sum(-1).to(torch.uint8)
    out = torch.zeros((n, nch * 2, (h + 15) // 16 * 16, (w + 31) // 32 * 32), dtype=torch.uint8, device=raw.device)
    out[:, :, :h, :w] = bits
    return out


@pytest.mark.parametrize("n,h,w,c1,c2,cout", [(2, 32, 64, 64, 0, 64), (1, 18, 34, 64, 64, 128), (3, 2, 2, 128, 0, 64), (1, 40, 72, 16, 0, 64)])
def test_relu_mask_plane_of_the_forward_kernels(n, h, w, c1, c2, cout):
    """The 1-bit ReLU mask written by the training forward (wsu_conv3x3_pl_fwd relu_mask_out, wsu_conv3x3_first_pl_fwd) is exactly the sign
    pattern of the stored f16 planes -- what the data gradient used to re-read (ragged tiles, the smallest image, fused concat)."""
    ops = _ops()
    x1 = planar_encode(torch.relu(_rand((n, c1, h, w), 31)))
    x2 = planar_encode(torch.relu(_rand((n, c2, h, w), 32))) if c2 else None
    wgt = _rand((cout, c1 + c2, 3, 3), 33, (2.0 / (9 * (c1 + c2))) ** 0.5).to(DEV)
    b = _rand((cout,), 34, 0.1).to(DEV)
    y, mask = ops.conv3x3_pl(x1, x2, ops.pack_conv3x3(wgt, ops.MODE_F16F8), b, cout, want_mask=True)
    y0 = ops.conv3x3_pl(x1, x2, ops.pack_conv3x3(wgt, ops.MODE_F16F8), b, cout)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int32), y0.view(torch.int32))                  # asking for the mask does not change y
    assert torch.equal(mask, _mask_bits_ref(y))
    assert 0.2 < float((planar_decode(y) > 0).float().mean()) < 0.8               # a real mix of zeros and positives
    img = _rand((n, 1, h, w), 35).to(DEV)
    w1, b1 = _rand((64, 1, 3, 3), 36, 0.5).to(DEV), _rand((64,), 37, 0.1).to(DEV)
    f, fmask = ops.conv3x3_first_pl(img, w1, b1, want_mask=True)
    assert torch.equal(fmask, _mask_bits_ref(f))


@pytest.mark.parametrize("products", ["f16f8", "f16"])
@pytest.mark.parametrize("n,h,w,cin,csplit,cout", [
    (2, 32, 64, 64, 64, 64), (1, 37, 70, 128, 64, 64), (2, 18, 34, 64, 64, 128), (1, 96, 160, 128, 128, 64),
    (3, 96, 160, 64, 64, 32), (3, 96, 160, 64, 64, 48), (2, 200, 96, 64, 64, 80),     # 2 / 3 / 5 steps per tile, several tiles per workgroup: with products
])                                                                                     # 'f16' the mask pieces ride the counted vmcnt waits of the 4-stage ring
def test_conv3x3_pl_bwd_data_mask_bits_equal_activation_masks(n, h, w, cin, csplit, cout, products):
    """The data gradient fed the 1-bit planes (LDS-DMA of 4 KB per tile) returns bitwise what it returns fed the activations themselves
    (16 granule loads per loader lane and tile): same masks, same arithmetic (reflect padding incl. the border fold; fused concat)."""
    ops = _ops()
    live = slice(0, 2) if products == "f16" else slice(0, 3)
    wd = _rand((cout, cin, 3, 3), 41, (2.0 / (9 * cin)) ** 0.5).to(DEV)
    g = planar_encode(_rand((n, cout, h, w), 42), GRAD_LO)
    act = torch.relu(_rand((n, cin, h, w), 43))
    m1 = planar_encode(act[:, :csplit]); m2 = planar_encode(act[:, csplit:]) if csplit < cin else None
    wp, wr = ops.pack_conv3x3(wd, ops.MODE_F16F8, dgrad=True), ops.pack_conv3x3_ring(wd)
    a1, a2 = ops.conv3x3_pl_bwd_data(g, wp, wr, cin, csplit, m1, m2, products=products)
    mb1, mb2 = _mask_bits_ref(m1), None if m2 is None else _mask_bits_ref(m2)
    for rep_ in range(3):                                                # (repeats: a missing wait on the mask pieces shows as a launch-to-launch difference)
        b1, b2 = ops.conv3x3_pl_bwd_data(g, wp, wr, cin, csplit, m1, m2, mask1_bits=mb1, mask2_bits=mb2, products=products)
        torch.cuda.synchronize()
        assert torch.equal(a1[:, :, live].view(torch.int32), b1[:, :, live].view(torch.int32))
        if a2 is not None:
            assert torch.equal(a2[:, :, live].view(torch.int32), b2[:, :, live].view(torch.int32))
    got = planar_decode(b1, GRAD_LO, f16_only=products == "f16")
    assert float(got[(act[:, :csplit] <= 0)].abs().max()) == 0.0 and float(got.abs().max()) > 0


@pytest.mark.parametrize("n,h,w,c1,c2,cout", [
    (2, 16, 32, 64, 0, 64),
    (1, 37, 70, 64, 0, 128),            # partial tiles, several tiles per image column (rolling row window)
    (2, 24, 40, 64, 64, 64),            # fused concat
    (3, 10, 33, 128, 0, 64),
    # shapes where a workgroup of the ring kernel walks several steps (256 CUs): across column ends, with empty splits, the LDS ring wrapping
    (4, 100, 96, 64, 0, 64),            # 600 tiles over 256 workgroups: 3 tiles each, columns of 50 tiles, 56 empty splits
    (2, 320, 128, 64, 0, 64),           # 1280 tiles: 5 tiles + prologue per workgroup (ring of 4 U / 5 V slots wraps)
    (1, 200, 96, 128, 0, 128),          # 4 (mb, nb) workgroups per split: 64 splits of 5 tiles, columns of 100
    (1, 96, 160, 64, 64, 64),           # fused concat, 240 tiles over 128 splits
])
def test_conv3x3_pl_bwd_weight(n, h, w, c1, c2, cout):
    ops = _ops()
    cin = c1 + c2
    x = _q(torch.relu(_rand((n, cin, h, w), 5)), 4096.0)
    g = _q(_rand((n, cout, h, w), 6), GRAD_LO)
    wgt = torch.zeros((cout, cin, 3, 3), requires_grad=True)
    b = torch.zeros(cout, requires_grad=True)
    F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), wgt, b).backward(g)
    x1 = planar_encode(x[:, :c1])
    x2 = planar_encode(x[:, c1:]) if c2 else None
    dw, db = ops.conv3x3_pl_bwd_weight(planar_encode(g, GRAD_LO), x1, x2)
    torch.cuda.synchronize()
    assert rel_l2(dw.cpu(), wgt.grad) < REL_L2, rel_l2(dw.cpu(), wgt.grad)
    assert rel_l2(db.cpu(), b.grad) < 2e-6, rel_l2(db.cpu(), b.grad)
    dw2, _ = ops.conv3x3_pl_bwd_weight(planar_encode(g, GRAD_LO), x1, x2)
    assert torch.equal(dw, dw2)                                        # fixed-order reduction


@pytest.mark.parametrize("n,h,w,cin,csplit,cout,masked,pad_zero", [
    (2, 16, 32, 64, 64, 64, False, True),
    (1, 40, 72, 64, 64, 64, True, False),       # partial tiles, border ring
    (2, 32, 64, 128, 64, 64, False, False),     # fused concat: two gradients
    (1, 24, 40, 128, 128, 32, True, True),
    (1, 3, 5, 64, 64, 64, True, False),
    (1, 96, 160, 64, 64, 128, True, False),     # several tiles per workgroup, 8 chunks
])
def test_conv3x3_pl_bwd_data_f16_products(n, h, w, cin, csplit, cout, masked, pad_zero):
    """products = 'f16' (wsu.h WSU_PRODUCTS_F16): the kernel multiplies the f16 parts of gradient and weights and nothing else -- equal, up to the
    accumulation order and the store encoding, to the exact adjoint taken on f16-rounded operands; against the unrounded adjoint the operand
    rounding shows as ~1e-4 relative L2."""
    ops = _ops()
    wgt = _rand((cout, cin, 3, 3), 1, (2.0 / (9 * cin)) ** 0.5)
    g = _q(_rand((n, cout, h, w), 2), GRAD_LO)
    act = torch.relu(_rand((n, cin, h, w), 3)) if masked else None
    refs = []
    for gg, ww in ((_h(g), _h(wgt)), (g, wgt)):
        x = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
        F.conv2d(F.pad(x, (1, 1, 1, 1), mode="constant" if pad_zero else "reflect"), ww.double()).backward(gg.double())
        refs.append(x.grad * (act > 0) if masked else x.grad)
    wd = wgt.to(DEV)
    wp = ops.pack_conv3x3(wd, ops.MODE_F16F8, dgrad=True)
    wr = None if pad_zero else ops.pack_conv3x3_ring(wd)
    m1 = planar_encode(act[:, :csplit]) if masked else None
    m2 = planar_encode(act[:, csplit:]) if (masked and csplit < cin) else None
    dx1, dx2 = ops.conv3x3_pl_bwd_data(planar_encode(g, GRAD_LO), wp, wr, cin, csplit, m1, m2, pad_zero=pad_zero, products="f16")
    torch.cuda.synchronize()
    got = planar_decode(dx1, GRAD_LO, f16_only=True)                    # products 'f16': the result is an f16 tensor (no residual plane is written)
    if dx2 is not None:
        got = torch.cat([got, planar_decode(dx2, GRAD_LO, f16_only=True)], dim=1)
    # = the exact adjoint of the f16 parts, rounded to f16 once (2^-12: 1.4e-4 relative L2) -- twice on the border ring of the reflect adjoint
    assert rel_l2(got, refs[0]) < 3e-4, rel_l2(got, refs[0])
    if pad_zero:
        assert rel_l2(got, _h(refs[0].float())) < 5e-5, rel_l2(got, _h(refs[0].float()))  # up to last-place flips from the accumulation order
    assert rel_l2(got, refs[1]) < 5e-4, rel_l2(got, refs[1])
    if masked:
        assert float(got[(act <= 0)].abs().max()) == 0.0


@pytest.mark.parametrize("n,h,w,c1,c2,cout", [
    (2, 16, 32, 64, 0, 64),
    (1, 40, 72, 64, 0, 64),             # partial tiles
    (2, 320, 128, 64, 0, 64),           # the ring wraps
    (1, 200, 96, 128, 0, 128),
    (1, 96, 160, 64, 64, 64),           # fused concat
])
def test_conv3x3_pl_bwd_weight_f16_products(n, h, w, c1, c2, cout):
    """products = 'f16': dW from the f16 parts of gradient and activations (exact products, fp32 accumulation), db = the sum of the gradient's
    f16 parts; deterministic.  On these random operands -- sums of zero-mean products, the worst case for rounding noise -- the operand rounding
    costs ~2e-4 relative L2 against the unrounded gradient."""
    ops = _ops()
    cin = c1 + c2
    x = _q(torch.relu(_rand((n, cin, h, w), 5)), 4096.0)
    g = _q(_rand((n, cout, h, w), 6), GRAD_LO)
    refs = []
    for gg, xx in ((_h(g), _h(x)), (g, x)):
        wgt = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        F.conv2d(F.pad(xx.double(), (1, 1, 1, 1), mode="reflect"), wgt, b).backward(gg.double())
        refs.append((wgt.grad, b.grad))
    x1 = planar_encode(x[:, :c1])
    x2 = planar_encode(x[:, c1:]) if c2 else None
    dw, db = ops.conv3x3_pl_bwd_weight(planar_encode(g, GRAD_LO), x1, x2, products="f16")
    torch.cuda.synchronize()
    assert rel_l2(dw.cpu(), refs[0][0]) < 5e-6, rel_l2(dw.cpu(), refs[0][0])
    assert rel_l2(db.cpu(), refs[0][1]) < 2e-6, rel_l2(db.cpu(), refs[0][1])
    assert rel_l2(dw.cpu(), refs[1][0]) < 5e-4, rel_l2(dw.cpu(), refs[1][0])
    dw2, db2 = ops.conv3x3_pl_bwd_weight(planar_encode(g, GRAD_LO), x1, x2, products="f16")
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("products", ["f16f8", "f16"])
def test_planar_backward_kernels_race_screen(products):
    """Repeat launches of the pipelined backward kernels (weight-gradient ring: LDS-DMA three steps deep; data gradient: persistent kernel -- two
    stages, or four with the DMA three steps ahead and counted vmcnt waits for products 'f16' -- + ring launches; transposed-conv data gradient:
    three / six stages) must be bitwise identical: a missing wait or barrier shows up as a launch-to-launch difference."""
    ops = _ops()
    n, h, w, c = 2, 320, 128, 64
    live = slice(0, 2) if products == "f16" else slice(0, 3)           # products 'f16' writes no residual plane
    x = planar_encode(torch.relu(_rand((n, c, h, w), 21)))
    g = planar_encode(_rand((n, c, h, w), 22), GRAD_LO)
    wd = _rand((c, c, 3, 3), 23, 0.05).to(DEV)
    wp, wr = ops.pack_conv3x3(wd, ops.MODE_F16F8, dgrad=True), ops.pack_conv3x3_ring(wd)
    mbits = _mask_bits_ref(x)
    wt = _rand((c, c, 2, 2), 24, 0.1).to(DEV)
    wtp = ops.pack_convt2x2_pl_dgrad(wt)
    xs = planar_encode(torch.relu(_rand((n, c, h // 2, w // 2), 25)))
    dw0, db0 = ops.conv3x3_pl_bwd_weight(g, x, None, products=products)
    dx0, _ = ops.conv3x3_pl_bwd_data(g, wp, wr, c, c, x, None, mask1_bits=mbits, products=products)
    dt0 = ops.convt2x2_pl_bwd_data(g, wtp, c, xs, products=products)
    dw0, db0, dx0, dt0 = dw0.clone(), db0.clone(), dx0[:, :, live].clone(), dt0[:, :, live].clone()
    for _ in range(15):
        dw, db = ops.conv3x3_pl_bwd_weight(g, x, None, products=products)
        dx, _ = ops.conv3x3_pl_bwd_data(g, wp, wr, c, c, x, None, mask1_bits=mbits, products=products)
        dt = ops.convt2x2_pl_bwd_data(g, wtp, c, xs, products=products)
        assert torch.equal(dw, dw0) and torch.equal(db, db0)
        assert torch.equal(dx[:, :, live].view(torch.int32), dx0.view(torch.int32))
        assert torch.equal(dt[:, :, live].view(torch.int32), dt0.view(torch.int32))


@pytest.mark.parametrize("products", ["f16f8", "f16"])
@pytest.mark.parametrize("n,h,w,cin,cout", [
    (2, 8, 32, 64, 64), (1, 13, 40, 128, 64), (2, 5, 7, 64, 128), (3, 64, 96, 64, 64),
    (1, 100, 64, 256, 128),             # 8 (mb, nb) workgroups per split: 64 splits of 1-2 tiles (the register prefetch runs), the last ones empty
])
def test_convt2x2_pl_bwd_weight(n, h, w, cin, cout, products):
    """products 'f16': exact products of the f16 parts (reference on f16-rounded operands: 5e-6), ~2e-4 from the unrounded gradient on
    these zero-mean random operands; db = the sum of dy's f16 parts."""
    ops = _ops()
    x = _q(torch.relu(_rand((n, cin, h, w), 7)), 4096.0)
    dy = _q(_rand((n, cout, 2 * h, 2 * w), 8), GRAD_LO)
    refs = []
    for xx, dd in ((x, dy), (_h(x), _h(dy))):
        wgt = torch.zeros((cin, cout, 2, 2), dtype=torch.float64, requires_grad=True)
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(xx.double(), wgt, b, stride=2).backward(dd.double())
        refs.append((wgt.grad, b.grad))
    dw, db = ops.convt2x2_pl_bwd_weight(planar_encode(x), planar_encode(dy, GRAD_LO), products=products)
    torch.cuda.synchronize()
    if products == "f16":
        assert rel_l2(dw.cpu(), refs[1][0]) < 5e-6, rel_l2(dw.cpu(), refs[1][0])
        assert rel_l2(db.cpu(), refs[1][1]) < 2e-6, rel_l2(db.cpu(), refs[1][1])
        assert rel_l2(dw.cpu(), refs[0][0]) < 5e-4, rel_l2(dw.cpu(), refs[0][0])
    else:
        assert rel_l2(dw.cpu(), refs[0][0]) < REL_L2, rel_l2(dw.cpu(), refs[0][0])
        assert rel_l2(db.cpu(), refs[0][1]) < 2e-6, rel_l2(db.cpu(), refs[0][1])   # partial tiles: clamped copies of edge pixels are not summed


@pytest.mark.parametrize("products", ["f16f8", "f16"])
@pytest.mark.parametrize("n,h,w,cin,cout,masked", [
    (2, 8, 32, 64, 64, True), (1, 13, 40, 128, 64, True), (2, 5, 7, 64, 32, False), (1, 4, 64, 256, 128, True),
    (5, 64, 128, 64, 32, True),         # 320 tiles of 2 steps: workgroups walk 1-2 tiles, the six-stage ring of products 'f16' fills and drains
    (3, 60, 100, 64, 112, False),       # 7 steps per tile (the ring wraps inside a tile), partial tiles
])
def test_convt2x2_pl_bwd_data(n, h, w, cin, cout, masked, products):
    """products 'f16': only the f16 planes of dy and of the weights are fetched and multiplied (reference on f16-rounded operands: 2e-5, the
    store encoding), six LDS stages instead of three."""
    ops = _ops()
    wgt = _rand((cin, cout, 2, 2), 9, (1.0 / cin) ** 0.5)
    dy = _q(_rand((n, cout, 2 * h, 2 * w), 10), GRAD_LO)
    act = torch.relu(_rand((n, cin, h, w), 11))
    refs = []
    for ww, dd in ((wgt, dy), (_h(wgt), _h(dy))):
        x = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(x, ww.double(), stride=2).backward(dd.double())
        refs.append(x.grad * (act > 0) if masked else x.grad)
    wp = ops.pack_convt2x2_pl_dgrad(wgt.to(DEV))
    dx = ops.convt2x2_pl_bwd_data(planar_encode(dy, GRAD_LO), wp, cin, planar_encode(act) if masked else None, products=products)
    torch.cuda.synchronize()
    got = planar_decode(dx, GRAD_LO, f16_only=products == "f16")
    if products == "f16":
        assert rel_l2(got, _h(refs[1].float())) < 5e-5, rel_l2(got, _h(refs[1].float()))
        assert rel_l2(got, refs[0]) < 5e-4, rel_l2(got, refs[0])
    else:
        assert rel_l2(got, refs[0]) < REL_L2, rel_l2(got, refs[0])
        assert float((got - refs[0]).abs().max()) < 2e-3 * float(refs[0].abs().max())


@pytest.mark.parametrize("products", ["f16f8", "f16"])
@pytest.mark.parametrize("with_skip", [True, False])
def test_maxpool2x2_pl_bwd(with_skip, products):
    ops = _ops()
    n, c, h, w = 2, 32, 12, 20
    act = _q(torch.relu(_rand((n, c, h, w), 12)), 4096.0)
    act[0, :, 0:2, 0:2] = 0.0                                           # an all-zero window: nothing is routed
    act[0, :, 2:4, 2:4] = 1.5                                           # a tie: the first position wins
    skip = _q(_rand((n, c, h, w), 13), GRAD_LO)
    dyp = _q(_rand((n, c, h // 2, w // 2), 14), GRAD_LO)
    a = act.clone().requires_grad_(True)
    F.max_pool2d(a, 2).backward(dyp)
    if products == "f16":               # gradient tensors are f16 tensors: their residual planes are neither read nor written
        skip, dyp = _h(skip), _h(dyp)
        a = act.clone().requires_grad_(True)
        F.max_pool2d(a, 2).backward(dyp)
    ref = (a.grad + (skip if with_skip else 0)) * (act > 0)
    g = ops.maxpool2x2_pl_bwd(planar_encode(skip, GRAD_LO) if with_skip else None, planar_encode(dyp, GRAD_LO), planar_encode(act), products=products)
    torch.cuda.synchronize()
    got = planar_decode(g, GRAD_LO, f16_only=products == "f16")
    if products == "f16":
        assert torch.equal(got, _h(ref))                                # one f16 rounding of an exact fp32 sum
    else:
        assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max()) + 1e-7     # one re-encoding of an fp32 sum
    assert float(got[0, :, 0:2, 0:2].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [(2, 64, 24, 40), (2, 64, 192, 200)])      # the second: more pixels than one grid pass (the sum kernels take two pixels per thread then, some threads one)
@pytest.mark.parametrize("products", ["f16f8", "f16"])
def test_head_and_first_layer_pl_bwd(products, shape):
    ops = _ops()
    f16 = products == "f16"
    n, c, h, w = shape
    x = _q(torch.relu(_rand((n, c, h, w), 15)), 4096.0)
    wh = _rand((1, c, 1, 1), 16, 0.2).requires_grad_(True)
    bh = torch.zeros(1, requires_grad=True)
    xa = x.clone().requires_grad_(True)
    out = torch.sigmoid(F.conv2d(xa, wh, bh))
    dout = _rand((n, 1, h, w), 17, 3.0)
    out.backward(dout)
    g, dw, db = ops.conv1x1_sigmoid_pl_bwd(planar_encode(x), wh.detach().to(DEV), out.detach().to(DEV), dout.to(DEV), products=products)
    torch.cuda.synchronize()
    ref_g = xa.grad * (x > 0)
    assert rel_l2(planar_decode(g, GRAD_LO, f16_only=f16), ref_g) < (3e-4 if f16 else 3e-5)      # f16: one 2^-12 rounding per value
    assert rel_l2(dw.cpu(), wh.grad) < 1e-5 and rel_l2(db.cpu(), bh.grad) < 1e-5
    # per-channel sums and the first layer's weight gradient from the same planar gradient
    gq = planar_decode(g, GRAD_LO, f16_only=f16)
    assert rel_l2(ops.colsum_pl(g, products=products).cpu(), gq.sum(dim=(0, 2, 3))) < 2e-6
    img = torch.rand((n, 1, h, w), generator=torch.Generator().manual_seed(18))
    w1 = torch.zeros((c, 1, 3, 3), requires_grad=True)
    b1 = torch.zeros(c, requires_grad=True)
    F.conv2d(F.pad(img, (1, 1, 1, 1), mode="reflect"), w1, b1).backward(gq)
    dw1, db1 = ops.conv3x3_first_pl_bwd_weight(g, img.to(DEV), products=products)
    torch.cuda.synchronize()
    assert rel_l2(dw1.cpu(), w1.grad) < 1e-5 and rel_l2(db1.cpu(), b1.grad) < 2e-6


@pytest.fixture(scope="module")
def grad_golden():
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "unet_grad.npz"))


@pytest.mark.parametrize("products", ["f16f8", "f16"])
@pytest.mark.parametrize("ns", [0, 1, 2])
def test_unet_gradients_golden_planar(grad_golden, ns, products):
    """train_mode 'f16f8p' end to end against the reference's autograd golden (tests/golden/make_golden.py: L1WS on 2x1x64x64 pairs):
    planar activations and gradients, the bands of test_gpu_backward.py::test_unet_gradients_golden for the split arithmetics."""
    ops = _ops()
    g = grad_golden
    model = gpu_model(ns, "he", "f16f8p")
    model.train_mode = "f16f8p"
    model.train_products = products
    cov_u8 = formula.synthetic_images(2, 64, 64, seed=11)
    st_u8 = cov_u8.copy(); st_u8[0] = formula.lsbr_embed(cov_u8[0], 0.4, seed=5)
    covers = torch.from_numpy(cov_u8.astype(np.float32) / np.float32(255.))[:, None].to(DEV)
    inputs = torch.from_numpy(st_u8.astype(np.float32) / np.float32(255.))[:, None].to(DEV)
    alphas = torch.tensor([0.4, 0.0], device=DEV)
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        out = model(inputs)
        loss = losses.L1WSLoss()(out, (covers, alphas), inputs)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_timer(None)
    used = timer.summary()
    assert "conv3x3_pl_bwd_data" in used and "conv3x3_pl_bwd_weight" in used and "conv3x3_bwd_data" not in used     # the planar path ran
    assert math.isclose(loss.item(), float(g[f"grad{ns}_loss"][0]), rel_tol=1e-5)
    np.testing.assert_allclose(out.detach().cpu().numpy(), g[f"grad{ns}_out"], atol=1e-4, rtol=0)
    for k, p in model.named_parameters():
        got = p.grad.detach().cpu().numpy().reshape(-1)
        ref = g[f"grad{ns}_{k}_sub"]
        if not (ns == 0 or got.size <= 4096):
            got = got[::97]
        scale = float(np.abs(ref).max())
        np.testing.assert_allclose(got, ref, rtol=0, atol=1.5e-2 * scale + 1e-12, err_msg=f"unet_{ns} {k}")
        full = p.grad.detach().double().cpu().numpy()
        assert math.isclose(float(np.sqrt((full ** 2).sum())), g[f"grad{ns}_{k}_sum"][2], rel_tol=8e-3), k
    first = {k: p.grad.clone() for k, p in model.named_parameters()}
    model.zero_grad()
    losses.L1WSLoss()(model(inputs), (covers, alphas), inputs).backward()
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, first[k]), k                        # deterministic


@pytest.mark.parametrize("products", ["f16f8", "f16"])
@pytest.mark.parametrize("n,size", [(2, 128), (1, 512), (1, 1024)])
def test_planar_vs_fp32_storage_gradients_smooth_loss(n, size, products):
    """The two training paths of one model under a smooth (L2) loss: same arithmetic class, different storage -- every parameter gradient agrees
    to a relative L2 of 2e-3 (ReLU-mask flips on rounding noise are the floor; test_gpu_backward_large.py).  At 512x512 every persistent
    workgroup of the data-gradient kernel walks several tiles and the weight-gradient ring several steps."""
    model = gpu_model(2, "he", "f16f8p")
    model.train_products = products                 # f16 products in the backward matrix kernels: the same band (its rounding noise sits below the mask flips)
    x = torch.rand((n, 1, size, size), generator=torch.Generator().manual_seed(3)).to(DEV)
    tgt = torch.rand((n, 1, size, size), generator=torch.Generator().manual_seed(4)).to(DEV)
    res = {}
    for tm in ("f32", "f16f8p"):
        model.train_mode = tm
        model.zero_grad()
        ((model(x) - tgt) ** 2).mean().backward()
        res[tm] = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters()}
    for k in res["f32"]:
        assert rel_l2(res["f16f8p"][k], res["f32"][k]) < 2e-3, (k, rel_l2(res["f16f8p"][k], res["f32"][k]))


@pytest.mark.parametrize("ns", [3, 4])
def test_planar_training_deep_nets(ns):
    """unet_3 / unet_4 (512 / 1024 channels, 4x4 images at the bottom of a 64x64 input).  On these deep nets at this size ReLU-mask flips put
    every non-exact arithmetic 2e-3 .. 7e-3 (relative L2 per parameter) away from the exact-fp32 path (tools/diag_deep.py), so the planar path is
    held to the deviation of round 1's split-bf16 path on the same model and input: at most 1.5x + 5e-4 per parameter, and below 1e-2."""
    model = gpu_model(ns, "he", "f16f8p")
    x = torch.rand((2, 1, 64, 64), generator=torch.Generator().manual_seed(5)).to(DEV)
    tgt = torch.rand((2, 1, 64, 64), generator=torch.Generator().manual_seed(6)).to(DEV)
    res = {}
    for tm in ("f32", "f16f8p", "bf16x3"):
        model.train_mode = tm
        model.zero_grad()
        ((model(x) - tgt) ** 2).mean().backward()
        res[tm] = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters()}
    for k in res["f32"]:
        dp, dx = rel_l2(res["f16f8p"][k], res["f32"][k]), rel_l2(res["bf16x3"][k], res["f32"][k])
        assert dp < 1.5 * dx + 5e-4 and dp < 1e-2, (k, dp, dx)


@pytest.mark.parametrize("products", ["f16", "f16f8"])
def test_planar_input_gradient_matches_the_oracle(products):
    """Round 4 (VERDICT r03 missing #4): a default-mode model asked for dL/dx (saliency, src/saliency.py:159-174: parameters frozen, backward from
    ONE output pixel) stays on the planar training path -- wsu_conv3x3_first_pl_bwd_data closes the chain -- and the input gradient matches the
    CPU oracle's autograd; a model with more than one input plane still takes the fp32-storage path (its first-layer weight gradient is
    single-plane only)."""
    from oracle import unet_ref
    ops = _ops()
    model = gpu_model(2, "he", None)
    model.train_products = products
    assert model.train_mode == "f16f8p"
    for p in model.parameters():
        p.requires_grad = False
    x = torch.rand((2, 1, 64, 96), generator=torch.Generator().manual_seed(9))
    xi = x.clone().to(DEV).requires_grad_(True)
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        out = model(xi)
        (out[0, 0, 20, 31] + out[1, 0, 1, 0]).backward()                  # an interior pixel and a corner (the reflect adjoint)
        torch.cuda.synchronize()
    finally:
        ops.set_timer(None)
    used = set(timer.summary())
    assert {"conv3x3_first_pl_bwd_data", "conv3x3_pl_bwd_data"} <= used and "conv3x3_bwd_data" not in used and "conv3x3_first_bwd_data" not in used, used
    ref = unet_ref.build_ref(2, formula.formula_state_dict(2, "he"))
    xr = x.clone().requires_grad_(True)
    o = ref(xr)
    (o[0, 0, 20, 31] + o[1, 0, 1, 0]).backward()
    got, want = xi.grad.detach().cpu(), xr.grad.detach()
    assert float(got[0, 0, 50:, :].abs().max()) == 0.0 and float(got[0, 0, :, 70:].abs().max()) == 0.0      # confined to the receptive field
    err = rel_l2(got, want)
    print("planar input gradient, products", products, "relative L2 vs oracle", err)
    assert err < (5e-3 if products == "f16" else 5e-4), err      # measured 1.1e-3 / 4.9e-5


def test_planar_training_range_fallback(caplog):
    """Activations beyond +-448 (here: e11 scaled up, e12 scaled down) make the FIRST planar training forward switch the model to fp32 storage,
    loudly; the gradients of that call already come from the fp32-storage path."""
    import logging
    ops = _ops()
    model = gpu_model(1, "he", "f16f8p")
    with torch.no_grad():
        model.e11.weight.mul_(3000.0); model.e11.bias.mul_(3000.0); model.e12.weight.div_(3000.0)
    model.invalidate_packed()
    x = torch.rand((1, 1, 32, 64), generator=torch.Generator().manual_seed(10)).to(DEV)
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        with caplog.at_level(logging.WARNING):
            model(x).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.set_timer(None)
    assert model.train_mode == "bf16x3"
    assert any("train_mode 'f16f8p'" in r.getMessage() for r in caplog.records)
    used = set(timer.summary())
    assert "conv3x3_bwd_data" in used and "conv3x3_pl_bwd_data" not in used
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
