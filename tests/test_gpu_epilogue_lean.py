"""The tile epilogue of conv3x3_q / conv3x3_qu after its instruction diet (csrc/wsu_device.h: wsu_q4_pre; conv3x3_q.hip / conv3x3_qu.hip:
finish_tile): ONE maximum chain on the fp32 values gives the block scale (through one f16 conversion) and the range flag, the store offsets of a
tile are formed once, and the one-plane head variant tests its plane count at compile time.

Controlled blocks: zero weights and a per-channel bias, so every stored value of channel c is bias[c] (relu: max(bias[c], 0)) and every pixel
carries the same 16 blocks (cout = 256).  What is stored must be, bit for bit, the encoding gpu_util restates (planar_q_parts): f16 planes,
scale bytes, the f16 parts' nibbles and the residual nibbles (exact fp32 residual, one rounding -- equality held on the library before this
change too, so it is required, not the one-grid-step bound of _check_q_tensor).  The block patterns sit where the maximum can go wrong: in each of
the 16 channel positions (X / Y halves, lane and partner lane), around the mantissa-1.5 rule of wsu_q4_block_exp, where the fp32 maximum rounds up
into the next f16 binade, f16 subnormals, an all-zero block, a negative value of largest magnitude, values that overflow f16.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, fp4_codes, planar_decode, planar_q_decode, planar_q_encode, planar_q_parts, q_block_exp
from test_gpu_fixed_costs import _conv3x3_q_ref, _operands, _walk_case

pytestmark = pytest.mark.gpu

COUT = 256


def _position_bias():
    """block k: the largest value in channel position k, signs mixed below it"""
    b = torch.zeros(16, 16)
    for k in range(16):
        for j in range(16):
            b[k, j] = (0.1 + 0.05 * j) * (-1.0 if (j + k) % 3 == 0 else 1.0)
        b[k, k] = 3.0 + 0.125 * k
    return b.reshape(-1)


_EDGE_MAXIMA = [
    1.5,                                  # f16 mantissa exactly 1.5: the finer grid (largest / 2^E = 6)
    1.5 - 2.0 ** -10,                     # one f16 step below: finer grid too
    1.5 + 2.0 ** -10,                     # one f16 step above: the coarser grid
    96.0,                                 # 1.5 * 2^6
    1.5 + 2.0 ** -12,                     # fp32 above 1.5 that rounds DOWN to f16 1.5: the rule reads the f16 bits
    1.5 + 2.0 ** -11 + 2.0 ** -20,        # rounds UP to 1.5 + one step
    1.99999,                              # rounds up into the next binade: f16 2.0
    255.97,                               # ... f16 256.0 (spacing 0.125 below it)
    3e-6,                                 # f16 subnormal
    6.0e-5,                               # just below the smallest normal f16 (2^-14 = 6.1035e-5)
    0.0,                                  # all-zero block
    -5.0,                                 # negative value of largest magnitude
    70000.0,                              # overflows f16: inf
    65520.0,                              # the tie between 65504 and 2^16: rounds to inf
    65519.0,                              # rounds to the largest finite f16
    2.0 ** -14,                           # the smallest normal f16: exponent field 1, mantissa 0
]
_FILL = [0.61, -0.33, 0.2, 0.87, -0.05, 0.45, 0.0, 0.99, -0.72, 0.13, 0.5, -0.25, 0.66, 0.31, -0.9]


def _edge_bias():
    b = torch.zeros(16, 16)
    for k, m in enumerate(_EDGE_MAXIMA):
        pos = (5 * k + 3) % 16
        fill = iter(_FILL)
        for j in range(16):
            b[k, j] = m if j == pos else abs(m) * next(fill)
    return b.reshape(-1)


_BIAS = {"positions": _position_bias, "edges": _edge_bias}


def _expected(vals):
    """per block (chunk, 16): f16 bits, E, the nibbles of the f16 parts and of the residuals of the 256 stored values -- planar_q_parts, with the
    one case it does not cover restated: a block whose largest f16 part is inf (bits 0x7C00: exponent field 31, mantissa 0) has E = 31 - 16 - 1 = 14,
    which is also E of 65504."""
    xc = vals.reshape(COUT // 16, 16).float()
    hi = xc.half()
    amax = hi.float().abs().amax(dim=-1)
    e = q_block_exp(amax.clamp_max(65504.0))
    sc = torch.exp2(e)[..., None]
    ch, cr = fp4_codes(hi.float() / sc), fp4_codes((xc - hi.float()) * 2048.0 / sc)
    fin = torch.isfinite(amax)                                       # every other block: the helper itself is the reference
    h2, c2, r2, e2 = planar_q_parts(vals.reshape(1, COUT, 1, 1))
    assert torch.equal(h2[0, :, 0, 0][fin].view(torch.int16), hi[fin].view(torch.int16)) and torch.equal(e2[0, :, 0, 0][fin], e[fin])
    assert torch.equal(c2[0, :, 0, 0][fin], ch[fin]) and torch.equal(r2[0, :, 0, 0][fin], cr[fin])
    return hi, e, ch, cr


def _assert_q_is(t, vals, what):
    """every pixel of the planar Q tensor t holds exactly the encoding of `vals` (256 values, one per channel)"""
    _, hi, ch, cr, e = planar_q_decode(t, parts=True)
    xh, xe, xch, xcr = (v.to(hi.device) for v in _expected(vals))
    assert hi.shape[1] == COUT // 16 and hi.shape[2] * hi.shape[3] > 0
    bad = lambda got, want: float((got != want[None, :, None, None]).float().mean())
    f = {"f16 planes": bad(hi.view(torch.int16), xh.view(torch.int16)), "scale bytes": float((e != xe[None, :, None, None]).float().mean()),
         "f16 parts' nibbles": bad(ch, xch), "residual nibbles": bad(cr, xcr)}
    print(f"[epilogue lean {what}] differing fractions: {f}")
    if f["f16 planes"]:
        d = (hi.view(torch.int16)[0, :, 0, 0] != xh.view(torch.int16)).nonzero()
        print("  first pixel, (block, position): stored f16 / expected f16 / value:",
              [(int(k), int(j), float(hi[0, k, 0, 0, j]), float(xh[k, j]), float(vals.reshape(-1, 16)[k, j])) for k, j in d[:8]])
    for k, v in f.items():
        assert v == 0.0, (what, k, v)


@functools.lru_cache(maxsize=None)
def _q_inputs(cin, h, w):
    from ws_unet_amd import ops
    xq = planar_q_encode(torch.rand((1, cin, h, w), generator=torch.Generator().manual_seed(7)))
    return xq, ops.pack_conv3x3_f4(torch.zeros((COUT, cin, 3, 3), device=DEV))


@pytest.mark.parametrize("pattern", ["positions", "edges"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("cin,h,w", [(16, 16, 32),         # one tile, half-block work items, one chunk step per tile
                                     (64, 34, 66)])       # nine tiles, the last row and column past the image: the store predicates
def test_q_controlled_blocks(cin, h, w, pool, relu, pattern):
    from ws_unet_amd import ops
    bias = _BIAS[pattern]()
    vals = torch.relu(bias + 0.0) if relu else bias + 0.0         # what the epilogue sees: accumulator (+0) + bias, so a bias of -0 is stored as +0
    xq, wp = _q_inputs(cin, h, w)
    out = ops.conv3x3_q(xq, None, wp, bias.to(DEV), COUT, relu=relu, pool=pool, y_format=ops.PLANAR_Q)
    torch.cuda.synchronize()
    what = f"q {cin}ch {h}x{w} pool={pool} relu={relu} {pattern}"
    _assert_q_is(out[0] if pool else out, vals, what + " y")
    if pool:
        assert (out[1].h, out[1].w) == (h // 2, w // 2)
        _assert_q_is(out[1], vals, what + " y_pool")                  # the pool of a constant plane is the constant


@pytest.mark.parametrize("pattern", ["positions", "edges"])
@pytest.mark.parametrize("relu", [True, False])
def test_up_q_controlled_blocks(relu, pattern):
    from ws_unet_amd import ops
    hl, wl, cl, cup, c2 = 10, 20, 16, 16, 16
    bias = _BIAS[pattern]()
    vals = torch.relu(bias + 0.0) if relu else bias + 0.0         # what the epilogue sees: accumulator (+0) + bias, so a bias of -0 is stored as +0
    w_skip, w_low, _ = ops.pack_conv3x3_up(torch.zeros((COUT, cup + c2, 3, 3), device=DEV), torch.zeros((cl, cup, 2, 2), device=DEV), None, None)
    g = torch.Generator().manual_seed(8)
    ql, qs = planar_q_encode(torch.rand((1, cl, hl, wl), generator=g)), planar_q_encode(torch.rand((1, c2, 2 * hl, 2 * wl), generator=g))
    y = ops.conv3x3_up_q(ql, qs, w_skip, w_low, bias.to(DEV), COUT, relu=relu)
    torch.cuda.synchronize()
    assert (y.h, y.w) == (2 * hl, 2 * wl)
    _assert_q_is(y, vals, f"up_q relu={relu} {pattern}")


# ---- the range flag: `!(|x| <= 448)` on the fp32 value, now from the encode's own maximum -------------------------------------------------------

@pytest.mark.parametrize("channel", [2, 9, 5, 14])          # lanes 0-31: X = ch 0-3, Y = ch 8-11; lanes 32-63: X = ch 4-7, Y = ch 12-15
@pytest.mark.parametrize("value,flag", [(448.0, 0), (448.1, 1), (448.25, 1), (float("nan"), 1)])
def test_range_flag_single_channel(value, flag, channel):
    """one channel of one block carries the value (448.1 rounds to 448.0 in f16: the test must stay on the fp32 value; a NaN counts where no ReLU
    replaces it), every other channel 1.0: plain and pooled format-Q outputs, the head variant's y, the fused decoder entry"""
    from ws_unet_amd import ops
    n, h, w, cin, cout = 1, 20, 40, 32, 64
    xq = planar_q_encode(torch.rand((n, cin, h, w), generator=torch.Generator().manual_seed(5)))
    wp = ops.pack_conv3x3_f4(torch.zeros((cout, cin, 3, 3), device=DEV))
    bias = torch.ones(cout)
    bias[16 * (channel % 4) + channel] = value
    bias = bias.to(DEV)
    hw_, hb = torch.full((1, cout, 1, 1), 0.01, device=DEV), torch.zeros(1, device=DEV)
    relus = (False,) if value != value else (False, True)
    for relu in relus:
        for kw in ({}, {"pool": True}, {"pool": True, "want_y": False}, {"head_w": hw_, "head_b": hb, "want_y": True}):
            rf = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.conv3x3_q(xq, None, wp, bias, cout, relu=relu, range_flag=rf, **kw)
            assert int(rf.item()) == flag, (value, channel, relu, sorted(kw))
        hl, wl, cl, cup, c2 = 10, 20, 16, 16, 16
        w_skip, w_low, _ = ops.pack_conv3x3_up(torch.zeros((cout, cup + c2, 3, 3), device=DEV), torch.zeros((cl, cup, 2, 2), device=DEV), None, None)
        g = torch.Generator().manual_seed(6)
        ql, qs = planar_q_encode(torch.rand((n, cl, hl, wl), generator=g)), planar_q_encode(torch.rand((n, c2, 2 * hl, 2 * wl), generator=g))
        rf = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.conv3x3_up_q(ql, qs, w_skip, w_low, bias, cout, relu=relu, range_flag=rf)
        assert int(rf.item()) == flag, (value, channel, relu, "up_q")


# ---- the head variant (one plane: `o < head_cout` is a compile-time test) ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _head_small():
    x, wgt, b = _operands(1, 34, 66, 64, 64, seed=61)
    return x, wgt, b, torch.relu(_conv3x3_q_ref(x, wgt, b))


@pytest.mark.parametrize("case", ["34x66", "5x128x256"])
def test_q_head_variant_one_plane(case):
    """64 -> 64 + the 1-plane head: nine tiles with the last row and column past the image, with y beside the head; and several tiles per workgroup,
    the head alone (the network's last layer).  Bounds of test_q_head_variant."""
    from ws_unet_amd import ops
    x, wgt, b, act = _head_small() if case == "34x66" else _walk_case()
    want_y = case == "34x66"
    g = torch.Generator().manual_seed(62)
    hw_, hb = torch.randn((1, 64, 1, 1), generator=g) * 0.2, torch.randn(1, generator=g) * 0.1
    ref = torch.sigmoid(F.conv2d(act, hw_, hb))
    res = ops.conv3x3_q(planar_q_encode(x), None, ops.pack_conv3x3_f4(wgt.to(DEV)), b.to(DEV), 64, head_w=hw_.to(DEV), head_b=hb.to(DEV), want_y=want_y)
    torch.cuda.synchronize()
    out = res[0] if want_y else res
    err = float((out.cpu() - ref).abs().max())
    print(f"[epilogue lean head {case}] max |sigmoid - emulation| = {err:.2e}")
    assert err < 2e-5, err
    if want_y:
        assert float((planar_decode(res[1]) - act).abs().max()) < 3e-5 * float(act.abs().max())
