"""The fixed per-step and per-tile parts of conv3x3_q / conv3x3_qu (csrc/conv3x3_q.hip, conv3x3_qu.hip): the lane offsets of a step formed in
front of its barrier with running slot counters, and a tile's first matrix unit taking a literal zero for C instead of cleared accumulators.
What can go wrong there shows where a workgroup walks several tiles (the counters run on across tiles, the accumulators of tile k + 1 must not see
tile k), where a tile has ONE step (its first step is its split last step), in the half-block and head instantiations, in both step kinds of the
fused decoder entry, in format H, and in the range flag (unchanged: `!(|x| <= limit)` on the fp32 value).  The checkers
restate the arithmetic on the CPU with the format helpers of gpu_util, with the tolerances of test_gpu_q / test_gpu_qu / test_gpu_f16p: they
follow from the storage formats, not from the shape."""
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_util import (DEV, fp4_codes, fp4_values, planar_decode, planar_h_decode, planar_h_encode, planar_q_decode, planar_q_encode,
                      planar_q_parts, q_block_exp)

pytestmark = pytest.mark.gpu


# ---- the arithmetic and the storage formats restated on the CPU, on the format helpers of gpu_util (fp64 accumulation) ------------------------

def _blocks_to_nchw(t):                                    # (n, chunk, h, w, 16) -> (n, c, h, w)
    n, nch, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, nch * 16, h, w)


def _q_conv_terms(xp, w):
    """the three product families of the fp4-cross-term arithmetic for a VALID conv of the padded input xp with w (any kernel size):
    f16(w) f16(x) + fp4(w residual) fp4(f16 x) + fp4(f16 w) fp4(x residual); blocks = 16 channels per pixel / per (co, tap) (include/wsu.h K1q)"""
    hi, ch, cr, e = planar_q_parts(xp)
    sc = torch.exp2(e)[..., None]
    xh, xc4, xr4 = _blocks_to_nchw(hi.float()), _blocks_to_nchw(fp4_values(ch) * sc), _blocks_to_nchw(fp4_values(cr) * sc / 2048.0)
    co, ci, kh, kw = w.shape
    whi, wch, wcr, we = planar_q_parts(w.permute(0, 2, 3, 1).contiguous().reshape(co * kh * kw, ci, 1, 1))
    wsc = torch.exp2(we)[..., None]
    back = lambda t: _blocks_to_nchw(t).reshape(co, kh, kw, ci).permute(0, 3, 1, 2)
    wh, wc4, wr4 = back(whi.float()), back(fp4_values(wch) * wsc), back(fp4_values(wcr) * wsc / 2048.0)
    return F.conv2d(xh.double(), wh.double()) + F.conv2d(xc4.double(), wr4.double()) + F.conv2d(xr4.double(), wc4.double())


def _conv3x3_q_ref(x, w, b):
    return (_q_conv_terms(F.pad(x, (1, 1, 1, 1), mode="reflect"), w) + b.double()[None, :, None, None]).float()


def _up_q_ref(xl, xs, w3, wc, bias, cup):
    """the fused decoder entry: 3x3 terms on the skip half + per parity class a 2x2-tap conv on the clamp-padded low tensor (include/wsu.h K1u)"""
    _, _, hl, wl = xl.shape
    y = _q_conv_terms(F.pad(xs, (1, 1, 1, 1), mode="reflect"), w3[:, cup:])
    xlp = F.pad(xl, (1, 1, 1, 1), mode="replicate")
    for py in range(2):
        for px in range(2):
            t = _q_conv_terms(xlp, wc[:, :, py, px].float())
            y[:, :, py::2, px::2] += t[:, :, py:py + hl, px:px + wl]
    return (y + bias.double()[None, :, None, None]).float()


def _q_roundtrip(v):
    """fp32 NCHW -> what a planar Q tensor keeps of it: f16 part + fp4 residual * 2^(E - 11)"""
    hi, _, cr, e = planar_q_parts(v)
    return _blocks_to_nchw(hi.float() + fp4_values(cr) * torch.exp2(e - 11)[..., None])


def _check_q_tensor(tq, ta, what):
    """A planar Q tensor against the e4m3-residual tensor `ta` the same kernel wrote from the same fp32 values: the f16 planes are the same bytes;
    block exponents and the f16 parts' fp4 nibbles are functions of the f16 planes -- exact; the residual nibbles come from the exact fp32
    residual while `ta` carries it rounded to e4m3 -- at most one grid step apart, on fewer than 8 % of the nibbles (1-5 % measured by test_gpu_q)."""
    _, hi, ch, cr, e = planar_q_decode(tq, parts=True)
    raw = ta.detach().contiguous().view(torch.uint8)                                        # (n, chunk, 3, h, w, 16)
    n, nch, _, h, w, _ = raw.shape
    hi_a = torch.stack([raw[:, :, 0], raw[:, :, 1]], dim=-2).contiguous().view(torch.float16).reshape(n, nch, h, w, 16)
    res_a = raw[:, :, 2].contiguous().view(torch.float8_e4m3fn).float() / 4096.0
    assert torch.equal(hi.view(torch.int16), hi_a.view(torch.int16)), what + ": f16 planes"
    e_a = q_block_exp(hi_a.float().abs().amax(dim=-1))
    assert torch.equal(e, e_a), what + ": scale bytes"
    sc = torch.exp2(e_a)[..., None]
    assert torch.equal(fp4_values(ch), fp4_values(fp4_codes(hi_a.float() / sc))), what + ": fp4 nibbles of the f16 parts"
    want = fp4_values(fp4_codes(res_a * 2048.0 / sc))
    d = (fp4_values(cr) - want).abs()
    step = torch.where(want.abs() >= 4, 2.0, torch.where(want.abs() >= 2, 1.0, 0.5))
    assert bool((d <= step).all()), what + ": a residual nibble is more than one grid step off"
    assert float((d > 0).float().mean()) < 0.08, (what, float((d > 0).float().mean()))


def _up_case(n, hl, wl, cl, cup, c2, cout, seed):
    g = torch.Generator().manual_seed(seed)
    xl = torch.relu(torch.randn((n, cl, hl, wl), generator=g)) * torch.exp2(torch.randint(-3, 4, (n, cl, 1, 1), generator=g).float())
    xs = torch.relu(torch.randn((n, c2, 2 * hl, 2 * wl), generator=g)) * torch.exp2(torch.randint(-3, 4, (n, c2, 1, 1), generator=g).float())
    wt = torch.randn((cl, cup, 2, 2), generator=g) * (1.0 / cl) ** 0.5
    bt = torch.randn(cup, generator=g) * 0.1
    w3 = torch.randn((cout, cup + c2, 3, 3), generator=g) * (2.0 / (9 * (cup + c2))) ** 0.5
    b3 = torch.randn(cout, generator=g) * 0.1
    return xl, xs, wt, bt, w3, b3


def r16(t):
    return t.half().float()


def conv_emul(x, w, b):
    """format H: the exact f16 products in fp64, reflect padding, + bias"""
    return F.conv2d(F.pad(r16(x).double(), (1, 1, 1, 1), mode="reflect"), r16(w).double(), b.double())


def _operands(n, h, w, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn((n, cin, h, w), generator=g)) * torch.exp2(torch.randint(-3, 4, (n, cin, 1, 1), generator=g).float())
    wgt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return x, wgt, b


@functools.lru_cache(maxsize=None)
def _walk_case():
    """n = 5, 64 -> 64 at 128 x 256: 320 tiles of 4 chunk steps on at most 256 workgroups -- the operands and the emulation, computed once"""
    x, wgt, b = _operands(5, 128, 256, 64, 64, seed=41)
    return x, wgt, b, torch.relu(_conv3x3_q_ref(x, wgt, b))


@functools.lru_cache(maxsize=None)
def _walk_case_h():
    x, wgt, b = _operands(5, 128, 256, 64, 64, seed=43)
    return x, wgt, b, torch.relu(conv_emul(r16(x), wgt, b))


def _check_q_conv(x, wgt, b, ref, pool, **kw):
    """conv3x3_q with the e4m3-residual output against the emulation (3e-5 of the output's scale: accumulation order and the store encoding, as
    test_gpu_q), the pooled output against the pool of the stored one, and the planar Q output of the same launch shape against those bytes"""
    from ws_unet_amd import ops
    cout = wgt.shape[0]
    wp, xq, bd = ops.pack_conv3x3_f4(wgt.to(DEV)), planar_q_encode(x), b.to(DEV)
    out = ops.conv3x3_q(xq, None, wp, bd, cout, pool=pool, y_format=ops.PLANAR_A, **kw)
    torch.cuda.synchronize()
    ya = out[0] if pool else out
    y = planar_decode(ya)
    scale = float(ref.abs().max())
    err = float((y - ref).abs().max())
    print(f"[fixed costs q {tuple(x.shape)} -> {cout} pool={pool}] max |y - emulation| = {err / scale:.2e} of the scale")
    assert err < 3e-5 * scale, err / scale
    outq = ops.conv3x3_q(xq, None, wp, bd, cout, pool=pool, y_format=ops.PLANAR_Q, **kw)
    _check_q_tensor(outq[0] if pool else outq, ya, "y")
    if pool:
        assert float((planar_decode(out[1]) - F.max_pool2d(y, 2)).abs().max()) == 0.0
        _check_q_tensor(outq[1], out[1], "y_pool")


@pytest.mark.parametrize("pool", [False, True])
def test_q_workgroups_walk_several_tiles(pool):
    x, wgt, b, ref = _walk_case()
    _check_q_conv(x, wgt, b, ref, pool)


@pytest.mark.parametrize("n,h,w", [
    (1, 16, 32),                              # one tile: half-block work items (MSPLIT), J = 1
    (1, 34, 66),                              # nine tiles, those of the last row and column past the image (half-block items too)
    (16, 34, 66),                             # 144 tiles: whole-block items, the single step is the split last step of every tile
])
def test_q_one_chunk_per_tile(n, h, w):
    x, wgt, b = _operands(n, h, w, 16, 64, seed=100 + n + h)
    _check_q_conv(x, wgt, b, torch.relu(_conv3x3_q_ref(x, wgt, b)), pool=False)


def test_q_head_variant():
    """64 -> 64 with the fused 1x1 head (1 plane), tiles past the image, more work items than half the device would split"""
    from ws_unet_amd import ops
    n, h, w = 3, 40, 72
    x, wgt, b = _operands(n, h, w, 64, 64, seed=47)
    g = torch.Generator().manual_seed(48)
    hw_, hb = torch.randn((1, 64, 1, 1), generator=g) * 0.2, torch.randn(1, generator=g) * 0.1
    act = torch.relu(_conv3x3_q_ref(x, wgt, b))
    ref = torch.sigmoid(F.conv2d(act, hw_, hb))
    xq, wp = planar_q_encode(x), ops.pack_conv3x3_f4(wgt.to(DEV))
    out, ya = ops.conv3x3_q(xq, None, wp, b.to(DEV), 64, head_w=hw_.to(DEV), head_b=hb.to(DEV), want_y=True)
    torch.cuda.synchronize()
    err = float((out.cpu() - ref).abs().max())
    print(f"[fixed costs q head] max |sigmoid - emulation| = {err:.2e}")
    assert err < 2e-5, err                                            # the bound of test_gpu_q's head cases
    assert float((planar_decode(ya) - act).abs().max()) < 3e-5 * float(act.abs().max())


@pytest.mark.parametrize("n", [1, 80])       # 4 tiles per image: one tile per workgroup / 320 tiles, a second tile for a quarter of the workgroups
def test_up_q_one_skip_chunk_one_low_chunk(n):
    """the fused decoder entry with the shortest K loop: one step of each kind per tile, 32 x 64 output pixels"""
    from ws_unet_amd import ops
    hl, wl, cl, cup, c2, cout = 16, 32, 16, 16, 16, 64
    xl, xs, wt, bt, w3, b3 = _up_case(n, hl, wl, cl, cup, c2, cout, seed=53)
    xu = F.conv_transpose2d(xl.double(), wt.double(), bt.double(), stride=2)
    exact = torch.relu(F.conv2d(F.pad(torch.cat([xu, xs.double()], 1), (1, 1, 1, 1), mode="reflect"), w3.double(), b3.double())).float()
    w_skip, w_low, bias, dense = ops.pack_conv3x3_up(w3.to(DEV), wt.to(DEV), bt.to(DEV), b3.to(DEV), want_dense=True)
    y = ops.conv3x3_up_q(planar_q_encode(xl), planar_q_encode(xs), w_skip, w_low, bias, cout)
    torch.cuda.synchronize()
    got = planar_q_decode(y)
    scale = float(exact.abs().max())
    ref = torch.relu(_up_q_ref(xl, xs, w3, dense.cpu(), bias.cpu(), cup))
    d = (got - _q_roundtrip(ref)).abs()                               # through the same encoding: the bounds of test_gpu_qu
    frac = float((d > 3e-5 * scale).float().mean())
    print(f"[fixed costs up_q n={n}] beyond 3e-5: {frac:.2e}, max {float(d.max()) / scale:.2e}, vs emulation {float((got - ref).abs().max()) / scale:.2e}, vs exact {float((got - exact).abs().max()) / scale:.2e}")
    assert frac < 0.02, frac
    assert float(d.max()) < 2.5e-4 * scale and float((got - ref).abs().max()) < 1.6e-4 * scale
    assert float((got - exact).abs().max()) < 5e-4 * scale


def _check_h_conv(x, wgt, b, act, pool):
    """conv3x3_h against the fp64 sum of its exact f16 products: the bounds of test_gpu_f16p (one f16 rounding step, on a few values)"""
    from ws_unet_amd import ops
    cout = wgt.shape[0]
    rf = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = ops.conv3x3_h(planar_h_encode(x), None, ops.pack_conv3x3_h(wgt.to(DEV)), b.to(DEV), cout, pool=pool, range_flag=rf)
    torch.cuda.synchronize()
    assert int(rf.item()) == 0
    y = res[0] if pool else res
    got, ref = planar_h_decode(y).double(), r16(act.float()).double()
    d = (got - ref).abs()
    print(f"[fixed costs h {tuple(x.shape)} -> {cout} pool={pool}] differing stored values {float((d > 0).double().mean()):.2e}, max {float(d.max()):.2e}")
    assert float((d > 0).double().mean()) <= 2e-3
    assert float(d.max()) <= float(ref.abs().max()) * 2 ** -10
    if pool:
        assert float((planar_h_decode(res[1]) - F.max_pool2d(planar_h_decode(y), 2)).abs().max()) == 0.0


@pytest.mark.parametrize("pool", [False, True])
def test_h_workgroups_walk_several_tiles(pool):
    x, wgt, b, act = _walk_case_h()
    _check_h_conv(x, wgt, b, act, pool)


@pytest.mark.parametrize("n,h,w", [(1, 16, 32), (1, 34, 66), (16, 34, 66)])
def test_h_one_chunk_per_tile(n, h, w):
    x, wgt, b = _operands(n, h, w, 16, 64, seed=200 + n + h)
    _check_h_conv(x, wgt, b, torch.relu(conv_emul(r16(x), wgt, b)), pool=False)


_NEXT_F16_ABOVE_448 = 448.25                 # f16 has 10 mantissa bits: spacing 2^-2 in [256, 512)


@pytest.mark.parametrize("value,flag", [(448.0, 0), (448.1, 1), (_NEXT_F16_ABOVE_448, 1), (float("nan"), 1)])
def test_range_flag_on_the_fp32_value(value, flag):
    """zero weights: every stored value is the bias.  The flag is `!(|x| <= 448)` on the fp32 value: 448.1 sets it although it rounds to 448.0
    in f16, and so does a NaN (no ReLU in these launches: the ReLU's max against zero would replace a NaN by 0 before the check)."""
    from ws_unet_amd import ops
    n, h, w, cin, cout = 2, 20, 40, 32, 64
    xq = planar_q_encode(torch.rand((n, cin, h, w), generator=torch.Generator().manual_seed(5)))
    wp = ops.pack_conv3x3_f4(torch.zeros((cout, cin, 3, 3), device=DEV))
    bias = torch.full((cout,), value, device=DEV)
    for kw in ({}, {"pool": True}, {"y_format": ops.PLANAR_A}):
        rf = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.conv3x3_q(xq, None, wp, bias, cout, relu=False, range_flag=rf, **kw)
        assert int(rf.item()) == flag, (value, kw)
    if value == value:                                                # with the ReLU: the same for every value that is a number
        rf = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.conv3x3_q(xq, None, wp, bias, cout, range_flag=rf)
        assert int(rf.item()) == flag, value
    # the fused decoder entry: its packed bias is an argument of the launch
    hl, wl, cl, cup, c2 = 10, 20, 16, 16, 16
    w_skip, w_low, _ = ops.pack_conv3x3_up(torch.zeros((cout, cup + c2, 3, 3), device=DEV), torch.zeros((cl, cup, 2, 2), device=DEV), None, None)
    g = torch.Generator().manual_seed(6)
    ql, qs = planar_q_encode(torch.rand((n, cl, hl, wl), generator=g)), planar_q_encode(torch.rand((n, c2, 2 * hl, 2 * wl), generator=g))
    rf = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.conv3x3_up_q(ql, qs, w_skip, w_low, bias, cout, relu=False, range_flag=rf)
    assert int(rf.item()) == flag, value
