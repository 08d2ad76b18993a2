"""The step head of conv3x3_q / conv3x3_qu (csrc/conv3x3_q.hip: begin_step, q4_reads; conv3x3_qu.hip: sync_step, skip_units): the five fp4
units of a step read through ONE set of lane bases formed in front of the step's barrier (the lane half's term -- the partner tap one column
on, or a row on and two columns back -- is a constant of the base) plus compile-time immediates, and lanes 32-63 of the ninth tap read
their zero operands from a zero block in LDS.  What can go wrong is a wrong immediate, a wrong lane-half term, or a zero block that is not
zero -- each reads a neighbouring pixel, tap, channel half or scale byte.

Exact tap isolation.  The weights carry ONE non-zero tap and one non-zero input channel per output channel, the inputs encode their position,
and every product family of the arithmetic (include/wsu.h K1q: f16 w * f16 x + fp4(w residual) * fp4(f16 x) + fp4(f16 w) * fp4(x residual)) is
exact on them, so the accumulators hold the fp64 conv exactly and the stored bytes are its encoding:
  * a pixel's 16-channel block is {0, .5, 1, 1.5, 2, 3, 4} * 2^s (fp4-exact under the block's scale; channel 15 = 4 * 2^s pins the scale): the
    digits are the base-7 digits of the pixel's index, s = (y + 2 x + chunk + image) % 4 - 1 -- one pixel or one row off changes a digit;
  * kind 'f16': nothing has a residual; 'wres': w = +-2^t (1 + 2^-14), a residual of exactly fp4 code 0.5; 'xres': every x >= 2^s carries a
    residual of exactly fp4 code 0.5 (+ 2^(s - 12)).  The cross term the arithmetic leaves out (w residual * x residual) is zero in each.
  * tap 8 with residuals is the case where a lane half of the ninth tap's unit that read real data would add a second product.
The restated terms (gpu_util's format helpers) are checked against the fp64 conv on the CPU before they are used.  Outputs are compared through
their own storage encoding (restated by gpu_util), with torch.equal; in format A ('F16F8P') the expected values are representable, so there
the comparison is with the fp64 conv itself.

(The half-block variant works on 32 output channels of a 64-channel block: it is what Cout = 64 and 128 run as on the small grids here.)
The fused decoder entry is checked against the CPU restatement and in the tolerances of test_gpu_fixed_costs.py (helpers copied from there),
format H runs the same cases once as the control (it has no fp4 unit)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_util import (DEV, _q_sblock_index, fp4_values, planar_decode, planar_encode, planar_h_decode, planar_h_encode, planar_q_decode, planar_q_encode,
                      planar_q_parts)

pytestmark = pytest.mark.gpu

KINDS = ("f16", "wres", "xres")
_DIGITS = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0], dtype=torch.float64)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _x(n, h, w, cin, xres, dev):
    """(n, cin, h, w) fp64 on `dev`: position-coded, fp4-exact blocks; xres: + the residual of fp4 code 0.5 where the digit is >= 1"""
    i, y, x = torch.meshgrid(torch.arange(n), torch.arange(h), torch.arange(w), indexing="ij")
    idx = (i * h + y) * w + x
    out = torch.empty((n, cin, h, w), dtype=torch.float64)
    for c in range(cin):
        k, j = divmod(c, 16)
        s = ((y + 2 * x + k + i) % 4 - 1).double()
        d = _DIGITS[(idx // 7 ** (j % 4) + 3 * (j // 4) + k) % 7] if j < 15 else torch.full(idx.shape, 4.0, dtype=torch.float64)
        out[:, c] = d * torch.exp2(s) + (torch.where(d >= 1, torch.exp2(s - 12), torch.zeros_like(s)) if xres else 0.0)
    return out.to(dev)


@functools.lru_cache(maxsize=None)
def _xq(n, h, w, cin, xres):
    """... and its planar Q tensor on the device (read-only: shared by the cases)"""
    return planar_q_encode(_x(n, h, w, cin, xres, DEV).float())


def _cmap(cin, cout):
    return [cin - 1 - (co % cin) for co in range(cout)]                          # the input channel of output channel co: every chunk is read


def _wvec(cout, wres):
    co = torch.arange(cout)
    v = torch.exp2((co % 5 - 2).double()) * torch.where(co % 3 == 0, -1.0, 1.0).double()
    return v * (1.0 + 2.0 ** -14) if wres else v


def _weights(cin, cout, tap, wres):
    w = torch.zeros((cout, cin, 3, 3), dtype=torch.float64)
    w[torch.arange(cout), torch.tensor(_cmap(cin, cout)), tap // 3, tap % 3] = _wvec(cout, wres)
    return w


def _conv_exact(x64, cin, cout, tap, wres):
    """the fp64 conv of the one-tap weights by gathering: out[co] = w[co] * x[c(co)] shifted by the tap, reflect padding"""
    xp = F.pad(x64, (1, 1, 1, 1), mode="reflect")
    h, w = x64.shape[2:]
    dy, dx = tap // 3, tap % 3
    sel = xp[:, torch.tensor(_cmap(cin, cout), device=x64.device), dy:dy + h, dx:dx + w]
    ref = sel * _wvec(cout, wres).to(x64.device)[None, :, None, None]
    assert torch.equal(ref.float().double(), ref)                              # an fp32 accumulator holds it
    return ref


# ---- the arithmetic restated on the format helpers of gpu_util (copied from test_gpu_fixed_costs.py) ------------------------------------------

def _blocks_to_nchw(t):
    n, nch, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, nch * 16, h, w)


def _q_conv_terms(xp, w):
    hi, ch, cr, e = planar_q_parts(xp)
    sc = torch.exp2(e)[..., None]
    xh, xc4, xr4 = _blocks_to_nchw(hi.float()), _blocks_to_nchw(fp4_values(ch) * sc), _blocks_to_nchw(fp4_values(cr) * sc / 2048.0)
    co, ci, kh, kw = w.shape
    whi, wch, wcr, we = planar_q_parts(w.permute(0, 2, 3, 1).contiguous().reshape(co * kh * kw, ci, 1, 1))
    wsc = torch.exp2(we)[..., None]
    back = lambda t: _blocks_to_nchw(t).reshape(co, kh, kw, ci).permute(0, 3, 1, 2)
    wh, wc4, wr4 = back(whi.float()), back(fp4_values(wch) * wsc), back(fp4_values(wcr) * wsc / 2048.0)
    return F.conv2d(xh.double(), wh.double()) + F.conv2d(xc4.double(), wr4.double()) + F.conv2d(xr4.double(), wc4.double())


def _up_q_ref(xl, xs, w3, wc, bias, cup):
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


# ---- the CPU confirmation: on these operands the three restated product families ARE the fp64 conv --------------------------------------------

@functools.lru_cache(maxsize=None)
def _confirmed(kind, tap):
    n, h, w, cin, cout = 2, 18, 35, 32, 64
    x = _x(n, h, w, cin, kind == "xres", "cpu")
    wgt = _weights(cin, cout, tap, kind == "wres")
    assert torch.equal(x.float().double(), x) and torch.equal(wgt.float().double(), wgt)
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect")
    conv = F.conv2d(xp, wgt)
    assert torch.equal(_conv_exact(x, cin, cout, tap, kind == "wres"), conv)                        # the gather is the conv
    assert torch.equal(_q_conv_terms(xp.float(), wgt.float()), conv)                                 # ... and so are the kernel's three families
    # each kind exercises the family it is named for
    hi, _, cr, _ = planar_q_parts(x.float())
    assert bool((fp4_values(cr) != 0).any()) == (kind == "xres") and torch.equal(_blocks_to_nchw(hi.float()).double() == x, ~(_blocks_to_nchw(fp4_values(cr)) != 0))
    _, _, wcr, _ = planar_q_parts(wgt.float().permute(0, 2, 3, 1).contiguous().reshape(cout * 9, cin, 1, 1))
    assert bool((fp4_values(wcr) != 0).any()) == (kind == "wres")
    return True


# ---- launches -------------------------------------------------------------------------------------------------------------------------------

def _bytes(t):
    """the bytes a launch writes: a plain tensor (format A, the head's plane), a planar H tensor, or a planar Q tensor without the scale plane's
    padding (a tile block of 512 scale bytes is written only where the image has pixels)"""
    if isinstance(t, torch.Tensor):
        return t.contiguous().view(torch.uint8).clone()
    if not hasattr(t, "h") or t.data.shape[-1] == 32 * t.h * t.w:
        return t.data.clone()
    hw = t.h * t.w
    return torch.cat([t.data[:, :, :48 * hw], t.data[:, :, (48 * hw + _q_sblock_index(t.h, t.w, t.data.device)).reshape(-1)]], dim=-1)


def _raw(o):
    return [_bytes(t) for t in (o if isinstance(o, tuple) else (o,))]


def _launch_twice(fn):
    a = fn()
    ra = _raw(a)
    b = fn()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(ra, _raw(b))), "two launches, different bytes"
    return a


def _assert_q(t, ref, what):
    got = planar_q_decode(t)
    want = _q_roundtrip(ref.float()).cpu()
    bad = (got != want)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist())


def _assert_a(t, ref, what):
    got = planar_decode(t)
    assert torch.equal(planar_decode(planar_encode(ref.float())).double(), ref.cpu()), what + ": the expected values are representable in format A"
    bad = (got.double() != ref.cpu())
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist())


# (n, h, w, cin, cout, variant): 1-5 chunk steps (3 and 5 put the three input slots and the two weight slots out of phase, 1 is the single-step
# tile); 16 x 32 = one tile, 34 x 66 = nine ragged tiles (half-block work items up to 128 of them); 16 / 15 images = whole-block work items, the
# split last step -- with one step per tile and with three
_CONFIGS = [
    (1, 16, 32, 16, 64, "q"),
    (1, 16, 32, 48, 64, "a"),
    (1, 34, 66, 32, 64, "pool"),
    (1, 34, 66, 64, 128, "norelu"),
    (1, 34, 66, 80, 128, "q"),
    (1, 34, 66, 80, 64, "a"),
    (16, 34, 66, 16, 64, "q"),
    (15, 34, 66, 48, 64, "pool-norelu"),
]


def _run_config(kind, tap, n, h, w, cin, cout, variant):
    from ws_unet_amd import ops
    wres, xres = kind == "wres", kind == "xres"
    x, xq = _x(n, h, w, cin, xres, DEV), _xq(n, h, w, cin, xres)
    wp = ops.pack_conv3x3_f4(_weights(cin, cout, tap, wres).float().to(DEV))
    relu, pool = "norelu" not in variant, "pool" in variant
    ref = _conv_exact(x, cin, cout, tap, wres)
    if relu:
        ref = torch.relu(ref)
    what = f"{kind} tap {tap} {n}x{cin}x{h}x{w}->{cout} {variant}"
    fmt = ops.PLANAR_A if variant == "a" else ops.PLANAR_Q
    out = _launch_twice(lambda: ops.conv3x3_q(xq, None, wp, None, cout, relu=relu, pool=pool, y_format=fmt))
    y = out[0] if pool else out
    (_assert_a if variant == "a" else _assert_q)(y, ref, what)
    if pool:
        _assert_q(out[1], F.max_pool2d(ref, 2), what + " y_pool")


@pytest.mark.parametrize("tap", range(9))
@pytest.mark.parametrize("kind", KINDS)
def test_one_tap(kind, tap):
    assert _confirmed(kind, tap)
    for cfg in _CONFIGS:
        _run_config(kind, tap, *cfg)


@pytest.mark.parametrize("cin", [16, 48])
@pytest.mark.parametrize("kind,tap", [("wres", 8), ("xres", 8), ("xres", 3), ("wres", 5), ("f16", 0)])
def test_second_tile_of_a_workgroup(kind, tap, cin):
    """5 x 128 x 256: 320 tiles on at most 256 workgroups -- a workgroup walks a second tile: the zero block and the slot counters survive a tile end"""
    assert _confirmed(kind, tap)
    _run_config(kind, tap, 5, 128, 256, cin, 64, "q")


@pytest.mark.parametrize("kind,tap", [("f16", 4), ("wres", 8), ("xres", 8), ("xres", 2)])
def test_head_variant(kind, tap):
    """the head instantiation: y beside the head is format A (exact), the head's plane is an fp32 sum of 64 products (the bound of test_gpu_q's
    head cases)"""
    from ws_unet_amd import ops
    assert _confirmed(kind, tap)
    n, h, w, cin, cout = 3, 40, 72, 48, 64
    x = _x(n, h, w, cin, kind == "xres", DEV)
    ref = torch.relu(_conv_exact(x, cin, cout, tap, kind == "wres"))
    g = torch.Generator().manual_seed(62)
    hw_, hb = torch.randn((1, 64, 1, 1), generator=g) * 0.05, torch.randn(1, generator=g) * 0.1
    xq, wp = _xq(n, h, w, cin, kind == "xres"), ops.pack_conv3x3_f4(_weights(cin, cout, tap, kind == "wres").float().to(DEV))
    out, ya = _launch_twice(lambda: ops.conv3x3_q(xq, None, wp, None, cout, head_w=hw_.to(DEV), head_b=hb.to(DEV), want_y=True))
    _assert_a(ya, ref, f"head {kind} tap {tap} y")
    want = torch.sigmoid(F.conv2d(ref.cpu(), hw_.double(), hb.double()))
    err = float((out.cpu().double() - want).abs().max())
    print(f"[step bases head {kind} tap {tap}] max |sigmoid - fp64| = {err:.2e}")
    assert err < 2e-5, err


# ---- format H: the same cases once, as the control (f16 products only: kind 'f16' is exact there too) --------------------------------------------

@functools.lru_cache(maxsize=None)
def _xh(n, h, w, cin):
    return planar_h_encode(_x(n, h, w, cin, False, "cpu").float())


def test_format_h_control():
    from ws_unet_amd import ops
    for tap in range(9):
        for n, h, w, cin, cout, variant in _CONFIGS:
            x, xh = _x(n, h, w, cin, False, DEV), _xh(n, h, w, cin)
            relu, pool = "norelu" not in variant, "pool" in variant
            ref = _conv_exact(x, cin, cout, tap, False)
            ref = torch.relu(ref) if relu else ref
            wp = ops.pack_conv3x3_h(_weights(cin, cout, tap, False).float().to(DEV))
            out = _launch_twice(lambda: ops.conv3x3_h(xh, None, wp, None, cout, relu=relu, pool=pool))
            y = out[0] if pool else out
            assert torch.equal(planar_h_decode(y).double(), ref.cpu()), (tap, n, h, w, cin, cout, variant)      # the values are f16 numbers
            if pool:
                assert torch.equal(planar_h_decode(out[1]).double(), F.max_pool2d(ref, 2).cpu())


# ---- the fused decoder entry: (skip chunks, low chunks) -- skip steps of every phase of the two regions, a low step between and behind them ----

_UP_CASES = [(s, l, hl, wl) for s, l in ((1, 1), (2, 1), (1, 2), (3, 2)) for hl, wl in ((8, 16), (17, 33))]


@pytest.mark.parametrize("nchs,nchl,hl,wl", _UP_CASES)
def test_up_q(nchs, nchl, hl, wl):
    """against the CPU restatement, in the tolerances of test_gpu_fixed_costs.test_up_q_one_skip_chunk_one_low_chunk"""
    from ws_unet_amd import ops
    n, cl, cup, c2, cout = 2, 16 * nchl, 16, 16 * nchs, 64
    xl, xs, wt, bt, w3, b3 = _up_case(n, hl, wl, cl, cup, c2, cout, seed=300 + 10 * nchs + nchl + hl)
    xu = F.conv_transpose2d(xl.double(), wt.double(), bt.double(), stride=2)
    exact = torch.relu(F.conv2d(F.pad(torch.cat([xu, xs.double()], 1), (1, 1, 1, 1), mode="reflect"), w3.double(), b3.double())).float()
    w_skip, w_low, bias, dense = ops.pack_conv3x3_up(w3.to(DEV), wt.to(DEV), bt.to(DEV), b3.to(DEV), want_dense=True)
    ql, qs = planar_q_encode(xl), planar_q_encode(xs)
    y = _launch_twice(lambda: ops.conv3x3_up_q(ql, qs, w_skip, w_low, bias, cout))
    got = planar_q_decode(y)
    scale = float(exact.abs().max())
    ref = torch.relu(_up_q_ref(xl, xs, w3, dense.cpu(), bias.cpu(), cup))
    d = (got - _q_roundtrip(ref)).abs()
    frac = float((d > 3e-5 * scale).float().mean())
    print(f"[step bases up_q S{nchs} L{nchl} {2 * hl}x{2 * wl}] beyond 3e-5: {frac:.2e}, max {float(d.max()) / scale:.2e}, vs emulation {float((got - ref).abs().max()) / scale:.2e}, vs exact {float((got - exact).abs().max()) / scale:.2e}")
    assert frac < 0.02, frac
    assert float(d.max()) < 2.5e-4 * scale and float((got - ref).abs().max()) < 1.6e-4 * scale
    assert float((got - exact).abs().max()) < 5e-4 * scale


@pytest.mark.parametrize("tap", range(9))
@pytest.mark.parametrize("kind", KINDS)
def test_up_q_one_skip_tap(kind, tap):
    """exact tap isolation through the skip half of the fused entry (its class planes: the tap offsets are the wave's, the lane half's choice a
    constant of the lane): zero transposed-conv weights leave the skip half alone; three skip chunks, nine ragged tiles"""
    from ws_unet_amd import ops
    assert _confirmed(kind, tap)
    n, hl, wl, cl, cup, c2, cout = 1, 17, 33, 16, 16, 48, 64
    xs = _x(n, 2 * hl, 2 * wl, c2, kind == "xres", DEV)
    w3 = torch.zeros((cout, cup + c2, 3, 3), dtype=torch.float64)
    w3[:, cup:] = _weights(c2, cout, tap, kind == "wres")
    w_skip, w_low, bias = ops.pack_conv3x3_up(w3.float().to(DEV), torch.zeros((cl, cup, 2, 2), device=DEV), None, None)
    ql, qs = _xq(n, hl, wl, cl, False), _xq(n, 2 * hl, 2 * wl, c2, kind == "xres")
    y = _launch_twice(lambda: ops.conv3x3_up_q(ql, qs, w_skip, w_low, bias, cout))
    _assert_q(y, torch.relu(_conv_exact(xs, c2, cout, tap, kind == "wres")), f"up_q {kind} tap {tap}")


def test_up_h_control():
    """format H through the fused-entry cases once (the bounds of test_gpu_f16p.test_conv3x3_up_h: one f16 rounding step, on a few values)"""
    from ws_unet_amd import ops
    for nchs, nchl, hl, wl in _UP_CASES:
        n, cl, cup, c2, cout = 2, 16 * nchl, 16, 16 * nchs, 64
        xl, xs, wt, bt, w3, b3 = _up_case(n, hl, wl, cl, cup, c2, cout, seed=300 + 10 * nchs + nchl + hl)
        xl, xs = r16(xl), r16(xs)
        wsk, wlo, bias, dense = ops.pack_conv3x3_up_h(w3.to(DEV), wt.to(DEV), bt.to(DEV), b3.to(DEV), want_dense=True)
        hl_, hs_ = planar_h_encode(xl), planar_h_encode(xs)
        y = _launch_twice(lambda: ops.conv3x3_up_h(hl_, hs_, wsk, wlo, bias, cout))
        got = planar_h_decode(y).double()
        wc = dense.cpu()
        emu = F.conv2d(F.pad(xs.double(), (1, 1, 1, 1), mode="reflect"), r16(w3[:, cup:]).double())
        xlp = F.pad(xl.double(), (1, 1, 1, 1), mode="replicate")
        for py in range(2):
            for px in range(2):
                t = F.conv2d(xlp, r16(wc[:, :, py, px]).double())
                emu[:, :, py::2, px::2] += t[:, :, py:py + hl, px:px + wl]
        emu = r16(torch.relu(emu + bias.cpu().double()[None, :, None, None]).float()).double()
        d = (got - emu).abs()
        assert float(d.max()) <= float(emu.abs().max()) * 2 ** -10, (nchs, nchl, hl, wl, float(d.max()))
        assert float((d > 0).double().mean()) <= 2e-3, (nchs, nchl, hl, wl, float((d > 0).double().mean()))
