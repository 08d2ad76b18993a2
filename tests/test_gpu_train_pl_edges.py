"""The pointwise kernels of the planar training path (csrc/train_pl.hip: max-pool backward, head backward, per-channel sums, first-layer weight and
data gradient, the reflect ring of the 3x3 data gradient) at their edges: every channel count the entries accept, one-window and one-row
images, rows narrower than a block's lane count, more rows than blocks, both grid-stride loops, constructed pool windows, the residual
planes under products 'f16', and every refused argument.

References are plain torch in float64 on the values the planar tensors hold (planar_decode(planar_encode(.))), as in
tests/test_gpu_planar_train.py, whose bands these tests keep; the two grid-stride cases compare with torch's own ops (the pool's on the
device in fp32).  The measured figure of every band stands next to it (MI355X; `pytest -s` prints them again)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, GRAD_LO, planar_decode, planar_encode
from ws_unet_amd import _lib, formula
from ws_unet_amd.model import get_model

pytestmark = pytest.mark.gpu

REL_L2 = 3e-4                     # tests/test_gpu_planar_train.py: one data-gradient layer against the exact adjoint
BOTH = ["f16f8", "f16"]


def _ops():
    from ws_unet_amd import ops
    return ops


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _rand_dev(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)


def _h(t):
    """what the f16 planes of a planar tensor hold for t (from fp64: through fp32, as a kernel's fp32 result is stored)"""
    return t.float().half().float()


def _q(t, lo):
    """the values a planar tensor holds for t"""
    return planar_decode(planar_encode(t, lo), lo)


def _decode_dev(t, lo, f16_only=False):
    """gpu_util.planar_decode without the copy to the host (the large cases and their fp64 sums stay on the device)"""
    raw = t.detach().contiguous().view(torch.uint8)
    n, nch, _, h, w, _ = raw.shape
    hi = torch.stack([raw[:, :, 0], raw[:, :, 1]], dim=-2).contiguous().view(torch.float16).reshape(n, nch, h, w, 16).float()
    lo_ = 0.0 if f16_only else raw[:, :, 2].contiguous().view(torch.float8_e4m3fn).float() / lo
    return (hi + lo_).permute(0, 1, 4, 2, 3).reshape(n, nch * 16, h, w)


def _live(t, products):
    """the planes of a planar gradient that `products` writes, as integers (bitwise comparison)"""
    return t[:, :, :2 if products == "f16" else 3].contiguous().view(torch.int32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. max-pool backward -------------------------------------------------------------------------------------------------------------------------
_A, _B = 1.0 + 2.0 ** -12, 1.0 + 3.0 * 2.0 ** -13          # one f16 part (1.0), residuals 1.0 and 1.5 e4m3 units of 2^-12: _B > _A


def _pool_patterns() -> torch.Tensor:
    """Windows in the order (0,0) (0,1) (1,0) (1,1).  The first 12: the maximum _B at i, the runner-up _A at j, which differ in the residual
    plane only, 1.0 and 0.5 elsewhere -- an argmax over the f16 parts sees a three-way tie and takes its first."""
    rows = []
    for i in range(4):
        for j in range(4):
            if i != j:
                r, rest = [0.0] * 4, [k for k in range(4) if k not in (i, j)]
                r[i], r[j], r[rest[0]], r[rest[1]] = _B, _A, 1.0, 0.5
                rows.append(r)
    rows += [[1.5] * 4,                                       # four-way tie: the first position wins
             [0.5, 2.0, 2.0, 1.0], [0.5, 1.0, 2.0, 2.0], [2.0, 1.0, 0.5, 2.0],      # ties at (1,2), (2,3), (0,3)
             [0.0] * 4,                                       # nothing is routed
             [0.0, 0.0, 2.0 ** -24, 0.0],                     # the smallest stored positive passes the mask and takes the gradient
             [-0.0, -0.0, 1.0, -0.0], [-0.0] * 4]             # -0.0 is not positive
    return torch.tensor(rows, dtype=torch.float32)


def _windows(t):
    n, c, h, w = t.shape
    return t.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)


def _unwindows(wn):
    n, c, hp, wp, _ = wn.shape
    return wn.reshape(n, c, hp, wp, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * hp, 2 * wp)


def _pool_ref(act, dyp, skip):
    """fp64: the gradient goes to the FIRST position of a window that holds its maximum; plus the skip gradient; times (act > 0)"""
    wn = _windows(act.double())
    ismax = wn == wn.amax(-1, keepdim=True)
    first = ismax & (ismax.cumsum(-1) == 1)
    routed = _unwindows(first * dyp.double()[..., None])
    return (routed + (skip.double() if skip is not None else 0.0)) * (act > 0)


POOL_SHAPES = [(1, 16, 2, 2),             # one window; c = 16: one lane pair per pixel (ncg >> 1 == 1)
               (3, 16, 6, 10),            # n > 2, odd pooled sizes 3 x 5
               (2, 48, 2, 66),            # one window row, odd pooled width 33, three chunks
               (1, 64, 34, 2),            # one window column, odd pooled height 17
               (2, 1024, 4, 4),           # the bottom of unet_4
               (1, 256, 8, 8)]


@functools.lru_cache(maxsize=2)
def _pool_case(n, c, h, w):
    act = _q(torch.relu(_rand((n, c, h, w), 12)), 4096.0)
    wn = _windows(act).reshape(-1, 4).clone()
    pat = _pool_patterns()
    step = 3 if wn.shape[0] >= 3 * len(pat) else 1            # every third window is a constructed one (all of them when there are few)
    idx = torch.arange(0, wn.shape[0], step)
    wn[idx] = pat[torch.arange(len(idx)) % len(pat)]
    act = _unwindows(wn.reshape(n, c, h // 2, w // 2, 4)).contiguous()
    assert torch.equal(_q(act, 4096.0), act)                  # every constructed value is exact in the format
    return act, _q(_rand((n, c, h, w), 13), GRAD_LO), _q(_rand((n, c, h // 2, w // 2), 14), GRAD_LO)


@pytest.mark.parametrize("products", BOTH)
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool2x2_pl_bwd_edges(shape, with_skip, products):
    """'f16': bitwise the f16 rounding of the exact sum.  'f16f8': max |got - ref| <= 2e-5 max|ref| + 1e-7, one re-encoding of an fp32 sum
    (half an e4m3 step of half an f16 step: 2^-16 = 1.5e-5 relative at most) -- measured 1.25e-5 at most."""
    ops = _ops()
    act, skip, dyp = _pool_case(*shape)
    f16 = products == "f16"
    sk, dy = (_h(skip), _h(dyp)) if f16 else (skip, dyp)      # 'f16': gradient tensors are f16 tensors
    ref = _pool_ref(act, dy, sk if with_skip else None)

    def run():
        g = ops.maxpool2x2_pl_bwd(planar_encode(skip, GRAD_LO) if with_skip else None, planar_encode(dyp, GRAD_LO), planar_encode(act), products=products)
        torch.cuda.synchronize()
        return g
    g = run()
    got = planar_decode(g, GRAD_LO, f16_only=f16)
    if f16:
        assert torch.equal(got, _h(ref))
    else:
        err, top = float((got - ref).abs().max()), float(ref.abs().max())
        print(f"pool_bwd {shape} skip={with_skip}: max err / max ref = {err / top:.2e}")
        assert err <= 2e-5 * top + 1e-7
    assert not bool((got[act <= 0] != 0).any())
    assert float(got.abs().max()) > 0
    assert torch.equal(_live(g, products), _live(run(), products))


@pytest.fixture(scope="module")
def pool_large():
    """(1, 256, 520, 512): 32 x 260 x 256 = 2 129 920 threads' worth of work for a grid capped at 8192 x 256 = 2 097 152 -- the last 32 768
    (pooled pixel, channel group) pairs, the end of the last channels, come from the second pass of the grid-stride loop."""
    n, c, h, w = 1, 256, 520, 512
    assert n * (c // 8) * (h // 2) * (w // 2) > 8192 * 256
    act = _decode_dev(planar_encode(torch.relu(_rand_dev((n, c, h, w), 101))), 4096.0)
    act[-1, -1, -2:, -2:] = torch.tensor([[1.0, _A], [0.5, _B]], device=DEV)         # the very last window: decided by the residual plane
    skip = _decode_dev(planar_encode(_rand_dev((n, c, h, w), 102), GRAD_LO), GRAD_LO)
    dyp = _decode_dev(planar_encode(_rand_dev((n, c, h // 2, w // 2), 103), GRAD_LO), GRAD_LO)
    a = act.clone().requires_grad_(True)
    pooled = F.max_pool2d(a, 2)
    routed = {f16: torch.autograd.grad(pooled, a, dyp.half().float() if f16 else dyp, retain_graph=True)[0] for f16 in (False, True)}
    del pooled, a
    yield {"act": act, "act_pl": planar_encode(act), "skip": skip, "dyp": dyp, "routed": routed}
    torch.cuda.empty_cache()


@pytest.mark.parametrize("products", BOTH)
@pytest.mark.parametrize("with_skip", [True, False])
def test_maxpool2x2_pl_bwd_grid_stride(pool_large, with_skip, products):
    """The grid-stride loop (68 M elements, the smallest shape past the grid cap) against torch's max_pool2d backward on the device; the bands of
    test_maxpool2x2_pl_bwd_edges -- measured 8.2e-6 'f16f8' on the whole tensor and on the last windows, equal bits 'f16'."""
    ops = _ops()
    p, f16 = pool_large, products == "f16"
    act, skip = p["act"], (p["skip"].half().float() if f16 else p["skip"])
    ref = p["routed"][f16] + skip if with_skip else p["routed"][f16].clone()
    ref *= act > 0
    g = ops.maxpool2x2_pl_bwd(planar_encode(p["skip"], GRAD_LO) if with_skip else None, planar_encode(p["dyp"], GRAD_LO), p["act_pl"], products=products)
    torch.cuda.synchronize()
    got = _decode_dev(g, GRAD_LO, f16_only=f16)
    if f16:
        ref = ref.half().float()
    tail = (slice(None), slice(-16, None), slice(-2, None))                         # the last window row of the last two chunks: second pass
    assert float(got[tail].abs().max()) > 0
    if f16:
        assert torch.equal(got[tail], ref[tail])
        assert torch.equal(got, ref)
    else:
        top = float(ref.abs().max())
        err, err_tail = float((got - ref).abs().max()), float((got[tail] - ref[tail]).abs().max())
        print(f"pool_bwd grid-stride skip={with_skip}: max err / max ref = {err / top:.2e}, last windows {err_tail / top:.2e}")
        assert err_tail <= 2e-5 * top + 1e-7
        assert err <= 2e-5 * top + 1e-7
    # the last window of all: its maximum _B sits at (1,1), ahead of _A at (0,1) by the residual alone
    assert float(got[-1, -1, -1, -1]) != (float(skip[-1, -1, -1, -1]) if with_skip else 0.0)
    for y, x in ((-2, -2), (-2, -1), (-1, -2)):
        assert float(got[-1, -1, y, x]) == (float(skip[-1, -1, y, x]) if with_skip else 0.0)
    assert float(got[act <= 0].abs().max()) == 0.0
    del got, ref


# ---- 2. head backward -----------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(2, 24, 40),
               (3, 700, 8)]               # n h = 2100 rows over 2048 blocks: 52 blocks walk two rows; w = 8 < the 128 / 64 / 32 / 16 pixel lanes of a group


@functools.lru_cache(maxsize=2)
def _head_case(cout, c, n, h, w):
    """fp64 autograd of sigmoid(conv2d).  dout has mean 1 so that no db[o] = sum dz[o] is a cancelled sum: a per-plane relative band would
    otherwise measure the conditioning of that sum, not the kernel."""
    x = _q(torch.relu(_rand((n, c, h, w), 15)), 4096.0)
    wh = _rand((cout, c, 1, 1), 16, 0.2)
    bh = _rand((cout,), 19, 0.3)
    dout = _rand((n, cout, h, w), 17, 3.0) + 1.0
    xa, wa, ba = x.double().requires_grad_(True), wh.double().requires_grad_(True), bh.double().requires_grad_(True)
    out = torch.sigmoid(F.conv2d(xa, wa, ba))
    out.backward(dout.double())
    return x, wh, out.detach().float().contiguous(), dout, xa.grad * (x > 0), wa.grad.reshape(cout, c), ba.grad


@pytest.mark.parametrize("products", BOTH)
@pytest.mark.parametrize("shape", HEAD_SHAPES)
@pytest.mark.parametrize("c", [16, 32, 64, 128])
@pytest.mark.parametrize("cout", [1, 2, 3, 4])
def test_conv1x1_sigmoid_pl_bwd_planes_and_channels(cout, c, shape, products):
    """Both instances of head_bwd_pl_kernel (one plane; 2..4 planes) at every accepted channel count.  g: relative L2 < 3e-5 ('f16f8', one
    encoding) / 3e-4 ('f16', one 2^-12 rounding per value) -- measured 5.0e-6 / 2.1e-4 at most; dw, db: < 1e-5 on every output plane alone
    -- measured dw 5.7e-8, db 1.0e-7 at most."""
    ops = _ops()
    f16 = products == "f16"
    x, wh, out, dout, ref_g, ref_dw, ref_db = _head_case(cout, c, *shape)
    xp = planar_encode(x)

    def run():
        r = ops.conv1x1_sigmoid_pl_bwd(xp, wh.to(DEV), out.to(DEV), dout.to(DEV), products=products)
        torch.cuda.synchronize()
        return r
    g, dw, db = run()
    assert tuple(dw.shape) == (cout, c, 1, 1) and tuple(db.shape) == (cout,)
    eg = rel_l2(planar_decode(g, GRAD_LO, f16_only=f16), ref_g)
    ew = [rel_l2(dw[o].reshape(-1).cpu(), ref_dw[o]) for o in range(cout)]
    eb = [abs(float(db[o]) - float(ref_db[o])) / abs(float(ref_db[o])) for o in range(cout)]
    print(f"head_bwd cout={cout} c={c} {shape} {products}: g {eg:.2e} dw {max(ew):.2e} db {max(eb):.2e}")
    assert eg < (3e-4 if f16 else 3e-5), eg
    for o in range(cout):                                     # a wrong plane must not hide in the norm of four
        assert ew[o] < 1e-5 and eb[o] < 1e-5, (o, ew, eb)
    g2, dw2, db2 = run()
    assert torch.equal(_live(g, products), _live(g2, products)) and torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("products", BOTH)
def test_three_plane_head_trains_on_the_planar_path(products):
    """A unet_1 with three output planes under a smooth loss: the planar training path (head_bwd_pl_kernel<4> closes its backward) against
    fp32 storage, every parameter's relative L2 < 2e-3 (ReLU-mask flips on rounding noise are the floor, test_gpu_planar_train.py) --
    measured 1.8e-4 ('f16f8') / 3.9e-4 ('f16'), both at e11.weight."""
    ops = _ops()
    sd = formula.formula_state_dict(1, "he", out_channels=3)
    model = get_model("unet_1", in_channels=1, out_channels=3, channel=[0], drop_rate=None, mode="f16f8p")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(DEV)
    model.train_products = products
    x = torch.rand((2, 1, 64, 96), generator=torch.Generator().manual_seed(3)).to(DEV)
    tgt = torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(4)).to(DEV)
    res, used = {}, {}
    for tm in ("f32", "f16f8p"):
        model.train_mode = tm
        model.zero_grad()
        timer = ops.KernelTimer()
        ops.set_timer(timer)
        try:
            ((model(x) - tgt) ** 2).mean().backward()
            torch.cuda.synchronize()
        finally:
            ops.set_timer(None)
        used[tm] = set(timer.summary())
        res[tm] = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters()}
    assert model.train_mode == "f16f8p"                       # no range fallback happened
    assert {"conv1x1_sigmoid_pl_bwd", "conv3x3_pl_bwd_data"} <= used["f16f8p"] and "conv1x1_sigmoid_pl_bwd" not in used["f32"], used
    errs = {k: rel_l2(res["f16f8p"][k], res["f32"][k]) for k in res["f32"]}
    print(f"three-plane unet_1 {products}: worst parameter {max(errs, key=errs.get)} {max(errs.values()):.2e}")
    assert tuple(res["f32"]["outconv.weight"].shape) == (3, 64, 1, 1)
    for k, e in errs.items():
        assert e < 2e-3, (k, e)


# ---- 3. channel sums and the first layer's weight gradient ----------------------------------------------------------------------------------------
SUM_SHAPES = [(2, 5, 7),                  # rows far narrower than the lanes of a group
              (3, 700, 8),                # 2100 rows over 2048 blocks
              (1, 40, 300)]               # rows wider than the lanes of a group: several pixels per lane


@pytest.mark.parametrize("products", BOTH)
@pytest.mark.parametrize("shape", SUM_SHAPES)
@pytest.mark.parametrize("c", [16, 32, 128, 512, 2048])       # 128 .. 1 pixel lanes per 8-channel group
def test_colsum_pl_channel_counts(c, shape, products):
    """Relative L2 against the fp64 sum of the decoded tensor < 2e-6 (fixed-order fp32 sums of at most 16 800 terms here, 76 800 in
    test_gpu_planar_train.py) -- measured 2.0e-7 at most."""
    ops = _ops()
    n, h, w = shape
    f16 = products == "f16"
    g = planar_encode(_rand_dev((n, c, h, w), 51), GRAD_LO)
    ref = _decode_dev(g, GRAD_LO, f16_only=f16).double().sum(dim=(0, 2, 3))
    got = ops.colsum_pl(g, products=products)
    torch.cuda.synchronize()
    e = rel_l2(got, ref)
    print(f"colsum_pl c={c} {shape} {products}: {e:.2e}")
    assert tuple(got.shape) == (c,) and e < 2e-6, e
    assert torch.equal(got, ops.colsum_pl(g, products=products))


@pytest.mark.parametrize("products", BOTH)
@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 3, 5), (1, 4, 2), (3, 700, 8), (2, 24, 40)])
@pytest.mark.parametrize("c", [16, 32, 128, 256])
def test_conv3x3_first_pl_bwd_weight_channel_counts(c, shape, products):
    """fp64 autograd of the reflect-padded conv (the smallest images reflect every tap): dw < 1e-5, db < 2e-6 -- measured dw 1.9e-7, db 1.9e-7 at most."""
    ops = _ops()
    n, h, w = shape
    f16 = products == "f16"
    g = planar_encode(_rand((n, c, h, w), 52), GRAD_LO)
    gq = planar_decode(g, GRAD_LO, f16_only=f16)
    img = torch.rand((n, 1, h, w), generator=torch.Generator().manual_seed(18))
    w1 = torch.zeros((c, 1, 3, 3), dtype=torch.float64, requires_grad=True)
    b1 = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    F.conv2d(F.pad(img.double(), (1, 1, 1, 1), mode="reflect"), w1, b1).backward(gq.double())
    dw, db = ops.conv3x3_first_pl_bwd_weight(g, img.to(DEV), products=products)
    torch.cuda.synchronize()
    ew, eb = rel_l2(dw.cpu(), w1.grad), rel_l2(db.cpu(), b1.grad)
    print(f"first_pl_bwd_weight c={c} {shape} {products}: dw {ew:.2e} db {eb:.2e}")
    assert tuple(dw.shape) == (c, 1, 3, 3) and ew < 1e-5 and eb < 2e-6, (ew, eb)
    dw2, none = ops.conv3x3_first_pl_bwd_weight(g, img.to(DEV), want_bias=False, products=products)
    assert none is None and torch.equal(dw, dw2)


# ---- 4. first-layer data gradient -----------------------------------------------------------------------------------------------------------------
def _frame(h, w):
    """rows and columns 0, 1, h-2, h-1 (w-2, w-1): where the reflect adjoint folds"""
    m = torch.zeros((h, w), dtype=torch.bool)
    m[[0, 1, h - 2, h - 1], :] = True
    m[:, [0, 1, w - 2, w - 1]] = True
    return m


def _first_dgrad_check(n, cin, c, h, w, products):
    ops = _ops()
    f16 = products == "f16"
    g = planar_encode(_rand((n, c, h, w), 61), GRAD_LO)
    gq = planar_decode(g, GRAD_LO, f16_only=f16)
    wgt = _rand((c, cin, 3, 3), 62, (2.0 / (9 * c)) ** 0.5)
    x = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
    F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), wgt.double()).backward(gq.double())
    dx = ops.conv3x3_first_pl_bwd_data(g, wgt.to(DEV), products=products)
    torch.cuda.synchronize()
    got, m = dx.cpu(), _frame(h, w)
    e, ef = rel_l2(got, x.grad), rel_l2(got[:, :, m], x.grad[:, :, m])
    print(f"first_pl_bwd_data n={n} cin={cin} c={c} {h}x{w} {products}: whole {e:.2e} frame {ef:.2e}")
    assert tuple(dx.shape) == (n, cin, h, w)
    assert e < 1e-5 and ef < 1e-5, (e, ef)
    assert torch.equal(dx, ops.conv3x3_first_pl_bwd_data(g, wgt.to(DEV), products=products))


@pytest.mark.parametrize("products", BOTH)
@pytest.mark.parametrize("n,cin,c,h,w", [
    (2, 1, 64, 2, 2),                     # every border branch coincides
    (1, 1, 16, 3, 3),                     # y == 1 == h - 2
    (1, 2, 32, 4, 4),
    (2, 3, 64, 3, 9),
    (1, 1, 64, 9, 4),
    (2, 1, 64, 24, 40),
    (1, 8, 256, 6, 10),                   # 73 728 B of weights in LDS: runs since the kernel's dynamic-LDS limit is raised
])
def test_conv3x3_first_pl_bwd_data_edges(n, cin, c, h, w, products):
    """fp64 autograd of conv2d(pad(x, reflect), w) driven by the decoded gradient; relative L2 < 1e-5 (the project's band for fixed-order fp32
    sums of this length: 9 c .. 36 c fused multiply-adds per output), on the whole tensor and on the border frame alone -- measured
    3.2e-7 at most on either (2.8e-7 whole / 2.6e-7 frame 'f16f8', 3.2e-7 / 3.1e-7 'f16'), so the 4x-the-fp32-floor allowance is not needed."""
    _first_dgrad_check(n, cin, c, h, w, products)


@pytest.mark.parametrize("products", BOTH)
def test_conv3x3_first_pl_bwd_data_grid_stride(products):
    """(1, 3, 16, 840, 840): 2 116 800 outputs for a grid capped at 8192 x 256 = 2 097 152 threads; the same band -- measured
    9.7e-8 whole, 9.9e-8 frame."""
    assert 3 * 840 * 840 > 8192 * 256
    _first_dgrad_check(1, 3, 16, 840, 840, products)


# ---- 5. the reflect ring of the 3x3 data gradient -------------------------------------------------------------------------------------------------
RING_SIZES = [(h, w) for h in (2, 3, 4, 5) for w in (2, 3, 4, 5)] + [(2, 40), (40, 2)]


@functools.lru_cache(maxsize=None)
def _ring_weights(cin, cout):
    ops = _ops()
    wgt = _rand((cout, cin, 3, 3), 1, (2.0 / (9 * cin)) ** 0.5)
    wd = wgt.to(DEV)
    return wgt, ops.pack_conv3x3(wd, ops.MODE_F16F8, dgrad=True), ops.pack_conv3x3_ring(wd)


@pytest.mark.parametrize("products", BOTH)
@pytest.mark.parametrize("h,w", RING_SIZES)
def test_conv3x3_pl_bwd_data_reflect_ring_sizes(h, w, products):
    """ring_gather_pl / ring_fold_pl for h - 2 and w - 2 in {0, 1, 2, > 2}: one and two gradients (fused concat), masked and not.  The
    assertions of test_conv3x3_pl_bwd_data ('f16': against the adjoint of the f16-rounded operands, as ..._f16_products), on the whole
    tensor and on rows 1, h-2 / columns 1, w-2 alone: relative L2 < 3e-4, max error < 2e-3 max|ref|.
    Measured 'f16f8': relative L2 <= 1.3e-5, max 2.1e-5 at every size.
    Measured 'f16': relative L2 2.3e-4 .. 2.93e-4 (whole and ring alike at the all-ring sizes), max <= 6.3e-4.  One f16 rounding costs
    2.1e-4 relative L2 and a ring pixel takes two (the main conv's stored result, the folded sum): f16(f16(zero-pad adjoint) + ring part)
    in exact fp64 arithmetic gives 2.3e-4 .. 2.9e-4 at these sizes.  A third rounding -- the strips' conv outputs stored as f16, as they
    were until the strips kept their residual plane -- gives 2.8e-4 .. 3.4e-4 and missed this band at 14 of the 18 sizes (measured
    2.6e-4 .. 3.2e-4).  Against the unrounded adjoint, the 5e-4 of ..._f16_products: measured 4.4e-4 at most ('f16f8', held to 3e-4: 1.3e-5)."""
    ops = _ops()
    n, cout, f16 = 2, 32, products == "f16"
    ring = torch.zeros((h, w), dtype=torch.bool)
    ring[[1, h - 2], :] = True
    ring[:, [1, w - 2]] = True
    missed = []
    for cin, csplit in ((64, 64), (128, 64)):
        wgt, wp, wr = _ring_weights(cin, cout)
        g = _q(_rand((n, cout, h, w), 2), GRAD_LO)
        act = torch.relu(_rand((n, cin, h, w), 3))
        x = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
        F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), (_h(wgt) if f16 else wgt).double()).backward((_h(g) if f16 else g).double())
        xu = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)      # the adjoint of the unrounded operands
        F.conv2d(F.pad(xu, (1, 1, 1, 1), mode="reflect"), wgt.double()).backward(g.double())
        for masked in (False, True):
            ref = x.grad * (act > 0) if masked else x.grad
            m1 = planar_encode(act[:, :csplit]) if masked else None
            m2 = planar_encode(act[:, csplit:]) if (masked and csplit < cin) else None
            dx1, dx2 = ops.conv3x3_pl_bwd_data(planar_encode(g, GRAD_LO), wp, wr, cin, csplit, m1, m2, pad_zero=False, products=products)
            torch.cuda.synchronize()
            assert (dx2 is None) == (csplit == cin)
            got = planar_decode(dx1, GRAD_LO, f16_only=f16)
            if dx2 is not None:
                got = torch.cat([got, planar_decode(dx2, GRAD_LO, f16_only=f16)], dim=1)
            what = (h, w, cin, masked, products)
            for name, sel in (("whole", slice(None)), ("ring", ring)):
                a, b = got[:, :, sel], ref[:, :, sel]
                e, emax = rel_l2(a, b), float((a - b).abs().max()) / float(b.abs().max())
                print(f"ring {what} {name}: rel L2 {e:.2e} max {emax:.2e}")
                if not e < REL_L2:
                    missed.append((what, name, "rel L2", e))
                if not emax < 2e-3:
                    missed.append((what, name, "max", emax))
            eu = rel_l2(got, xu.grad * (act > 0) if masked else xu.grad)
            print(f"ring {what} unrounded: rel L2 {eu:.2e}")
            if not eu < (5e-4 if f16 else REL_L2):
                missed.append((what, "unrounded", eu))
            if masked:
                assert float(got[act <= 0].abs().max()) == 0.0, what
    assert not missed, missed                                 # (every configuration is measured before the first miss is reported)


# ---- 6. products 'f16': the gradients' residual planes are neither read nor written ------------------------------------------------------------
SENTINEL = 0xA5                                               # pre-filled into every planar output
BIG_E4M3 = 0x7E                                               # e4m3 448: 448 / 2^14 = 0.027 on top of every value, were the plane read


def _plane2(t, byte):
    t = t.clone()
    t.view(torch.uint8)[:, :, 2] = byte
    return t


def _grad_out(n, c, h, w):
    t = torch.empty(_ops().planar_shape(n, c, h, w), dtype=torch.float32, device=DEV)
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def _f16_pool(byte):
    ops, lib = _ops(), _lib.load()
    n, c, h, w = 2, 32, 6, 10
    act = planar_encode(torch.relu(_rand((n, c, h, w), 71)))
    skip = _plane2(planar_encode(_rand((n, c, h, w), 72), GRAD_LO), byte)
    dyp = _plane2(planar_encode(_rand((n, c, h // 2, w // 2), 73), GRAD_LO), byte)
    g = _grad_out(n, c, h, w)
    ops.check(lib.wsu_maxpool2x2_pl_bwd(skip.data_ptr(), dyp.data_ptr(), act.data_ptr(), g.data_ptr(), n, h, w, c, ops.products_id("f16"), _stream()), "wsu_maxpool2x2_pl_bwd")
    g_alias = ops.maxpool2x2_pl_bwd(skip.clone(), dyp, act, products="f16")        # written in place of the skip gradient: its plane 2 stays
    assert bool((g_alias.view(torch.uint8)[:, :, 2] == byte).all())
    assert torch.equal(_live(g_alias, "f16"), _live(g, "f16"))
    return [_live(g, "f16")], [g]


def _f16_head(byte):
    ops, lib = _ops(), _lib.load()
    x, wh, out, dout, *_ = _head_case(3, 32, 2, 5, 7)
    n, c, h, w = x.shape
    g, dw, db = _grad_out(n, c, h, w), torch.empty((3, c), device=DEV), torch.empty(3, device=DEV)
    ws = torch.empty(lib.wsu_head_pl_bwd_workspace_bytes(c, 3) // 4, device=DEV)
    xp, wd, od, dd = planar_encode(x), wh.reshape(3, c).contiguous().to(DEV), out.to(DEV), dout.to(DEV)
    ops.check(lib.wsu_conv1x1_sigmoid_pl_bwd(xp.data_ptr(), wd.data_ptr(), od.data_ptr(), dd.data_ptr(), g.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                             ws.data_ptr(), ws.numel() * 4, n, h, w, c, 3, ops.products_id("f16"), _stream()), "wsu_conv1x1_sigmoid_pl_bwd")
    return [_live(g, "f16"), dw, db], [g]                     # (takes no gradient tensor: only its output side is under test)


def _f16_colsum(byte):
    return [_ops().colsum_pl(_plane2(planar_encode(_rand((2, 32, 5, 7), 74), GRAD_LO), byte), products="f16")], []


def _f16_first_weight(byte):
    g = _plane2(planar_encode(_rand((2, 32, 5, 7), 75), GRAD_LO), byte)
    img = torch.rand((2, 1, 5, 7), generator=torch.Generator().manual_seed(76)).to(DEV)
    return list(_ops().conv3x3_first_pl_bwd_weight(g, img, products="f16")), []


def _f16_first_data(byte):
    g = _plane2(planar_encode(_rand((2, 32, 5, 7), 77), GRAD_LO), byte)
    return [_ops().conv3x3_first_pl_bwd_data(g, _rand((32, 2, 3, 3), 78, 0.1).to(DEV), products="f16")], []


def _f16_conv_data(byte):
    ops, lib = _ops(), _lib.load()
    n, h, w, cin, csplit, cout = 2, 5, 7, 128, 64, 32
    _, wp, wr = _ring_weights(cin, cout)
    g = _plane2(planar_encode(_rand((n, cout, h, w), 79), GRAD_LO), byte)
    act = torch.relu(_rand((n, cin, h, w), 80))
    m1, m2 = planar_encode(act[:, :csplit]), planar_encode(act[:, csplit:])
    dx1, dx2 = _grad_out(n, csplit, h, w), _grad_out(n, cin - csplit, h, w)
    ws = torch.empty(lib.wsu_conv3x3_pl_bwd_data_workspace_bytes(n, h, w, cin, cout), dtype=torch.uint8, device=DEV)
    ops.check(lib.wsu_conv3x3_pl_bwd_data(g.data_ptr(), wp.data_ptr(), wr.data_ptr(), ws.data_ptr(), ws.numel(), dx1.data_ptr(), dx2.data_ptr(), csplit,
                                          m1.data_ptr(), m2.data_ptr(), None, None, n, h, w, cin, cout, 0, ops.products_id("f16"), _stream()), "wsu_conv3x3_pl_bwd_data")
    return [_live(dx1, "f16"), _live(dx2, "f16")], [dx1, dx2]


def _f16_conv_weight(byte):
    g = _plane2(planar_encode(_rand((2, 64, 5, 7), 81), GRAD_LO), byte)
    x1 = planar_encode(torch.relu(_rand((2, 64, 5, 7), 82)))
    return list(_ops().conv3x3_pl_bwd_weight(g, x1, None, products="f16")), []


def _f16_convt_data(byte):
    ops, lib = _ops(), _lib.load()
    n, h, w, cin, cout = 2, 5, 7, 64, 32
    wp = ops.pack_convt2x2_pl_dgrad(_rand((cin, cout, 2, 2), 83, 0.1).to(DEV))
    dy = _plane2(planar_encode(_rand((n, cout, 2 * h, 2 * w), 84), GRAD_LO), byte)
    mask = planar_encode(torch.relu(_rand((n, cin, h, w), 85)))
    dx = _grad_out(n, cin, h, w)
    ops.check(lib.wsu_convt2x2_pl_bwd_data(dy.data_ptr(), wp.data_ptr(), dx.data_ptr(), mask.data_ptr(), n, h, w, cin, cout, ops.products_id("f16"), _stream()), "wsu_convt2x2_pl_bwd_data")
    return [_live(dx, "f16")], [dx]


def _f16_convt_weight(byte):
    x = planar_encode(torch.relu(_rand((2, 64, 5, 7), 86)))
    dy = _plane2(planar_encode(_rand((2, 64, 10, 14), 87), GRAD_LO), byte)
    return list(_ops().convt2x2_pl_bwd_weight(x, dy, products="f16")), []


@pytest.mark.parametrize("kernel", [_f16_pool, _f16_head, _f16_colsum, _f16_first_weight, _f16_first_data, _f16_conv_data, _f16_conv_weight,
                                    _f16_convt_data, _f16_convt_weight], ids=lambda f: f.__name__[5:])
def test_products_f16_leaves_residual_planes_alone(kernel):
    """include/wsu.h, K7p: with WSU_PRODUCTS_F16 plane 2 of a gradient tensor is never touched.  Input side: the results are the same bits
    whether plane 2 of every input gradient holds zeros or e4m3 448 (0.027 per value where a kernel to read it; today's bands of 3e-4 allow
    the 2^-12 a real residual adds).  Output side: plane 2 of every planar output keeps the bytes it was given."""
    outs0, planar0 = kernel(0x00)
    outs1, planar1 = kernel(BIG_E4M3)
    torch.cuda.synchronize()
    assert len(outs0) == len(outs1) > 0
    for a, b in zip(outs0, outs1):
        assert float(a.float().abs().max()) > 0
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    for t in planar0 + planar1:
        assert bool((t.view(torch.uint8)[:, :, 2] == SENTINEL).all())
        assert not bool((t.view(torch.uint8)[:, :, :2] == SENTINEL).all())


# ---- 7. argument errors ---------------------------------------------------------------------------------------------------------------------------
def _refused(entry, call):
    """`call(p)` hands the entry the pointer p for every tensor: a zeroed-on-purpose 16 MB block, larger than anything the named shapes would
    touch.  The library's own error comes back, ops.check raises it with the entry's name, and nothing was launched: the block is unchanged."""
    ops = _ops()
    buf = torch.full((16 << 20,), 0x5A, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.WsuError, match=entry) as ei:
        ops.check(call(buf.data_ptr()), entry)
    torch.cuda.synchronize()
    assert entry[4:] in str(ei.value).split("):", 1)[1]       # the library's message names the entry too
    assert bool((buf == 0x5A).all())


BAD_PRODUCTS = 7


def _pool_args(h=4, w=4, c=16, products=0):
    return lambda p: _lib.load().wsu_maxpool2x2_pl_bwd(p, p, p, p, 1, h, w, c, products, _stream())


def _head_args(c=64, cout=1, products=0, short=0):
    def call(p):
        lib = _lib.load()
        nbytes = lib.wsu_head_pl_bwd_workspace_bytes(64 if short else c, 1 if short else cout)
        return lib.wsu_conv1x1_sigmoid_pl_bwd(p, p, p, p, p, p, p, p, nbytes - short, 1, 4, 4, c, cout, products, _stream())
    return call


def _colsum_args(c=64, products=0, short=0):
    def call(p):
        lib = _lib.load()
        return lib.wsu_colsum_pl(p, p, p, lib.wsu_chansum_pl_workspace_bytes(64 if short else c) - short, 1, 4, 4, c, products, _stream())
    return call


def _first_w_args(c=64, products=0, short=0):
    def call(p):
        lib = _lib.load()
        return lib.wsu_conv3x3_first_pl_bwd_weight(p, p, p, p, p, lib.wsu_chansum_pl_workspace_bytes(64 if short else c) - short, 1, 4, 4, c, products, _stream())
    return call


def _first_d_args(cin=1, c=64, products=0):
    return lambda p: _lib.load().wsu_conv3x3_first_pl_bwd_data(p, p, p, 1, 4, 4, cin, c, products, _stream())


def _ring_args(products=0, short=0):
    def call(p):
        lib = _lib.load()
        nbytes = lib.wsu_conv3x3_pl_bwd_data_workspace_bytes(1, 4, 4, 64, 32)
        return lib.wsu_conv3x3_pl_bwd_data(p, p, p, p, nbytes - short, p, None, 64, None, None, None, None, 1, 4, 4, 64, 32, 0, products, _stream())
    return call


REFUSED = [
    ("wsu_maxpool2x2_pl_bwd", "odd-h", _pool_args(h=3)), ("wsu_maxpool2x2_pl_bwd", "odd-w", _pool_args(w=5)),
    ("wsu_maxpool2x2_pl_bwd", "c=24", _pool_args(c=24)), ("wsu_maxpool2x2_pl_bwd", "c=8", _pool_args(c=8)),
    ("wsu_maxpool2x2_pl_bwd", "products", _pool_args(products=BAD_PRODUCTS)),
    ("wsu_conv1x1_sigmoid_pl_bwd", "cout=5", _head_args(cout=5)), ("wsu_conv1x1_sigmoid_pl_bwd", "cout=0", _head_args(cout=0)),
    ("wsu_conv1x1_sigmoid_pl_bwd", "c=48", _head_args(c=48)), ("wsu_conv1x1_sigmoid_pl_bwd", "c=256", _head_args(c=256)),
    ("wsu_conv1x1_sigmoid_pl_bwd", "products", _head_args(products=BAD_PRODUCTS)), ("wsu_conv1x1_sigmoid_pl_bwd", "workspace", _head_args(short=1)),
    ("wsu_colsum_pl", "c=48", _colsum_args(c=48)), ("wsu_colsum_pl", "c=4096", _colsum_args(c=4096)),
    ("wsu_colsum_pl", "products", _colsum_args(products=BAD_PRODUCTS)), ("wsu_colsum_pl", "workspace", _colsum_args(short=1)),
    ("wsu_conv3x3_first_pl_bwd_weight", "c=512", _first_w_args(c=512)), ("wsu_conv3x3_first_pl_bwd_weight", "products", _first_w_args(products=BAD_PRODUCTS)),
    ("wsu_conv3x3_first_pl_bwd_weight", "workspace", _first_w_args(short=1)),
    ("wsu_conv3x3_first_pl_bwd_data", "cin=9", _first_d_args(cin=9)), ("wsu_conv3x3_first_pl_bwd_data", "c=512", _first_d_args(c=512)),
    ("wsu_conv3x3_first_pl_bwd_data", "products", _first_d_args(products=BAD_PRODUCTS)),
    ("wsu_conv3x3_pl_bwd_data", "products", _ring_args(products=BAD_PRODUCTS)), ("wsu_conv3x3_pl_bwd_data", "workspace", _ring_args(short=1)),
]


@pytest.mark.parametrize("entry,call", [pytest.param(e, c, id=f"{e}-{i}") for e, i, c in REFUSED])
def test_refused_arguments(entry, call):
    """Every shape the entries of train_pl.hip refuse, a bad `products` id and a workspace one byte short (the reflect ring's entry included:
    its workspace is checked before its first launch): the library's argument error, never a launch."""
    _refused(entry, call)
