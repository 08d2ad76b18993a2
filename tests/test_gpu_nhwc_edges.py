"""The NHWC pointwise, pool, head and first-layer kernels (csrc/pointwise.hip and the non-matrix half of csrc/backward.hip) at their edges:
every channel count the entries accept, the smallest images (where every reflected tap coincides), partial last blocks and tiles, every
grid-stride loop past its cap, constructed pool windows, and every refused argument.

References are the fp64 restatements of tests/nhwc_np.py.  Every arithmetic kernel gets two kinds of input:
  exact   small dyadic operands (multiples of 2^-3): every fp32 product and partial sum is exact in any order, so the kernel must equal the
          fp64 reference BIT FOR BIT after one conversion to fp32 -- in bf16 storage after one rounding to bf16, to nearest with ties to
          even: wsu_pack_bf16x2 casts with (__bf16), which is v_cvt_pk_bf16_f32, and torch's .bfloat16() rounds the same way.  (-0 == +0.)
          The test asserts on the reference alone that the inputs keep that promise (nhwc_np.exact_budget).
  random  normal operands against the derived bound (K + 4) 2^-24 S of nhwc_np.dot_bound, S the operation on absolute values, per output
          element; bf16 storage adds half a bf16 ulp of |ref|.  Each test prints its largest err / bound (`pytest -s`); the figures
          measured on the MI355X stand in the docstrings."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nhwc_np as R
from gpu_util import DEV
from ws_unet_amd import _lib

pytestmark = pytest.mark.gpu

F32, BF16X3, BF16 = 0, 1, 2
MODE_IDS = {F32: "f32", BF16X3: "bf16x3", BF16: "bf16"}


def _ops():
    from ws_unet_amd import ops
    return ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync_cpu(t):
    torch.cuda.synchronize()
    return t.float().cpu() if t.dtype == torch.bfloat16 else t.cpu()


def _report(group, worst):
    print(f"{group}: largest err / bound = {worst:.3g}")
    assert worst <= 1.0, (group, worst)


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


def _as_bf16(x):
    """fp32 numbers that bf16 holds exactly -> bf16 by their bits (torch's own conversion replaces a NaN by one of its choosing)"""
    assert bool(((x.view(torch.int32) & 0xFFFF) == 0).all())
    return (x.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)


# ---- 1. first layer, forward ----------------------------------------------------------------------------------------------------------------------
FIRST_IMAGES = [(2, 2, 2), (2, 2, 3), (1, 3, 2), (2, 3, 3), (1, 5, 7), (3, 20, 36)]


@pytest.mark.parametrize("mode", [F32, BF16X3, BF16], ids=MODE_IDS.get)
@pytest.mark.parametrize("cout", [8, 16, 32, 64, 128, 256])
def test_conv3x3_first_fwd_edges(cout, mode):
    """cin 1..8 at every cout = 8 * 2^k up to 256 (1 .. 32 lanes per pixel; cin 8 x cout 256 holds 73 728 B of weights in LDS) in the three
    modes the entry takes (mode 1 stores fp32 like mode 0), on 2x2 .. 5x7 images and on (3, 20, 36), whose 2160 pixels are no multiple of
    any block's 8 * 256 / (cout / 8), with relu and bias each on and off.  Exact inputs: bitwise.  Random: K = 9 cin + 1 -- measured
    err / bound 0.25 at most with fp32 storage (cin = 1: ten roundings against the fourteen allowed) and 0.995 with bf16 storage, which is the
    rounding itself and not the sum: a value just above a power of two lies up to half a bf16 ulp = 2^-8 |v| from its bf16 number, the
    whole allowance."""
    ops, worst = _ops(), 0.0
    for cin in range(1, 9):
        for i, (n, h, w) in enumerate(FIRST_IMAGES):
            relu, has_b = bool((cin + i) & 1), bool((cin + i) & 2)
            assert (n * h * w) % (8 * 256 // (cout // 8)) != 0 or i < 5
            for exact in (True, False):
                seed = 1000 * cin + 10 * i
                if exact:
                    x, wt, b = R.dyadic((n, cin, h, w), seed), R.dyadic((cout, cin, 3, 3), seed + 1), R.dyadic((cout,), seed + 2)
                else:
                    x, wt, b = R.rand((n, cin, h, w), seed), R.rand((cout, cin, 3, 3), seed + 1, (2.0 / (9 * cin)) ** 0.5), R.rand((cout,), seed + 2, 0.3)
                b = b if has_b else None
                ref, s = R.conv_first(x, wt, b, relu)
                got = _sync_cpu(ops.conv3x3_first(_dev(x), _dev(wt), _dev(b), mode, relu=relu))
                assert tuple(got.shape) == (n, h, w, cout)
                what = (cin, (n, h, w), relu, has_b, exact)
                if exact:
                    R.exact_budget(ref, s, 2.0 ** -6)
                    want = ref.float().bfloat16().float() if mode == BF16 else ref.float()
                    assert torch.equal(got, want), what
                else:
                    e = R.dot_bound(9 * cin + 1, s)
                    r = R.ratio(got, ref, R.bf16_bound(e, ref) if mode == BF16 else e)
                    assert r <= 1.0, (what, r)
                    worst = max(worst, r)
    _report(f"conv3x3_first cout={cout} {MODE_IDS[mode]}", worst)


# ---- 2. first layer, weight gradient --------------------------------------------------------------------------------------------------------------
# pixel counts 4, 255, 256, 2048, 2049 and 3 * 2048 + 17: one tile short of, at and past the 256-pixel tile and the 2048-pixel chunk.  257 is a
# prime: no image with h, w >= 2 has it, so 258 and 259 stand in for "one tile and a little"
WGRAD_IMAGES = [(1, 2, 2), (1, 15, 17), (1, 16, 16), (1, 6, 43), (1, 7, 37), (2, 32, 32), (1, 3, 683), (1, 61, 101)]


@pytest.mark.parametrize("cout", [64, 128, 192])
def test_conv3x3_first_bwd_weight_edges(cout):
    """cin 1..8, one to three 64-channel block columns, one to four chunks with a partial last tile; with and without db (the C entry's
    db == NULL), and a repeat call that gives the same bits.  Exact inputs: bitwise.  Random: K = N H W -- measured err / bound 0.35 at most (at four pixels; 0.02 from 2048 pixels on)."""
    ops, worst = _ops(), 0.0
    assert [n * h * w for n, h, w in WGRAD_IMAGES] == [4, 255, 256, 258, 259, 2048, 2049, 3 * 2048 + 17]
    for cin in range(1, 9):
        for i, (n, h, w) in enumerate(WGRAD_IMAGES):
            for exact in (True, False):
                seed = 2000 * cin + 10 * i
                mk = R.dyadic if exact else R.rand
                g, x = mk((n, h, w, cout), seed), mk((n, cin, h, w), seed + 1)
                dw_ref, sw, db_ref, sb = R.conv_first_wgrad(g, x)
                gd, xd = _dev(g), _dev(x)
                dw, db = ops.conv3x3_first_bwd_weight(gd, xd)
                dw2, none = ops.conv3x3_first_bwd_weight(gd, xd, want_bias=False)
                dw3, db3 = ops.conv3x3_first_bwd_weight(gd, xd)
                torch.cuda.synchronize()
                what = (cin, (n, h, w), exact)
                assert none is None and torch.equal(dw, dw2) and torch.equal(dw, dw3) and torch.equal(db, db3), what
                assert tuple(dw.shape) == (cout, cin, 3, 3) and tuple(db.shape) == (cout,)
                if exact:
                    R.exact_budget(dw_ref, sw, 2.0 ** -6)
                    R.exact_budget(db_ref, sb, 2.0 ** -3)
                    assert torch.equal(dw.cpu(), dw_ref.float()) and torch.equal(db.cpu(), db_ref.float()), what
                else:
                    k = n * h * w
                    r = max(R.ratio(dw, dw_ref, R.dot_bound(k, sw)), R.ratio(db, db_ref, R.dot_bound(k, sb)))
                    assert r <= 1.0, (what, r)
                    worst = max(worst, r)
    _report(f"conv3x3_first_bwd_weight cout={cout}", worst)


def test_conv3x3_first_bwd_weight_uneven_chunks():
    """1 x 1449 x 1448 = 2 098 152 pixels, just above 1024 * 2048: the chunks are 2049 pixels long, no multiple of the 256-pixel tile, so every
    chunk ends in a tile of one pixel.  Inputs and the fp64 reference live on the device.  Operands from {-1/8, 0, 1/8} keep the sum of
    |terms| below 2^24 quanta of 2^-6 even here: bitwise.  Random operands: K = N H W (the bound is wide at this K) -- measured err / bound
    3.6e-8."""
    ops = _ops()
    n, cin, h, w, cout = 1, 1, 1449, 1448, 64
    assert n * h * w > 1024 * 2048 and -(-n * h * w // 1024) % 256 != 0
    g = torch.randint(-1, 2, (n, h, w, cout), generator=torch.Generator(device=DEV).manual_seed(21), device=DEV).float() / 8.0
    x = torch.randint(-1, 2, (n, cin, h, w), generator=torch.Generator(device=DEV).manual_seed(22), device=DEV).float() / 8.0
    dw_ref, sw, db_ref, sb = R.conv_first_wgrad(g, x)
    R.exact_budget(dw_ref.cpu(), sw.cpu(), 2.0 ** -6)
    R.exact_budget(db_ref.cpu(), sb.cpu(), 2.0 ** -3)
    dw, db = ops.conv3x3_first_bwd_weight(g, x)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw_ref.float()) and torch.equal(db, db_ref.float())
    assert float(dw.abs().max()) > 0
    del g, x, dw_ref, sw
    g, x = R.rand((n, h, w, cout), 23, device=DEV), R.rand((n, cin, h, w), 24, device=DEV)
    dw_ref, sw, db_ref, sb = R.conv_first_wgrad(g, x)
    dw, db = ops.conv3x3_first_bwd_weight(g, x)
    torch.cuda.synchronize()
    k = n * h * w
    _report("conv3x3_first_bwd_weight 1449x1448", max(R.ratio(dw, dw_ref, R.dot_bound(k, sw)), R.ratio(db, db_ref, R.dot_bound(k, sb))))
    del g, x, dw_ref, sw
    torch.cuda.empty_cache()


# ---- 3. first layer, data gradient ----------------------------------------------------------------------------------------------------------------
DGRAD_IMAGES = [(2, 2, 2), (2, 2, 3), (1, 3, 2), (2, 3, 3), (1, 4, 4), (1, 2, 40), (1, 40, 2), (1, 5, 7)]


def _nonzero(g):
    return torch.where(g == 0, torch.full_like(g, 0.125), g)


@pytest.mark.parametrize("cout", [4, 8, 64, 128, 256, 512])
def test_conv3x3_first_bwd_data_edges(cout):
    """fp64 autograd of conv2d(pad(x, reflect), w) with a gradient that is non-zero everywhere, cin 1..8, on the images where rows 1 and h - 2
    (columns 1 and w - 2) coincide, touch or lie apart.  cin 8 x cout 256 holds 73 728 B and cin 8 x cout 512 147 456 B of weights in LDS:
    they run since the entry raises the kernel's dynamic-LDS limit.  Exact inputs (|w| <= 1): bitwise.  Random: K = 36 cout, the four padded
    positions that can fold onto one pixel -- measured err / bound 0.012 at most (cout 4; 6e-5 at cout 512)."""
    ops, worst = _ops(), 0.0
    for cin in range(1, 9):
        for i, (n, h, w) in enumerate(DGRAD_IMAGES):
            for exact in (True, False):
                seed = 3000 * cin + 10 * i
                if exact:
                    g, wt = _nonzero(R.dyadic((n, h, w, cout), seed)), R.dyadic((cout, cin, 3, 3), seed + 1, 1.0)
                else:
                    g, wt = R.rand((n, h, w, cout), seed), R.rand((cout, cin, 3, 3), seed + 1, (2.0 / (9 * cout)) ** 0.5)
                assert bool((g != 0).all())
                ref, s = R.conv_first_dgrad(g, wt)
                got = _sync_cpu(ops.conv3x3_first_bwd_data(_dev(g), _dev(wt)))
                what = (cin, (n, h, w), exact)
                assert tuple(got.shape) == (n, cin, h, w)
                if exact:
                    R.exact_budget(ref, s, 2.0 ** -6)
                    assert torch.equal(got, ref.float()), what
                else:
                    r = R.ratio(got, ref, R.dot_bound(36 * cout, s))
                    assert r <= 1.0, (what, r)
                    worst = max(worst, r)
    _report(f"conv3x3_first_bwd_data cout={cout}", worst)


def test_conv3x3_first_bwd_data_grid_stride():
    """(1, 1, 1500, 1500) at cout 4: 2 250 000 outputs for a grid capped at 8192 x 256 = 2 097 152 threads, so the last 152 848 -- the last 101
    rows -- come from the second pass of the grid-stride loop.  Exact inputs: bitwise, the last rows on their own too, and non-zero there.
    Random: measured err / bound 0.018."""
    ops = _ops()
    n, cin, h, w, cout = 1, 1, 1500, 1500, 4
    assert n * cin * h * w > 8192 * 256
    first_second_pass = 8192 * 256 // w + 1
    g, wt = _nonzero(R.dyadic((n, h, w, cout), 31, device=DEV)), R.dyadic((cout, cin, 3, 3), 32, 1.0).to(DEV)
    ref, s = R.conv_first_dgrad(g, wt)
    R.exact_budget(ref.cpu(), s.cpu(), 2.0 ** -6)
    got = ops.conv3x3_first_bwd_data(g, wt)
    torch.cuda.synchronize()
    tail = (slice(None), slice(None), slice(first_second_pass, None))
    assert float(got[tail].abs().max()) > 0 and float((got[tail] != 0).float().mean()) > 0.9 and float(got[0, 0, -1, -1]) != 0
    assert torch.equal(got[tail], ref[tail].float())
    assert torch.equal(got, ref.float())
    g, wt = R.rand((n, h, w, cout), 33, device=DEV), R.rand((cout, cin, 3, 3), 34, 0.3).to(DEV)
    ref, s = R.conv_first_dgrad(g, wt)
    got = ops.conv3x3_first_bwd_data(g, wt)
    torch.cuda.synchronize()
    assert float(got[0, 0, -1, -1]) != 0
    bound = R.dot_bound(36 * cout, s)
    _report("conv3x3_first_bwd_data 1500x1500", max(R.ratio(got, ref, bound), R.ratio(got[tail], ref[tail], bound[tail])))


# ---- 4. head, forward -----------------------------------------------------------------------------------------------------------------------------
HEAD_PIXELS = [(1, 1, 1), (1, 1, 3), (2, 5, 7)]              # 70 pixels x (1 .. 64 lanes) never fill the last 256-thread block
SIGMOID_ATOL = 5e-6                                          # tests/test_gpu_forward.py: the head's sigmoid against the oracle's


@pytest.mark.parametrize("mode,c", [(F32, c) for c in (4, 8, 16, 32, 64, 128, 256)] + [(BF16, c) for c in (8, 16, 32, 64, 128, 256, 512)],
                         ids=lambda v: MODE_IDS.get(v, str(v)) if isinstance(v, int) and v < 3 else str(v))
def test_conv1x1_sigmoid_fwd_edges(mode, c):
    """Lane groups of 1 .. 64 per pixel (c = 4 in fp32 has no shuffle at all, c = 256 / 512 uses the whole wave), cout 1..4, one and three
    pixels and a partly empty last block, with and without bias.  Logit: exact inputs bitwise; random inputs K = c + 1 -- measured
    err / bound 0.24 at most (c = 4; 0.002 at c = 256).  Output: |out - sigmoid(fp64 logit)| <= 5e-6 + bound / 4 (the sigmoid's slope is
    at most 1/4) -- measured 1.1e-7 at most."""
    ops, worst, worst_out = _ops(), 0.0, 0.0
    for cout in range(1, 5):
        for i, (n, h, w) in enumerate(HEAD_PIXELS):
            assert (n * h * w * (c // (8 if mode == BF16 else 4))) % 256 != 0
            for exact in (True, False):
                seed = 4000 + 100 * cout + 10 * i
                if exact:
                    x, wt, b = R.dyadic((n, h, w, c), seed), R.dyadic((cout, c), seed + 1), R.dyadic((cout,), seed + 2)
                else:
                    x, wt, b = R.rand((n, h, w, c), seed), R.rand((cout, c), seed + 1, c ** -0.5), R.rand((cout,), seed + 2, 0.3)
                if mode == BF16:
                    x = x.bfloat16()                          # the stored activations are the operands (the dyadic ones are bf16 numbers)
                b = b if (cout + i) & 1 else None
                z_ref, s = R.head_fwd(x.float(), wt, b)
                out, z = ops.conv1x1_sigmoid(_dev(x), _dev(wt), _dev(b), mode, want_logit=True)
                only_out = ops.conv1x1_sigmoid(_dev(x), _dev(wt), _dev(b), mode)
                out, z = _sync_cpu(out), _sync_cpu(z)
                what = (cout, (n, h, w), exact, b is not None)
                assert tuple(out.shape) == (n, cout, h, w) and torch.equal(only_out.cpu(), out), what
                e = R.dot_bound(c + 1, s)
                if exact:
                    R.exact_budget(z_ref, s, 2.0 ** -6)
                    assert torch.equal(z, z_ref.float()), what
                else:
                    r = R.ratio(z, z_ref, e)
                    assert r <= 1.0, (what, r)
                    worst = max(worst, r)
                err = (out.double() - torch.sigmoid(z_ref)).abs()
                assert bool((err <= SIGMOID_ATOL + e / 4).all()), (what, float(err.max()))
                worst_out = max(worst_out, float(err.max()))
    print(f"conv1x1_sigmoid c={c} {MODE_IDS[mode]}: largest output error {worst_out:.2e}")
    _report(f"conv1x1_sigmoid c={c} {MODE_IDS[mode]} logit", worst)


@pytest.mark.parametrize("mode", [F32, BF16], ids=MODE_IDS.get)
def test_conv1x1_sigmoid_fwd_saturated_logits(mode):
    """Logits of +-30, +-100, +-200 (exp overflows fp32 past 88.7) among ordinary ones: the output stays finite, inside [0, 1] and monotone in
    the logit, 0 and 1 at +-200."""
    ops = _ops()
    zs = torch.tensor([-200.0, -100.0, -30.0, -8.0, -1.0, 0.0, 1.0, 8.0, 30.0, 100.0, 200.0])
    c = 64
    x = torch.zeros((1, 1, len(zs), c))
    x[0, 0, :, 5] = zs / 4.0                                  # bf16 numbers: -50 .. 50
    wt = torch.zeros((2, c))
    wt[0, 5], wt[1, 5] = 4.0, -4.0                            # plane 1 runs the logits backwards
    xd = _dev(x.bfloat16() if mode == BF16 else x)
    out, z = ops.conv1x1_sigmoid(xd, _dev(wt), None, mode, want_logit=True)
    out, z = _sync_cpu(out), _sync_cpu(z)
    assert torch.equal(z[0, 0, 0], zs) and torch.equal(z[0, 1, 0], -zs)
    for o in (out[0, 0, 0], out[0, 1, 0].flip(0)):
        assert bool(torch.isfinite(o).all()) and float(o.min()) >= 0.0 and float(o.max()) <= 1.0
        assert bool((o[1:] >= o[:-1]).all()) and bool((o[3:9][1:] > o[3:9][:-1]).all())
        assert float(o[0]) == 0.0 and float(o[-1]) == 1.0 and float(o[5]) == 0.5              # sigmoid(-200) = 1e-87 is 0 in fp32
        assert float((o.double() - torch.sigmoid(zs.double())).abs().max()) <= SIGMOID_ATOL


# ---- 5. head, backward ----------------------------------------------------------------------------------------------------------------------------
def _head_bwd_case(c, cout, n, h, w, relu_mask, exact, seed):
    if exact:
        x, wt = R.dyadic((n, h, w, c), seed, 2.0), R.dyadic((cout, c), seed + 1)
        out = torch.tensor([0.25, 0.5, 0.75])[torch.randint(0, 3, (n, cout, h, w), generator=torch.Generator().manual_seed(seed + 2))]
        dout = R.dyadic((n, cout, h, w), seed + 3, 1.0)       # out (1 - out) is 3/16 or 1/4: dz is a multiple of 2^-7, |dz| <= 1/4
    else:
        x, wt = R.rand((n, h, w, c), seed), R.rand((cout, c), seed + 1, c ** -0.5)
        out, dout = torch.sigmoid(R.rand((n, cout, h, w), seed + 2, 2.0)), R.rand((n, cout, h, w), seed + 3)
    if relu_mask:
        x = torch.relu(x)                                     # the saved post-ReLU input: about half of it is zero
        x.view(-1)[0] = 0.0
    return x, wt, out, dout


def _head_bwd_check(c, cout, n, h, w, relu_mask, exact, seed):
    ops = _ops()
    x, wt, out, dout = _head_bwd_case(c, cout, n, h, w, relu_mask, exact, seed)
    refs = R.head_bwd(x, wt, out, dout, relu_mask)
    args = (_dev(x), _dev(wt), _dev(out), _dev(dout))
    first = ops.conv1x1_sigmoid_bwd(*args, relu_mask=relu_mask)
    again = ops.conv1x1_sigmoid_bwd(*args, relu_mask=relu_mask)
    torch.cuda.synchronize()
    what = (c, cout, (n, h, w), relu_mask, exact)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), what
    got = {"gx": first[0].cpu(), "dw": first[1].cpu().reshape(cout, c), "db": first[2].cpu()}
    assert tuple(first[1].shape) == (cout, c, 1, 1)
    worst = 0.0
    for name, k, quantum in (("gx", cout, 2.0 ** -10), ("dw", n * h * w, 2.0 ** -10), ("db", n * h * w, 2.0 ** -7)):
        ref, s = refs[name]
        if exact:
            R.exact_budget(ref, s, quantum)
            assert torch.equal(got[name], ref.float()), (what, name)
        else:
            r = R.ratio(got[name], ref, R.dot_bound(k, s))
            assert r <= 1.0, (what, name, r)
            worst = max(worst, r)
    if relu_mask:
        assert float(got["gx"][x <= 0].abs().max() if bool((x <= 0).any()) else 0.0) == 0.0
    return worst


@pytest.mark.parametrize("c", [4, 8, 16, 32, 64, 128, 256])
def test_conv1x1_sigmoid_bwd_edges(c):
    """256 .. 4 pixels per block pass, cout 1..4, one pixel, one pixel short of a block's 256 / (c / 4) multiple and two past it (255, 257),
    the ReLU mask on and off over an input with zeros, every call repeated for equal bits.  Exact inputs (out from {1/4, 1/2, 3/4}): gx,
    dw and db bitwise.  Random: K = cout for gx, N H W for dw and db -- measured err / bound 0.64 at most: gx at cout = 1, one product of w with a dz that took three
    roundings itself (1 - out and two products), four of the five roundings that K + 4 allows."""
    worst = 0.0
    for cout in range(1, 5):
        for i, (n, h, w) in enumerate([(1, 1, 1), (1, 15, 17), (1, 1, 257)]):
            for relu_mask in (True, False):
                for exact in (True, False):
                    worst = max(worst, _head_bwd_check(c, cout, n, h, w, relu_mask, exact, 5000 + 100 * cout + 10 * i + relu_mask))
    _report(f"conv1x1_sigmoid_bwd c={c}", worst)


@pytest.mark.parametrize("c,npix", [(256, 4099), (64, 16400)])
def test_conv1x1_sigmoid_bwd_stride_loop(c, npix):
    """More pixels than 1024 blocks x 256 / (c / 4) cover in one pass: the first blocks walk two pixels each, the partial rows hold two
    pixels' sums.  Exact inputs bitwise, random inputs within the bound -- measured err / bound 0.67 at most (gx at cout = 1, as above)."""
    assert npix > 1024 * 256 // (c // 4)
    worst = 0.0
    for cout, relu_mask in ((1, True), (4, False), (3, True)):
        for exact in (True, False):
            worst = max(worst, _head_bwd_check(c, cout, 1, 1, npix, relu_mask, exact, 5900 + cout))
    _report(f"conv1x1_sigmoid_bwd c={c} {npix} pixels", worst)


# ---- 6. max-pool ----------------------------------------------------------------------------------------------------------------------------------
POOL_IMAGES = [(2, 2, 2), (2, 2, 3), (1, 3, 2), (2, 3, 3), (1, 5, 7), (1, 24, 40)]
_NAN, _INF = float("nan"), float("inf")
POOL_PATTERNS = [[1.0] * 4,                                              # all equal: the first wins
                 [0.0, -0.0, -0.0, 0.0], [-0.0, 0.0, 0.0, -0.0], [-0.0] * 4,          # +0 == -0: the first wins and its bits are stored
                 [_INF, 1.0, -_INF, _INF], [-_INF] * 4, [-_INF, 2.0, _INF, 0.0], [-3.0, -_INF, -2.0, -2.0],
                 [_NAN, 1.0, 2.0, 3.0], [3.0, _NAN, 2.0, 1.0], [1.0, 2.0, _NAN, 3.0], [1.0, 3.0, 2.0, _NAN], [_INF, _NAN, _INF, _INF],
                 [0.5, 2.0, 2.0, 1.0], [0.5, 1.0, 2.0, 2.0], [2.0, 1.0, 0.5, 2.0], [-1.0, -1.0, -4.0, -1.0]]


def _pool_input(n, h, w, c, seed, bf16):
    """random activations with a constructed window at every third (window, channel) -- at all of them where there are few"""
    x = R.rand((n, h, w, c), seed)
    if bf16:
        x = x.bfloat16().float()
    hp, wp = h // 2, w // 2
    win = torch.from_numpy(R.pool_windows(x.numpy()).copy()).reshape(-1, 4)
    pat = torch.tensor(POOL_PATTERNS, dtype=torch.float32)
    step = 3 if win.shape[0] >= 3 * len(pat) else 1
    at = torch.arange(seed % step, win.shape[0], step)
    win[at] = pat[(torch.arange(len(at)) + seed) % len(pat)]
    win = win.reshape(n, hp, wp, c, 4)
    for k, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        x[:, a:2 * hp:2, b:2 * wp:2] = win[..., k]
    return x.contiguous()


@pytest.mark.parametrize("mode,c", [(F32, c) for c in (4, 8, 12, 24, 64)] + [(BF16, c) for c in (8, 24, 64)],
                         ids=lambda v: MODE_IDS.get(v, str(v)) if isinstance(v, int) and v < 3 else str(v))
def test_maxpool2x2_fwd_edges(mode, c):
    """Values and argmax bitwise those of oracle/np_ops.maxpool2x2 on the even crop (a last odd row / column belongs to no window), on 2x2 ..
    24x40 images whose windows include ties, +0 against -0 (np.max may return either zero: the stored bits must be those of the FIRST, the
    element np.argmax names), +-inf and one NaN in each of the four positions (include/wsu.h: the NaN is the result)."""
    ops = _ops()
    bf16 = mode == BF16
    for i, (n, h, w) in enumerate(POOL_IMAGES):
        x = _pool_input(n, h, w, c, 60 + i, bf16)
        xd = _dev(_as_bf16(x) if bf16 else x)
        y, idx = ops.maxpool2x2(xd, mode, want_idx=True)
        y_only = ops.maxpool2x2(xd, mode)
        torch.cuda.synchronize()
        v_ref, a_ref = R.pool_fwd(x.numpy())
        picked = np.take_along_axis(R.pool_windows(x.numpy()), a_ref[..., None].astype(np.int64), axis=-1)[..., 0]
        got = y.float().cpu().numpy()
        assert got.shape == (n, h // 2, w // 2, c) and y.dtype == xd.dtype
        np.testing.assert_array_equal(idx.cpu().numpy(), a_ref, err_msg=str((n, h, w)))
        np.testing.assert_array_equal(got, v_ref, err_msg=str((n, h, w)))                      # NaN == NaN, +0 == -0 here ...
        np.testing.assert_array_equal(got.view(np.uint32), picked.view(np.uint32), err_msg=str((n, h, w)))     # ... and the bits here
        assert torch.equal(y_only.float().cpu().view(torch.int32), y.float().cpu().view(torch.int32))
        if (h, w) == (24, 40):
            assert np.isnan(got).any() and np.isinf(got).any() and (got == 0).any()


@pytest.mark.parametrize("mode", [F32, BF16], ids=MODE_IDS.get)
def test_maxpool2x2_fwd_two_nans(mode):
    """include/wsu.h: a NaN in the window is the result, with the bits and the index of the window's LAST NaN."""
    ops = _ops()
    c = 8
    x = torch.ones((1, 2, 2, c))
    nan_a, nan_b = torch.tensor([0x7FC10000, 0x7FC20000], dtype=torch.int32).view(torch.float32)     # two payloads that survive bf16
    x[0, 0, 0, :], x[0, 1, 0, :] = nan_a, nan_b
    x[0, 0, 1, 3], x[0, 1, 1, 3] = nan_a, _INF
    xd = _dev(_as_bf16(x) if mode == BF16 else x)
    y, idx = ops.maxpool2x2(xd, mode, want_idx=True)
    torch.cuda.synchronize()
    bits = y.float().cpu().view(torch.int32).reshape(-1)
    assert bits.tolist() == [0x7FC20000] * c and idx.cpu().reshape(-1).tolist() == [2] * c


@pytest.mark.parametrize("c", [4, 8, 12, 24, 64])
def test_maxpool2x2_bwd_edges(c):
    """Exact routing to the recorded position where the pooled activation is positive.  accumulate = 1 (through ops, odd sizes included): the
    bits of skip + routed in fp32, the dropped last row / column keeps the skip gradient.  accumulate = 0 (the C entry itself, on a buffer
    filled with NaN): the routed gradient alone, zeros in the dropped row / column.  The mask is zero over one whole window, on scattered
    elements, and absent."""
    ops, lib = _ops(), _lib.load()
    for i, (n, h, w) in enumerate(POOL_IMAGES):
        hp, wp = h // 2, w // 2
        gen = torch.Generator().manual_seed(70 + i)
        idx = torch.randint(0, 4, (n, hp, wp, c), generator=gen, dtype=torch.uint8)
        dyp, skip = R.rand((n, hp, wp, c), 71 + i), R.rand((n, h, w, c), 72 + i)
        mask = torch.relu(R.rand((n, hp, wp, c), 73 + i))
        mask[:, 0, 0, :] = 0.0
        mask[0, -1, -1, 0] = -0.0
        for mk in (mask, None):
            routed = R.pool_bwd_routed(dyp, idx, mk, h, w)
            dd, di, dm = _dev(dyp), _dev(idx), _dev(mk)
            got = ops.maxpool2x2_bwd(_dev(skip), dd, di, dm)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(got.cpu().numpy(), (skip + routed).numpy(), err_msg=str((n, h, w, mk is None)))
            assert torch.equal(got.cpu()[:, 2 * hp:], skip[:, 2 * hp:]) and torch.equal(got.cpu()[:, :, 2 * wp:], skip[:, :, 2 * wp:])
            g0 = torch.full((n, h, w, c), _NAN, device=DEV)
            ops.check(lib.wsu_maxpool2x2_bwd(g0.data_ptr(), dd.data_ptr(), di.data_ptr(), None if dm is None else dm.data_ptr(), n, h, w, c, 0, _stream()),
                      "wsu_maxpool2x2_bwd")
            torch.cuda.synchronize()
            np.testing.assert_array_equal(g0.cpu().numpy(), routed.numpy(), err_msg=str((n, h, w, mk is None)))
            assert float(g0[:, 2 * hp:].abs().sum()) == 0.0 and float(g0[:, :, 2 * wp:].abs().sum()) == 0.0
            if mk is not None:
                assert float(g0[:, 0:2, 0:2].abs().sum()) == 0.0                              # the window whose mask is zero throughout
            assert float(g0.abs().max()) > 0 or hp * wp == 1


@pytest.fixture(scope="module")
def pool_large():
    """Forward: (1, 2050, 2050, 64) = 1025 x 1025 x 16 = 16 810 000 threads' worth of work for a grid capped at 65 536 x 256 = 16 777 216 (1.08 GB).
    Backward: (1, 1451, 1448, 64) = 33 616 768 for a cap of 131 072 x 256 = 33 554 432 (0.54 GB), with an odd height.  References: torch's
    max_pool2d and its autograd on the device."""
    gen = torch.Generator(device=DEV).manual_seed(81)
    xf = torch.randn((1, 2050, 2050, 64), generator=gen, device=DEV)
    assert 1025 * 1025 * 16 > 65536 * 256
    vf, indf = F.max_pool2d(xf.permute(0, 3, 1, 2), 2, return_indices=True)
    kf = (((indf // 2050) & 1) * 2 + (indf & 1)).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    vf = vf.permute(0, 2, 3, 1).contiguous()
    del indf
    h, w = 1451, 1448
    assert h * w * 16 > 131072 * 256
    xb = torch.randn((1, h, w, 64), generator=gen, device=DEV)
    a = xb.permute(0, 3, 1, 2).requires_grad_(True)
    pooled, indb = F.max_pool2d(a, 2, return_indices=True)
    kb = (((indb // w) & 1) * 2 + (indb & 1)).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    dyp = torch.randn((1, h // 2, w // 2, 64), generator=gen, device=DEV)
    mask = pooled.detach().permute(0, 2, 3, 1).contiguous()
    routed = {}
    for masked in (False, True):
        d = dyp * (mask > 0) if masked else dyp
        routed[masked] = torch.autograd.grad(pooled, a, d.permute(0, 3, 1, 2), retain_graph=True)[0].permute(0, 2, 3, 1).contiguous()
    del pooled, a, indb
    skip = torch.randn((1, h, w, 64), generator=gen, device=DEV)
    yield {"xf": xf, "vf": vf, "kf": kf, "kb": kb, "dyp": dyp, "mask": mask, "routed": routed, "skip": skip}
    torch.cuda.empty_cache()


def test_maxpool2x2_fwd_grid_stride(pool_large):
    """The last 32 784 (window, channel group) items -- the last two window rows -- come from the second pass of the loop: values and
    argmax equal torch's on the whole tensor and on those rows alone."""
    ops, p = _ops(), pool_large
    y, idx = ops.maxpool2x2(p["xf"], F32, want_idx=True)
    torch.cuda.synchronize()
    assert torch.equal(y[0, -2:], p["vf"][0, -2:]) and torch.equal(idx[0, -2:], p["kf"][0, -2:]) and float(y[0, -2:].abs().max()) > 0
    assert torch.equal(y, p["vf"]) and torch.equal(idx, p["kf"])
    del y, idx


@pytest.mark.parametrize("masked", [False, True])
def test_maxpool2x2_bwd_grid_stride(pool_large, masked):
    """accumulate = 1 through ops and accumulate = 0 through the C entry on the odd-height tensor: the bits of skip + routed / of routed, torch's
    own routing; the last three rows (the second pass takes the last 62 336 items: the end of row 1448, row 1449 and the dropped row 1450) on their own too."""
    ops, lib, p = _ops(), _lib.load(), pool_large
    h, w, mk = 1451, 1448, (p["mask"] if masked else None)
    routed = p["routed"][masked]
    assert float(routed[0, -1].abs().max()) == 0.0 and float(routed[0, -2].abs().max()) > 0
    got = ops.maxpool2x2_bwd(p["skip"].clone(), p["dyp"], p["kb"], mk)
    torch.cuda.synchronize()
    want = p["skip"] + routed
    assert torch.equal(got[0, -3:], want[0, -3:]) and torch.equal(got[0, -1], p["skip"][0, -1])
    assert torch.equal(got, want)
    del got, want
    g0 = torch.full((1, h, w, 64), _NAN, device=DEV)
    ops.check(lib.wsu_maxpool2x2_bwd(g0.data_ptr(), p["dyp"].data_ptr(), p["kb"].data_ptr(), None if mk is None else mk.data_ptr(),
                                     1, h, w, 64, 0, _stream()), "wsu_maxpool2x2_bwd")
    torch.cuda.synchronize()
    assert torch.equal(g0[0, -3:], routed[0, -3:]) and torch.equal(g0, routed)
    del g0


# ---- 7. UniformDropout ----------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("c,channel", [(1, 0), (3, 0), (3, 2)])
def test_uniform_dropout_edges(c, channel):
    """Bitwise the float32 restatement in the kernel's row-major order (the file is compiled without contraction and the KB products are exact),
    n 1..3, on 2x2 and 2x3 (both reflections of a row land on the same pixel), 3x3 and 5x7; a given mask (with fractional values) and a drawn
    one, which equals the restated hash and comes back in mask_out; every other plane is copied."""
    ops = _ops()
    for n in (1, 2, 3):
        for i, (h, w) in enumerate([(2, 2), (2, 3), (3, 3), (5, 7)]):
            x = torch.rand((n, c, h, w), generator=torch.Generator().manual_seed(90 + 10 * n + i))
            mask = (torch.rand((n, 1, h, w), generator=torch.Generator().manual_seed(91 + i)) < 0.5).float()
            mask[0, 0, 0, 0], mask[-1, 0, -1, -1] = 0.3, 0.75
            y, mo = ops.uniform_dropout(_dev(x), _dev(mask), channel=channel, want_mask=True)
            torch.cuda.synchronize()
            assert torch.equal(_bits(mo.cpu()), _bits(mask)) and torch.equal(_bits(y.cpu()), _bits(R.dropout(x, mask, channel))), (n, h, w, "given")
            seed = 1234567 + 97 * i + n
            y, mo = ops.uniform_dropout(_dev(x), None, channel=channel, keep_prob=0.5, seed=seed, want_mask=True)
            y2 = ops.uniform_dropout(_dev(x), None, channel=channel, keep_prob=0.5, seed=seed)
            torch.cuda.synchronize()
            drawn = torch.from_numpy(R.dropout_mask(n, h, w, 0.5, seed))
            assert torch.equal(mo.cpu(), drawn), (n, h, w, "drawn mask")
            assert torch.equal(_bits(y.cpu()), _bits(R.dropout(x, drawn, channel))) and torch.equal(_bits(y2), _bits(y)), (n, h, w, "drawn")
            others = [k for k in range(c) if k != channel]
            assert torch.equal(_bits(y.cpu()[:, others]), _bits(x[:, others]))
    assert 0 < float(drawn.mean()) < 1


def test_uniform_dropout_grid_stride():
    """One plane of 4100 x 4100 = 16 810 000 elements for a grid capped at 65 536 x 256 = 16 777 216: the last 8 rows come from the second pass.
    The reference runs the same float32 operations with torch on the device."""
    ops = _ops()
    h = w = 4100
    assert h * w > 65536 * 256
    gen = torch.Generator(device=DEV).manual_seed(95)
    x = torch.rand((1, 1, h, w), generator=gen, device=DEV)
    mask = (torch.rand((1, 1, h, w), generator=gen, device=DEV) < 0.5).float()
    y, mo = ops.uniform_dropout(x, mask, want_mask=True)
    torch.cuda.synchronize()
    ref = R.dropout(x, mask, 0)
    assert torch.equal(_bits(y[..., -9:, :]), _bits(ref[..., -9:, :])) and torch.equal(_bits(y), _bits(ref)) and torch.equal(mo, mask)
    assert not torch.equal(y[..., -9:, :], x[..., -9:, :])
    y, mo = ops.uniform_dropout(x, None, keep_prob=0.25, seed=77, want_mask=True)
    torch.cuda.synchronize()
    assert torch.equal(mo.cpu(), torch.from_numpy(R.dropout_mask(1, h, w, 0.25, 77)))
    assert torch.equal(_bits(y), _bits(R.dropout(x, mo, 0))) and abs(float(mo.mean()) - 0.25) < 1e-3


# ---- 8. u8 -> unit float --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 255, 257, 16384 * 256 + 3])
def test_u8_to_unit_counts(count):
    """Bitwise numpy's x.astype(float32) / float32(255) on every byte value, below and past one block and past the grid cap of 16 384 blocks."""
    ops = _ops()
    x = ((np.arange(count, dtype=np.int64) * 7 + 250) % 256).astype(np.uint8)
    assert count < 256 or len(np.unique(x)) == 256
    got = ops.u8_to_unit(torch.from_numpy(x).to(DEV))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), (x.astype(np.float32) / np.float32(255)).view(np.uint32))


def test_u8_to_unit_all_bytes_and_nothing():
    ops, lib = _ops(), _lib.load()
    x = np.arange(256, dtype=np.uint8)
    got = ops.u8_to_unit(torch.from_numpy(x).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), (x.astype(np.float32) / np.float32(255)).view(np.uint32))
    assert got[0] == 0.0 and got[255] == 1.0
    buf = torch.full((1024,), 0x5A, dtype=torch.uint8, device=DEV)                  # count 0: success, nothing written
    ops.check(lib.wsu_u8_to_unit_f32(buf.data_ptr(), buf.data_ptr() + 512, 0, _stream()), "wsu_u8_to_unit_f32")
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())


# ---- 9. WS residual statistics and the epoch meter ------------------------------------------------------------------------------------------------
WS_IMAGES = [(3, 3), (3, 1025), (3, 1026), (3, 1027), (34, 34), (35, 35), (64, 48)]          # interiors of 1, 1023, 1024, 1025, 1024, 1089, 2852 pixels


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("h,w", WS_IMAGES)
def test_ws_residual_stats_edges(h, w, n):
    """One interior pixel for 1024 threads, interiors one short of, at and one past the 1024 threads.  The kernel sums exact float32 terms in
    fp64 and rounds once: at most one float32 ulp from the float32 operation sequence of oracle/np_ops.ws_stats accumulated in fp64 --
    measured 0 ulp everywhere.  A perfect predictor gives exactly 0 and 0, a flipped one exactly 1 and 1."""
    ops = _ops()
    rng = np.random.default_rng(100 + h + w + n)
    u8 = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    u8[0, 1, 1] = 255 if n == 1 else 0
    y = rng.random((n, h, w), dtype=np.float32)

    def run(pred):
        b, l = ops.ws_residual_stats(torch.from_numpy(u8).to(DEV), torch.from_numpy(pred).to(DEV))
        torch.cuda.synchronize()
        return b.cpu().numpy(), l.cpu().numpy()
    worst = 0.0
    for pred in (y, (u8.astype(np.float32) / np.float32(255))):
        gb, gl = run(pred)
        rb, rl = R.ws_stats(u8, pred)
        for got, ref in ((gb, rb), (gl, rl)):
            r32 = ref.astype(np.float32)
            ulps = np.abs(got.astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
            assert (ulps <= 1.0).all(), (got, ref)
            worst = max(worst, float(ulps.max()))
    print(f"ws_residual_stats {h}x{w} n={n}: {worst:.2f} ulp")
    gb, gl = run(u8.astype(np.float32) / np.float32(255))
    assert (gb == 0).all() and (gl == 0).all()
    gb, gl = run((u8 ^ 1).astype(np.float32) / np.float32(255))
    assert (gb == 1).all() and (gl == 1).all()


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("h,w", WS_IMAGES)
def test_ws_meter_beta_edges(h, w, n):
    """metrics.WSMeter.update's beta_hat in fp64 on the same float32 xi = x * 255; |got - ref| <= (cnt + 2) 2^-53 sum |term| (two roundings
    per term, a fixed-order sum of cnt terms) -- measured err / bound 1.8e-4 at most.  A third of the pixels are float32 x with x * 255 exactly
    k + 0.5, for even and for odd k, where np.round goes to the even neighbour: rounding half away from zero would flip x_bar, and the sign
    of the term, at every even k."""
    ops = _ops()
    even, odd = R.half_ties()
    assert len(even) > 100 and len(odd) > 100
    assert (even * np.float32(255) % 2 == 0.5).all() and (odd * np.float32(255) % 2 == 1.5).all()
    rng = np.random.default_rng(200 + h + w + n)
    x = (rng.integers(0, 256, (n, h, w)).astype(np.float32) / np.float32(255))
    pick = rng.integers(0, 6, (n, h, w))
    x = np.where(pick == 0, rng.choice(even, (n, h, w)), np.where(pick == 1, rng.choice(odd, (n, h, w)), x)).astype(np.float32)
    x[:, 1, 1] = even[3 % len(even)]
    y = rng.random((n, h, w), dtype=np.float32)
    got = ops.ws_meter_beta(torch.from_numpy(x[:, None]).to(DEV), torch.from_numpy(y[:, None]).to(DEV))
    torch.cuda.synchronize()
    ref, s = R.ws_meter(x, y)
    cnt = (h - 2) * (w - 2)
    bound = (cnt + 2) * 2.0 ** -53 * s
    err = np.abs(got.cpu().numpy() - ref)
    assert (s > 0).all()
    _report(f"ws_meter_beta {h}x{w} n={n}", float((err / bound).max()))


# ---- 10. the reflect ring of the NHWC 3x3 data gradient -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(2, 3), (3, 3), (4, 4), (2, 40), (40, 2)])
def test_conv3x3_bwd_data_reflect_ring_sizes(h, w):
    """ring_gather / ring_fold where rows 1 and h - 2 (columns 1 and w - 2) coincide, touch or swap: fp32 mode, one and two gradient outputs
    (cin 64, and 128 split 64 + 64), masked and not, against fp64 autograd; max error <= 2e-5 max|ref| (tests/test_gpu_backward.py), on
    the whole tensor and on the ring's rows and columns alone -- measured 7.1e-7 at most."""
    ops = _ops()
    n, cout, worst = 2, 64, 0.0
    ring = torch.zeros((h, w), dtype=torch.bool)
    ring[[1, h - 2], :] = True
    ring[:, [1, w - 2]] = True
    for cin, csplit in ((64, 64), (128, 64)):
        wt = R.rand((cout, cin, 3, 3), 300 + cin, (2.0 / (9 * cin)) ** 0.5)
        g = R.rand((n, cout, h, w), 301)
        act = torch.relu(R.rand((n, cin, h, w), 302))
        x = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
        F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), wt.double()).backward(g.double())
        wd, gd = _dev(wt), _dev(g.permute(0, 2, 3, 1))
        wp = ops.pack_conv3x3(wd, F32, dgrad=True)
        for masked in (False, True):
            ref = x.grad * (act > 0) if masked else x.grad
            m1 = _dev(act[:, :csplit].permute(0, 2, 3, 1)) if masked else None
            m2 = _dev(act[:, csplit:].permute(0, 2, 3, 1)) if (masked and csplit < cin) else None
            dx1, dx2 = ops.conv3x3_bwd_data(gd, wp, wd, csplit, m1, m2, F32)
            torch.cuda.synchronize()
            assert (dx2 is None) == (csplit == cin)
            got = torch.cat([t.cpu().permute(0, 3, 1, 2) for t in (dx1, dx2) if t is not None], dim=1)
            for sel in (slice(None), ring):
                a, b = got[:, :, sel].double(), ref[:, :, sel]
                rel = float((a - b).abs().max()) / float(b.abs().max())
                assert rel <= 2e-5, ((h, w), cin, masked, rel)
                worst = max(worst, rel)
            if masked:
                assert float(got[act <= 0].abs().max()) == 0.0
    print(f"conv3x3_bwd_data ring {h}x{w}: max err / max|ref| = {worst:.2e}")


# ---- 11. argument errors --------------------------------------------------------------------------------------------------------------------------
P = "P"                                                      # stands for the dummy non-null device pointer


def _c(entry, args, text, **change):
    """one refused call: `args` are the entry's valid arguments in order (P = the dummy pointer, the stream is appended), `change` replaces
    arguments by position (a3=...)"""
    args = list(args)
    for k, v in change.items():
        args[int(k[1:])] = v
    return pytest.param(entry, args, text, id=f"{entry[4:]}-{'-'.join(f'{k}={v}' for k, v in change.items())}")


_FIRST_FWD = [P, P, P, P, 1, 4, 4, 1, 64, 0, 1]              # x w bias y n h w cin cout mode relu
_HEAD_FWD = [P, P, P, P, P, 1, 4, 4, 64, 1, 0]               # x w bias out logit n h w c cout mode
_POOL_FWD = [P, P, P, 1, 4, 4, 8, 0]                         # x y idx n h w c mode
_DROPOUT = [P, "Q", P, P, 1, 1, 4, 4, 0, 0.5, 1]             # x y mask mask_out n c h w channel keep_prob seed  (Q: a second pointer)
_U8 = [P, P, 16]
_STATS = [P, P, P, P, 1, 4, 4]                               # x_u8 y01 beta l1 n h w
_METER = [P, P, P, 1, 4, 4]
_FIRST_BD = [P, P, P, 1, 4, 4, 1, 64]                        # g w dx n h w cin cout
_FIRST_BW = [P, P, P, P, P, 1 << 20, 1, 4, 4, 1, 64]         # g x dw db ws ws_bytes n h w cin cout
_RING = [P, P, P, P, 1 << 24, P, None, 64, None, None, 1, 4, 4, 64, 64, 0]      # g wp w ws ws_bytes dx1 dx2 csplit m1 m2 n h w cin cout mode
_POOL_BWD = [P, P, P, P, 1, 4, 4, 8, 1]                      # g dyp idx mask n h w c accumulate
_HEAD_BWD = [P, P, P, P, P, P, P, P, 1 << 22, 1, 4, 4, 64, 1, 1]                # x w out dout gx dw db ws ws_bytes n h w c cout relu_mask

REFUSED = (
    [_c("wsu_conv3x3_first_fwd", _FIRST_FWD, "conv3x3_first: bad mode", a9=m) for m in (-1, 3)]
    + [_c("wsu_conv3x3_first_fwd", _FIRST_FWD, "conv3x3_first: null pointer", **{f"a{i}": None}) for i in (0, 1, 3)]
    + [_c("wsu_conv3x3_first_fwd", _FIRST_FWD, "conv3x3_first: bad shape", **{f"a{i}": v}) for i, v in ((4, 0), (5, 1), (6, 1))]
    + [_c("wsu_conv3x3_first_fwd", _FIRST_FWD, "outside 1..8", a7=v) for v in (0, 9)]
    + [_c("wsu_conv3x3_first_fwd", _FIRST_FWD, f"cout={v} unsupported", a8=v) for v in (0, 4, 12, 24, 4096)]
    + [_c("wsu_conv3x3_first_fwd", _FIRST_FWD, "conv3x3_first: grid too large", a4=1 << 30, a8=2048)]
    + [_c("wsu_conv3x3_first_fwd", _FIRST_FWD, f"cin={ci} x cout={co}", a7=ci, a8=co) for ci, co in ((8, 1024), (3, 2048), (5, 1024))]
    + [_c("wsu_conv1x1_sigmoid_fwd", _HEAD_FWD, "conv1x1_sigmoid: bad mode", a10=m) for m in (-1, 3)]
    + [_c("wsu_conv1x1_sigmoid_fwd", _HEAD_FWD, "conv1x1_sigmoid: null pointer", **{f"a{i}": None}) for i in (0, 1, 3)]
    + [_c("wsu_conv1x1_sigmoid_fwd", _HEAD_FWD, "conv1x1_sigmoid: bad shape", **{f"a{i}": 0}) for i in (5, 6, 7, 9)]
    + [_c("wsu_conv1x1_sigmoid_fwd", _HEAD_FWD, f"c={v} must give", a8=v, a10=m) for v, m in ((0, 0), (6, 0), (12, 0), (512, 0), (4, 2), (24, 2), (1024, 2))]
    + [_c("wsu_conv1x1_sigmoid_fwd", _HEAD_FWD, "conv1x1_sigmoid: grid too large", a5=1 << 30, a6=64, a7=8, a8=4)]
    + [_c("wsu_maxpool2x2_fwd", _POOL_FWD, "maxpool2x2: bad mode", a7=m) for m in (-1, 3)]
    + [_c("wsu_maxpool2x2_fwd", _POOL_FWD, "maxpool2x2: null pointer", **{f"a{i}": None}) for i in (0, 1)]
    + [_c("wsu_maxpool2x2_fwd", _POOL_FWD, "maxpool2x2: bad shape", **ch) for ch in ({"a3": 0}, {"a4": 1}, {"a5": 1}, {"a6": 0}, {"a6": 6}, {"a6": 4, "a7": 2}, {"a6": 12, "a7": 2})]
    + [_c("wsu_uniform_dropout_fwd", _DROPOUT, "uniform_dropout: null or aliased", **ch) for ch in ({"a0": None}, {"a1": None}, {"a1": P})]
    + [_c("wsu_uniform_dropout_fwd", _DROPOUT, "uniform_dropout: bad shape", **ch) for ch in ({"a4": 0}, {"a5": 0}, {"a6": 1}, {"a7": 1}, {"a8": -1}, {"a8": 1}, {"a5": 3, "a8": 3})]
    + [_c("wsu_u8_to_unit_f32", _U8, "u8_to_unit_f32: null pointer", **{f"a{i}": None}) for i in (0, 1)]
    + [_c("wsu_ws_residual_stats", _STATS, "ws_residual_stats: null pointer", **{f"a{i}": None}) for i in range(4)]
    + [_c("wsu_ws_residual_stats", _STATS, "ws_residual_stats: bad shape", **{f"a{i}": v}) for i, v in ((4, 0), (5, 2), (6, 2))]
    + [_c("wsu_ws_meter_beta", _METER, "ws_meter_beta: null pointer", **{f"a{i}": None}) for i in range(3)]
    + [_c("wsu_ws_meter_beta", _METER, "ws_meter_beta: bad shape", **{f"a{i}": v}) for i, v in ((3, 0), (4, 2), (5, 2))]
    + [_c("wsu_conv3x3_first_bwd_data", _FIRST_BD, "conv3x3_first_bwd_data: null pointer", **{f"a{i}": None}) for i in range(3)]
    + [_c("wsu_conv3x3_first_bwd_data", _FIRST_BD, "conv3x3_first_bwd_data: bad shape", **{f"a{i}": v}) for i, v in ((3, 0), (4, 1), (5, 1), (6, 0), (6, 9), (7, 0), (7, 6))]
    + [_c("wsu_conv3x3_first_bwd_data", _FIRST_BD, f"cin={ci} x cout={co}", a6=ci, a7=co) for ci, co in ((8, 1024), (1, 4556), (5, 1024))]
    + [_c("wsu_conv3x3_first_bwd_weight", _FIRST_BW, "conv3x3_first_bwd_weight: null pointer", **{f"a{i}": None}) for i in (0, 1, 2, 4)]
    + [_c("wsu_conv3x3_first_bwd_weight", _FIRST_BW, "conv3x3_first_bwd_weight: bad shape", **{f"a{i}": v}) for i, v in ((6, 0), (7, 1), (8, 1), (9, 0), (9, 9), (10, 0), (10, 32), (10, 96))]
    + [_c("wsu_conv3x3_first_bwd_weight", _FIRST_BW, "conv3x3_first_bwd_weight: workspace too small", a5=10 * 64 * 4 - 1)]
    + [_c("wsu_conv3x3_bwd_data", _RING, "conv3x3_bwd_data: fp32-storage modes only", a15=m) for m in (2, 3, 4, 7)]
    + [_c("wsu_conv3x3_bwd_data", _RING, "conv3x3_bwd_data: null weight / workspace", **{f"a{i}": None}) for i in (2, 3)]
    + [_c("wsu_conv3x3_bwd_data", _RING, "conv3x3_bwd_data: cin=", **ch) for ch in ({"a13": 32}, {"a7": 62}, {"a14": 62})]
    + [_c("wsu_conv3x3_bwd_data", _RING, "conv3x3_bwd_data: workspace too small", a4=1024)]
    + [_c("wsu_maxpool2x2_bwd", _POOL_BWD, "maxpool2x2_bwd: null pointer", **{f"a{i}": None}) for i in range(3)]
    + [_c("wsu_maxpool2x2_bwd", _POOL_BWD, "maxpool2x2_bwd: bad shape", **{f"a{i}": v}) for i, v in ((4, 0), (5, 1), (6, 1), (7, 0), (7, 6))]
    + [_c("wsu_conv1x1_sigmoid_bwd", _HEAD_BWD, "conv1x1_sigmoid_bwd: null pointer", **{f"a{i}": None}) for i in range(8)]
    + [_c("wsu_conv1x1_sigmoid_bwd", _HEAD_BWD, f"conv1x1_sigmoid_bwd: c={v} unsupported", a12=v) for v in (0, 6, 12, 512)]
    + [_c("wsu_conv1x1_sigmoid_bwd", _HEAD_BWD, f"conv1x1_sigmoid_bwd: cout={v} outside", a13=v) for v in (0, 5)]
    + [_c("wsu_conv1x1_sigmoid_bwd", _HEAD_BWD, "conv1x1_sigmoid_bwd: workspace too small", a8=65 * 4 - 1)]
)


@pytest.fixture(scope="module")
def untouched():
    """16 MB of 0x5A that every refused call gets as each of its tensors: larger than anything the named shapes would touch"""
    return torch.full((16 << 20,), 0x5A, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("entry,args,text", REFUSED)
def test_refused_arguments(untouched, entry, args, text):
    """Every WSU_REQUIRE of the entries above: the call returns the argument error with the named text in wsu_last_error(), and nothing was
    launched -- the block every pointer names is unchanged."""
    lib = _lib.load()
    p = untouched.data_ptr()
    real = [p if a == P else (p + (8 << 20) if a == "Q" else a) for a in args]
    rc = getattr(lib, entry)(*real, _stream())
    msg = lib.wsu_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -1 and text in msg, (rc, msg)                # WSU_ERR_ARG
    with pytest.raises(_lib.WsuError, match=entry):
        _lib.check(rc, entry)
    assert bool((untouched == 0x5A).all())


def test_first_layer_lds_limit_is_the_compute_units():
    """include/wsu.h: cin * cout * 36 bytes of weights may fill the 160 KB of a compute unit's LDS, and the largest accepted products run:
    cin 1 x cout 2048 forward (73 728 B), cin 8 x cout 512 both ways (147 456 B), cin 1 x cout 4548 backward (163 728 B)."""
    ops = _ops()
    for cin, cout in ((1, 2048), (8, 512), (2, 2048)):
        x, wt = R.dyadic((1, cin, 3, 5), 400 + cin), R.dyadic((cout, cin, 3, 3), 401, 1.0)
        ref, s = R.conv_first(x, wt, None, False)
        R.exact_budget(ref, s, 2.0 ** -6)
        assert torch.equal(_sync_cpu(ops.conv3x3_first(_dev(x), _dev(wt), None, F32, relu=False)), ref.float()), (cin, cout)
    for cin, cout in ((8, 512), (1, 4548)):
        g, wt = R.dyadic((1, 3, 5, cout), 402 + cin, 1.0), R.dyadic((cout, cin, 3, 3), 403, 1.0)
        ref, s = R.conv_first_dgrad(g, wt)
        R.exact_budget(ref, s, 2.0 ** -6)
        assert torch.equal(_sync_cpu(ops.conv3x3_first_bwd_data(_dev(g), _dev(wt))), ref.float()), (cin, cout)
