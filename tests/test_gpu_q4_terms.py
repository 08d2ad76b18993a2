"""The forward kernels of the default inference mode 'f16f4p' on planar Q tensors -- conv3x3_q (K1q: plain, pooled, half-block, fused head,
fused first layer), conv3x3_up_q (K1u), their one-product siblings on planar H tensors, and the Q producers of planar.hip -- held to THEIR
arithmetic: f16 w * f16 x on the f16 pipe plus the two residual cross terms as block-scaled fp4, on the bytes the operands STORE, as restated
in tests/q4_np.py from include/wsu.h.  The bands of tests/test_gpu_q.py / test_gpu_qu.py (3e-5 of the scale with 2 % outliers, 5e-4 against
the exact convolution) admit a kernel without cross terms and cannot see an error confined to a few pixels; these tests can.

Family A (bit for bit): operands crafted as bytes from small dyadic sets -- the scale byte of every (pixel, chunk) hashed on its own -- so that
every product is a multiple of one quantum and the sum of their magnitudes stays below 2^24 quanta: any summation order and any rounding mode
give one fp32 value, and every byte the output format defines is determined (f16 planes, in-image scale bytes, all 32 nibbles; format A and H
planes; fp32 logits; the pooled tensor).  Variants (a) no residuals, (b) / (c) one cross term alone, (d) all three (tests/q4_cases.py).

Family B (realistic operands through the real encodings): E1 = rel_l2 between the f16-only and the three-term restatement, both through the
output's own encoding; the kernel must sit within 0.25 E1 of the three-term value over all pixels and over the image's border ring alone (a
wrong padding changes only the ring).

Stores: ragged shapes write into a caller's buffer between two 4 KiB guards; guards and the scale plane's padding slots stay untouched, and
every in-image byte is written.

Observed on an MI355X (profiles/r44): see q4_terms.txt there.
"""
import pytest
import torch

import f16f8_cases as C8
import f16f8_np as P8
import q4_cases as C
import q4_np as P
from gpu_util import DEV, planar_encode, planar_h_encode, planar_q_encode

pytestmark = pytest.mark.gpu
GUARD = 4096


def _ops():
    from ws_unet_amd import ops
    return ops


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _q(t):
    return None if t is None else _ops().PlanarQ(t.data.to(DEV), t.n, t.c, t.h, t.w)


def _h(t):
    return None if t is None else _ops().PlanarH(t.data.to(DEV), t.n, t.c, t.h, t.w)


def _back(t) -> P.QT:
    return P.QT(t.data.cpu(), t.n, t.c, t.h, t.w)


def _flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _dev(t):
    return None if t is None else t.to(DEV)


def run_conv(c: dict, y_format=None, pool=False, **head):
    """conv3x3_q / conv3x3_h on case c -> (what ops returns, range flag)"""
    ops = _ops()
    cout, flag = c["shape"][5], _flag()
    if c["kind"] == "h":
        res = ops.conv3x3_h(_h(c["x1"]), _h(c["x2"]), ops.pack_conv3x3_h(c["w"].to(DEV)), _dev(c["bias"]), cout, relu=c["relu"], pool=pool, range_flag=flag, **head)
    else:
        res = ops.conv3x3_q(_q(c["x1"]), _q(c["x2"]), ops.pack_conv3x3_f4(c["w"].to(DEV)), _dev(c["bias"]), cout, relu=c["relu"], pool=pool, range_flag=flag,
                            y_format=ops.PLANAR_Q if y_format is None else y_format, **head)
    return res, int(flag.item())


def run_up(c: dict):
    """conv3x3_up_q / conv3x3_up_h on case c -> (y, range flag); the packer's combined weights and bias are held to float64 first"""
    ops = _ops()
    fmt_h = c["kind"] == "uh"
    pack, conv, enc = (ops.pack_conv3x3_up_h, ops.conv3x3_up_h, _h) if fmt_h else (ops.pack_conv3x3_up, ops.conv3x3_up_q, _q)
    w_skip, w_low, bias, dense = pack(c["w3"].to(DEV), c["wt"].to(DEV), _dev(c.get("bt")), _dev(c.get("b3")), want_dense=True)
    if c["variant"] != "B":
        assert c["wc_exact"] and c["bias_exact"]
        assert torch.equal(dense.cpu(), c["wc"]), "combined class weights: dense != Wc"
        assert torch.equal(bias.cpu(), c["bias"]), "combined bias"
    else:                                                                   # fp32 sums in the packer's order against the fp64 sums rounded once
        assert float((dense.cpu().double() - c["wc"].double()).abs().max()) <= 2e-6 * float(c["wc"].abs().max())
    flag = _flag()
    y = conv(enc(c["xl"]), enc(c["xs"]), w_skip, w_low, bias, c["shape"][6], relu=c["relu"], range_flag=flag)
    return y, int(flag.item())


def _conditions(c: dict) -> None:
    """conditions on the operands of a family A case, asserted before the kernel's result is looked at"""
    assert C.window_ok(c), "the operands leave the exactness window"
    f16, ca, cb = c["raw"]
    v = c["variant"]
    if v == "a":
        assert float(ca.abs().max()) == 0 and float(cb.abs().max()) == 0
    if v == "b":
        assert float(ca.abs().max()) > 0 and float(cb.abs().max()) == 0 and float(f16.abs().max()) == 0
    if v == "c":
        assert float(cb.abs().max()) > 0 and float(ca.abs().max()) == 0 and float(f16.abs().max()) == 0
    if v == "d":
        assert float(ca.abs().max()) > 0 and float(cb.abs().max()) > 0 and float(f16.abs().max()) > 0


def _assert_q(got, want, what):
    bad = P.q_mismatch(_back(got), want)
    assert bad is None, (what, bad)


# ---- the restated encoders against tests/gpu_util.py ---------------------------------------------------------------------------------------
def test_store_encoding_restatements_match_gpu_util():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 32, 19, 45), generator=g) * torch.exp2(torch.randint(-6, 7, (2, 32, 1, 1), generator=g).float())
    x[0, :16, 3, 4] = 0.0                                                   # an all-zero block
    x[1, 5, 7, 8] = 447.9
    assert torch.equal(P.q_encode(x).data, planar_q_encode(x).data.cpu())
    assert torch.equal(P.h_encode(x).data, planar_h_encode(x).data.cpu())
    assert torch.equal(P.a_encode(x), planar_encode(x).view(torch.uint8).cpu())


# ---- family A: K1q ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", [(s, v) for s in C.Q_SHAPES for v in "abcd"], ids=_ids)
def test_a_conv3x3_q(shape, variant):
    ops = _ops()
    c = C.case("q", shape, variant)
    _conditions(c)
    pool = shape in C.Q_POOL
    want = c["three"]
    for fmt in ((ops.PLANAR_Q, ops.PLANAR_A) if variant == "d" or pool else (ops.PLANAR_Q,)):
        res, flag = run_conv(c, fmt, pool)
        y, yp = res if pool else (res, None)
        if fmt == ops.PLANAR_Q:
            _assert_q(y, want, ("y", shape, variant))
            if pool:
                _assert_q(yp, P.max_pool(want), ("y_pool", shape, variant))
        else:
            assert P.a_equal(y, want), ("y format A", shape, variant)
            assert not pool or P.a_equal(yp, P.max_pool(want)), ("y_pool format A", shape, variant)
        assert flag == 0
    if pool:                                                                # the pooled output alone
        (y_none, yp), _ = run_conv(c, ops.PLANAR_Q, True, want_y=False)
        assert y_none is None
        _assert_q(yp, P.max_pool(want), ("y_pool alone", shape, variant))


def test_a_conv3x3_q_large_grid_and_repeats():
    """320 work items of two steps (the non-split plain variant; workgroups walk two tiles): three launches, each exact -- so equal"""
    c = C.case("q", C.Q_LARGE, "d")
    _conditions(c)
    want = P.q_encode(c["three"].float())
    for _ in range(3):
        y, flag = run_conv(c)
        assert P.q_same_bytes(_back(y), want) and flag == 0


@pytest.mark.parametrize("channels", C.HEAD_CHANNELS + [(17,)], ids=_ids)
def test_a_conv3x3_q_head(channels):
    """the fused head with one-hot head weights: the fp32 logit IS the ReLU output of the selected channels (plus a dyadic head bias), which
    resolves every bit of variant d; a y beside the head is a format A tensor"""
    c = C.case("q", C.Q_HEAD, "d")
    _conditions(c)
    hc = len(channels)
    hw_ = torch.zeros((hc, 64, 1, 1))
    hw_[torch.arange(hc), list(channels)] = 1.0
    hb = torch.tensor([0.5, -1.0, 0.25][:hc])
    (out, logit, y), flag = run_conv(c, head_w=hw_.to(DEV), head_b=hb.to(DEV), want_logit=True, want_y=True)
    want = P.head_logit(c["three"], hw_, hb)
    assert torch.equal(want, c["three"][:, list(channels)] + hb.double()[None, :, None, None])
    assert P.exact_equal(logit, want), float((logit.cpu().double() - want).abs().max())
    assert P.a_equal(y, c["three"]) and flag == 0
    assert float((out.cpu().double() - torch.sigmoid(want)).abs().max()) < 1e-6
    (_, logit2), _ = run_conv(c, head_w=hw_.to(DEV), head_b=hb.to(DEV), want_logit=True, want_y=False)
    assert P.exact_equal(logit2, want)


@pytest.mark.parametrize("shape", C.H_SHAPES, ids=_ids)
def test_a_conv3x3_h(shape):
    c = C.case("h", shape, "a")
    _conditions(c)
    pool = shape in C.Q_POOL
    res, flag = run_conv(c, pool=pool)
    y, yp = res if pool else (res, None)
    assert P.h_equal(_back(y), c["three"]) and flag == 0
    assert not pool or P.h_equal(_back(yp), P.max_pool(c["three"]))


# ---- family A: the first layer and the fused first layer ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.F1_SHAPES, ids=_ids)
def test_a_first_layer_store_encodings(shape):
    """conv3x3_first_pl on image values k / 16 and dyadic weights: the fp32 value is exact, so the bytes of all three formats are determined"""
    ops = _ops()
    f = C.first_pl_case(shape)
    img, w1, b1 = f["img"].to(DEV), f["w1"].to(DEV), f["b1"].to(DEV)
    hi = P.f16_round(f["y"].float())
    assert float((f["y"] - hi).abs().max()) > 0                              # the values carry residuals
    flag = _flag()
    _assert_q(ops.conv3x3_first_pl(img, w1, b1, y_format=ops.PLANAR_Q, range_flag=flag), f["y"], ("first_pl Q", shape))
    assert P.a_equal(ops.conv3x3_first_pl(img, w1, b1, y_format=ops.PLANAR_A, range_flag=flag), f["y"])
    assert P.h_equal(_back(ops.conv3x3_first_pl(img, w1, b1, y_format=ops.PLANAR_H, range_flag=flag)), f["y"])
    assert int(flag.item()) == 0


@pytest.mark.parametrize("shape", C.F1_SHAPES, ids=_ids)
def test_a_fused_first_q(shape):
    """conv3x3_q_fused_first against the restated e11 -> planar Q encoding -> three-term conv -> pool"""
    ops = _ops()
    c = C.case("f1", shape, "d")
    assert c["xe11_exact"]
    _conditions(c)
    flag = _flag()
    y, yp = ops.conv3x3_q_fused_first(c["img"].to(DEV), c["w1"].to(DEV), c["b1"].to(DEV), ops.pack_conv3x3_f4(c["w"].to(DEV)), c["bias"].to(DEV), shape[3],
                                      range_flag=flag)
    _assert_q(y, c["three"], ("fused first y", shape))
    _assert_q(yp, P.max_pool(c["three"]), ("fused first y_pool", shape))
    assert int(flag.item()) == 0


# ---- family A: K1u ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", [(s, v) for s in C.U_SHAPES for v in "abcd"], ids=_ids)
def test_a_conv3x3_up_q(shape, variant):
    c = C.case("u", shape, variant)
    _conditions(c)
    y, flag = run_up(c)
    _assert_q(y, c["three"], (shape, variant))
    assert flag == 0


def test_a_conv3x3_up_q_large_grid_and_repeats():
    """270 work items of three steps (the step region's parity flips from tile to tile inside a workgroup): three launches, each exact"""
    c = C.case("u", C.U_LARGE, "d")
    _conditions(c)
    want = P.q_encode(c["three"].float())
    for _ in range(3):
        y, flag = run_up(c)
        assert P.q_same_bytes(_back(y), want) and flag == 0


@pytest.mark.parametrize("shape", C.UH_SHAPES, ids=_ids)
def test_a_conv3x3_up_h(shape):
    c = C.case("uh", shape, "a")
    _conditions(c)
    y, flag = run_up(c)
    assert P.h_equal(_back(y), c["three"]) and flag == 0


# ---- family A: the transposed conv as a Q producer -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["a", "b", "c", "d"])
@pytest.mark.parametrize("shape", C8.TF_SHAPES, ids=_ids)
def test_a_convt2x2_pl_writes_q(shape, variant):
    """the family A cases of the e4m3 transposed conv (tests/f16f8_cases.py: their exact fp32 outputs exist) with y_format = PLANAR_Q"""
    ops = _ops()
    c = C8.case("tf", shape, variant)
    assert C8.window_ok(c)
    flag = _flag()
    y = ops.convt2x2_pl(P8.as_device_planar(c["ub"], DEV), ops.pack_convt2x2(c["vb"].to(DEV), ops.mode_id("f16f8")), _dev(c["bias"]), shape[4],
                        range_flag=flag, y_format=ops.PLANAR_Q)
    _assert_q(y, c["three"], ("convt2x2_pl Q", shape, variant))
    assert int(flag.item()) == 0


# ---- family B --------------------------------------------------------------------------------------------------------------------------------
def _through_q(v):
    return P.q_decode(P.q_encode(v.float()))


def _ratios(got, three, f16, what):
    """(E1, ratio) over all pixels and over the border ring, through the Q encoding; prints them"""
    out = []
    m = P.ring(*three.shape[2:])
    for name, sel in (("all", slice(None)), ("ring", m)):
        g, t, f = got[..., sel], _through_q(three)[..., sel], _through_q(f16)[..., sel]
        e1 = P.rel_l2(f, t)
        r = P.ratio(g, t, e1)
        print(f"q4 terms: {what} {name}: E1={e1:.3e} ratio={r:.4f}")
        out.append((e1, r, P.ratio_ok(g, t, e1)))
    return out


@pytest.mark.parametrize("shape", C.B_SHAPES["q"], ids=_ids)
def test_b_conv3x3_q(shape):
    c = C.case("q", shape, "B")
    pool = shape in C.B_POOL
    res, flag = run_conv(c, pool=pool)
    y, yp = res if pool else (res, None)
    rs = _ratios(P.q_decode(_back(y)), c["three"], c["f16"], f"conv3x3_q {shape}")
    if pool:
        rs += _ratios(P.q_decode(_back(yp)), P.max_pool(c["three"]), P.max_pool(c["f16"]), f"conv3x3_q {shape} pooled")
    assert all(ok for _, _, ok in rs), rs
    assert flag == 0


@pytest.mark.parametrize("shape", C.B_SHAPES["u"], ids=_ids)
def test_b_conv3x3_up_q(shape):
    c = C.case("u", shape, "B")
    y, flag = run_up(c)
    rs = _ratios(P.q_decode(_back(y)), c["three"], c["f16"], f"conv3x3_up_q {shape}")
    assert all(ok for _, _, ok in rs), rs
    assert flag == 0


# ---- stores stay inside ----------------------------------------------------------------------------------------------------------------------
def _guarded(nbytes: int, fill: int):
    buf = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
    assert (buf.data_ptr() + GUARD) % 256 == 0
    return buf


def _check_guarded(launch, layouts):
    """launch(pointers) runs the C entry on output buffers the test owns.  layouts: per output (n * chunks, chunk bytes, in-image byte mask of a
    chunk or None = every byte).  Pre-filled with 0xA5 and 0x5A: the guards and the chunk bytes outside the mask keep the fill, the bytes inside
    are the same in both launches (so every one of them was written)."""
    runs = []
    for fill in (0xA5, 0x5A):
        bufs = [_guarded(k * cb, fill) for k, cb, _ in layouts]
        assert launch([b.data_ptr() + GUARD for b in bufs]) == 0
        torch.cuda.synchronize()
        for b, (k, cb, mask) in zip(bufs, layouts):
            host = b.cpu()
            assert bool((host[:GUARD] == fill).all()) and bool((host[-GUARD:] == fill).all()), "a guard was written"
            body = host[GUARD:-GUARD].reshape(k, cb)
            if mask is not None:
                assert bool((body[:, ~mask] == fill).all()), "a padding slot of the scale plane was written"
        runs.append([b.cpu()[GUARD:-GUARD].reshape(k, cb) for b, (k, cb, _) in zip(bufs, layouts)])
    for a, b, (_, _, mask) in zip(runs[0], runs[1], layouts):
        sel = slice(None) if mask is None else mask
        assert torch.equal(a[:, sel], b[:, sel]), "an in-image byte was not written"
    return runs[0]


def _q_layout(n, c, h, w):
    cb = P.q_chunk_bytes(h, w)
    mask = torch.zeros(cb, dtype=torch.bool)
    mask[:48 * h * w] = True
    mask[48 * h * w + P.scale_index(h, w).reshape(-1)] = True
    return (n * (c // 16), cb, mask)


def _as_qt(body, n, c, h, w):
    return P.QT(body.reshape(n, c // 16, -1), n, c, h, w)


def test_ragged_stores_stay_inside_conv3x3_q():
    from ws_unet_amd import _lib
    ops, lib = _ops(), _lib.load()
    for shape in ((1, 17, 33, 64, 0, 64), (1, 4, 6, 32, 48, 128)):
        n, h, w, c1, c2, cout = shape
        pool = shape in C.Q_POOL
        c = C.case("q", shape, "d")
        x1, x2, wp, bias = _q(c["x1"]), _q(c["x2"]), ops.pack_conv3x3_f4(c["w"].to(DEV)), c["bias"].to(DEV)
        layouts = [_q_layout(n, cout, h, w)] + ([_q_layout(n, cout, h // 2, w // 2)] if pool else [])
        launch = lambda p: lib.wsu_conv3x3_q_fwd(x1.data_ptr(), None if x2 is None else x2.data_ptr(), wp.data_ptr(), bias.data_ptr(), p[0], p[1] if pool else None,
                                                 None, None, None, None, 0, n, h, w, c1, c2, cout, 1, ops.PLANAR_Q, None, ops._stream())
        got = _check_guarded(launch, layouts)
        assert P.q_equal(_as_qt(got[0], n, cout, h, w), c["three"])
        assert not pool or P.q_equal(_as_qt(got[1], n, cout, h // 2, w // 2), P.max_pool(c["three"]))


def test_ragged_stores_stay_inside_conv3x3_up_q():
    from ws_unet_amd import _lib
    ops, lib = _ops(), _lib.load()
    shape = (1, 9, 17, 32, 32, 16, 128)
    n, hl, wl, cl, cup, c2, cout = shape
    c = C.case("u", shape, "d")
    w_skip, w_low, bias = ops.pack_conv3x3_up(c["w3"].to(DEV), c["wt"].to(DEV), _dev(c["bt"]), _dev(c["b3"]))
    xl, xs = _q(c["xl"]), _q(c["xs"])
    launch = lambda p: lib.wsu_conv3x3_up_q_fwd(xl.data_ptr(), xs.data_ptr(), w_skip.data_ptr(), w_low.data_ptr(), bias.data_ptr(), p[0],
                                                n, 2 * hl, 2 * wl, cl, c2, cout, 1, None, ops._stream())
    got = _check_guarded(launch, [_q_layout(n, cout, 2 * hl, 2 * wl)])
    assert P.q_equal(_as_qt(got[0], n, cout, 2 * hl, 2 * wl), c["three"])


def test_ragged_stores_stay_inside_first_pl_and_convt2x2_pl():
    from ws_unet_amd import _lib
    ops, lib = _ops(), _lib.load()
    shape = (1, 18, 34, 64)
    n, h, w, cout = shape
    f = C.first_pl_case(shape)
    img, w1, b1 = f["img"].to(DEV), f["w1"].to(DEV), f["b1"].to(DEV)
    launch = lambda p: lib.wsu_conv3x3_first_pl_fwd(img.data_ptr(), w1.data_ptr(), b1.data_ptr(), p[0], n, h, w, 1, cout, 1, ops.PLANAR_Q, None, None, ops._stream())
    got = _check_guarded(launch, [_q_layout(n, cout, h, w)])
    assert P.q_equal(_as_qt(got[0], n, cout, h, w), f["y"])
    shape = (1, 5, 33, 64, 64, True)
    c = C8.case("tf", shape, "d")
    n, h, w, cin, cout = shape[:5]
    x, wp, bias = P8.as_device_planar(c["ub"], DEV), ops.pack_convt2x2(c["vb"].to(DEV), ops.mode_id("f16f8")), c["bias"].to(DEV)
    launch = lambda p: lib.wsu_convt2x2_pl_fwd(x.data_ptr(), wp.data_ptr(), bias.data_ptr(), p[0], n, h, w, cin, cout, ops.PLANAR_Q, None, ops._stream())
    got = _check_guarded(launch, [_q_layout(n, cout, 2 * h, 2 * w)])
    assert P.q_equal(_as_qt(got[0], n, cout, 2 * h, 2 * w), c["three"])
