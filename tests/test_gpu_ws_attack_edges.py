"""GPU: the WS estimator kernel K11 (ops.ws_attack: wsu_ws_attack / wsu_ws_attack_taps) at its edges, against tests/ws_np.py -- K11 restated
in numpy with its three sums taken exactly -- and its two small neighbours (ops.filter3x3_valid, ops.lsb_delta_unit) bit for bit.

a. the returned sums (sum w, sum w s res, sum w s bias): |got - exact| <= (cnt + 2) 2^-53 sum |term|, cnt = (H-2)(W-2) -- the bound of
   test_gpu_nhwc_edges.py::test_ws_meter_beta_edges for a fixed-order fp64 sum of float32 terms (one rounding per addition, one for the
   reference): it holds only if every float32 term has the bits of numpy's.  Measured err / bound: 1.3e-5 at most, 0 in most cases (the
   fp64 sum of a few thousand float32 terms of similar size is usually exact);
b. beta_hat equals ws_np.finish of the RETURNED sums by value: the finish is a handful of fp64 operations and one rounding;
c. image i of a batch equals, bitwise, the call on image i alone;
d. non-finite predictions follow numpy: np.clip(nan, 0, None) is nan;
e. ops.filter3x3_valid and ops.lsb_delta_unit, with their grid-stride branches;
f. the refusals test_gpu_ws_attack.py does not try.
Shapes: the smallest that cross a boundary of the kernel (64 row parts per image, 256 threads across a row)."""
import numpy as np
import pytest
import torch

import ws_np
from gpu_util import DEV
from oracle import ws_ref
from ws_unet_amd import filters, formula, ops
from ws_unet_amd.ws import estimate

pytestmark = pytest.mark.gpu

K2D = {name: np.asarray(filters.NAMED_FILTERS_2D[name])[..., 0] for name in ("KB", "AVG", "AVG9")}
SOURCES = ("inner", "full", "filter", "filters")
MODES = [(w, cb, mean) for mean in ("AVG", "AVG9") for w in (1, 0, -1) for cb in (False, True)]
SHAPES = [(1, 3, 3), (2, 3, 258), (2, 3, 259), (1, 66, 3), (1, 67, 3), (3, 67, 259), (5, 35, 70), (300, 5, 6)]
CONTENTS = ("random", "zeros", "all255", "checker255", "checker01", "even", "odd", "synthetic")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _images(content, shape, rng):
    n, h, w = shape
    if content == "synthetic":
        return formula.synthetic_images(n, h, w, seed=17 + h + w)
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    board = ((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1).astype(np.uint8)
    return {"random": x, "zeros": np.zeros_like(x), "all255": np.full_like(x, 255), "checker255": np.broadcast_to(board * 255, shape).copy(),
            "checker01": np.broadcast_to(board, shape).copy(), "even": x & 254, "odd": x | 1}[content]


def _source(source, x, rng, filter_name="KB"):
    """the prediction of one source as ws_np's per-image keywords and as ops.ws_attack's batch keywords (host arrays)"""
    n, h, w = x.shape
    if source == "inner":                                    # interiors in pixel units
        hat = (rng.random((n, h - 2, w - 2), dtype=np.float32) * np.float32(255.0)).astype(np.float32)
        bias = rng.standard_normal((n, h - 2, w - 2)).astype(np.float32)
        return dict(x_hat=hat, x_bias=bias, hat_scale=1.0)
    if source == "full":                                     # full frames in [0, 1]
        hat = rng.random((n, h, w), dtype=np.float32)
        bias = (rng.standard_normal((n, h, w)) * 0.01).astype(np.float32)
        return dict(x_hat=hat, x_bias=bias, hat_scale=255.0)
    if source == "filter":
        return dict(pixel_filter=K2D[filter_name])
    return dict(pixel_filter=(rng.standard_normal((n, 3, 3)) * 0.3).astype(np.float32))      # a different filter for every image


def _one(src, i):
    """image i's share of a batch source, still a batch (of one)"""
    out = {}
    for k, v in src.items():
        per_image = k in ("x_hat", "x_bias") or (k == "pixel_filter" and np.ndim(v) == 3)
        out[k] = v[i:i + 1] if per_image else v
    return out


def _gpu(x, src, weighted, correct_bias, mean):
    kw = {k: v for k, v in src.items() if k not in ("x_hat", "x_bias")}
    hat = _dev(src["x_hat"]) if "x_hat" in src else None
    if "x_bias" in src and correct_bias:
        kw["x_bias"] = _dev(src["x_bias"])
    beta, sums = ops.ws_attack(_dev(x), hat, mean_filter=K2D[mean], weighted=weighted, correct_bias=correct_bias, return_sums=True, **kw)
    assert beta.dtype == torch.float32 and beta.shape == (x.shape[0],) and sums.dtype == torch.float64 and sums.shape == (x.shape[0], 3)
    return beta.cpu().numpy(), sums.cpu().numpy()


def _ref(x, src, i, weighted, correct_bias, mean):
    kw = dict(mean_kernel=K2D[mean], weighted=weighted, correct_bias=correct_bias)
    if "pixel_filter" in src:
        k = src["pixel_filter"]
        return ws_np.attack(x[i], pixel_kernel=k[i] if np.ndim(k) == 3 else k, **kw)
    return ws_np.attack(x[i], x_hat=src["x_hat"][i], x_bias=src["x_bias"][i], hat_scale=src["hat_scale"], **kw)


def _finish_all(sums, correct_bias):
    return np.array([ws_np.finish(s[0], s[1], s[2], correct_bias) for s in sums], dtype=np.float32)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check(x, src, weighted, correct_bias, mean, what, alone=True):
    """a, b and c of one batch; returns the largest err / bound of its sums"""
    n, h, w = x.shape
    cnt = (h - 2) * (w - 2)
    beta, sums = _gpu(x, src, weighted, correct_bias, mean)
    worst = 0.0
    for i in range(n):
        _, s_ref, s_abs = _ref(x, src, i, weighted, correct_bias, mean)
        bound = (cnt + 2) * 2.0 ** -53 * s_abs
        err = np.abs(sums[i] - s_ref)
        assert np.isfinite(s_ref).all() and np.isfinite(sums[i]).all() and s_abs[0] > 0, (what, i, sums[i], s_ref)
        assert (err <= bound).all(), (what, f"image {i}", "sums", sums[i], "exact", s_ref, "err / bound", err / np.maximum(bound, 1e-300))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    assert np.array_equal(beta, _finish_all(sums, correct_bias), equal_nan=True), (what, beta, sums)               # b
    if alone and n > 1:                                                                                           # c
        for i in range(n):
            b1, s1 = _gpu(x[i:i + 1], _one(src, i), weighted, correct_bias, mean)
            assert _bits_equal(b1[0], beta[i]) and _bits_equal(s1[0], sums[i]), (what, f"image {i} alone", b1, beta[i], s1, sums[i])
    return worst


def _report(group, worst):
    print(f"{group}: largest err / bound = {worst:.3g}")
    assert worst <= 1.0, (group, worst)


# ---- a, b, c: sums against the exact reference, the finish, batch positions ----------------------------------------------------------------

@pytest.mark.parametrize("source", SOURCES)
def test_sums_every_mode(source):
    """(3,67,259) random bytes -- 65 interior rows over 64 row parts, 257 interior columns over 256 threads -- with every weighted x
    correct_bias under both mean filters (AVG: mu, mu2 exact; AVG9: every tap product rounds); the one filter is KB under AVG and AVG9
    under AVG9."""
    shape = (3, 67, 259)
    rng = np.random.default_rng(1100 + SOURCES.index(source))
    x = _images("random", shape, rng)
    worst = 0.0
    for weighted, cb, mean in MODES:
        src = _source(source, x, rng, filter_name="KB" if mean == "AVG" else "AVG9")
        worst = max(worst, _check(x, src, weighted, cb, mean, f"{source} weighted={weighted} correct_bias={cb} mean={mean}"))
    _report(f"ws_attack sums {source} {shape} all modes", worst)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_shapes(shape, source):
    """one interior pixel; 256 / 257 interior columns; 64 / 65 interior rows; both at once; an ordinary ragged shape; many images.  The mode
    walks with the shape, so that every source meets every weighted, correct_bias and mean filter."""
    k = SHAPES.index(shape)
    weighted, cb, mean = (1, 0, -1)[k % 3], bool(k % 2), ("AVG", "AVG9")[(k // 2) % 2]
    rng = np.random.default_rng(1200 + 10 * k + SOURCES.index(source))
    x = _images("random", shape, rng)
    src = _source(source, x, rng, filter_name=("KB", "AVG9")[k % 2])
    _report(f"ws_attack sums {source} {shape} weighted={weighted} correct_bias={cb} mean={mean}",
            _check(x, src, weighted, cb, mean, f"{source} {shape}"))


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("content", CONTENTS)
def test_sums_contents(content, source):
    """flat planes (var = 0: the largest weight), the 0/255 checkerboard (the largest variance), the 0/1 checkerboard, planes of one parity
    (s of one sign: nothing cancels), and the package's synthetic images, at (5,35,70)"""
    k = CONTENTS.index(content)
    weighted, cb, mean = (1, -1, 0)[k % 3], bool((k + 1) % 2), ("AVG9", "AVG")[(k // 2) % 2]
    shape = (5, 35, 70)
    rng = np.random.default_rng(1300 + 10 * k + SOURCES.index(source))
    x = _images(content, shape, rng)
    src = _source(source, x, rng, filter_name=("AVG9", "KB")[k % 2])
    _report(f"ws_attack sums {source} {content} weighted={weighted} correct_bias={cb} mean={mean}",
            _check(x, src, weighted, cb, mean, f"{source} {content}"))


def _signed_hat(x, d, sign):
    """interior predictions (scale 1) x + sign * s * d, s = x - x_bar: every term w s res is -sign * w * d"""
    xi = x[:, 1:-1, 1:-1]
    s = xi.astype(np.float32) - (xi ^ 1).astype(np.float32)
    return (xi.astype(np.float32) + np.float32(sign) * s * np.asarray(d, dtype=np.float32)).astype(np.float32)


@pytest.mark.parametrize("weighted", [1, 0, -1])
def test_finish_takes_each_side_of_the_clip(weighted):
    """x_hat = x + s d, d > 0: the raw statistic is negative and beta_hat is 0 (also after the bias correction: 0 - 0 * c); x_hat = x - s d:
    positive, and the bias correction applies.  The side is asserted on the reference."""
    shape = (3, 9, 70)
    rng = np.random.default_rng(1400 + weighted)
    x = _images("random", shape, rng)
    d = rng.random((3, 7, 68), dtype=np.float32) + np.float32(0.5)
    bias = rng.standard_normal((3, 7, 68)).astype(np.float32)
    for sign, cb in ((+1, False), (+1, True), (-1, False), (-1, True)):
        src = dict(x_hat=_signed_hat(x, d, sign), x_bias=bias, hat_scale=1.0)
        for i in range(3):
            b_ref, s_ref, _ = _ref(x, src, i, weighted, cb, "AVG")
            assert (s_ref[1] / s_ref[0] < -0.5) if sign > 0 else (s_ref[1] / s_ref[0] > 0.5)
            assert (b_ref == 0) if sign > 0 else (b_ref != 0)
        _check(x, src, weighted, cb, "AVG", f"sign={sign} correct_bias={cb}")
        beta, _ = _gpu(x, src, weighted, cb, "AVG")
        assert ((beta == 0) if sign > 0 else (beta != 0)).all(), (sign, cb, beta)


@pytest.mark.parametrize("weighted", [1, 0, -1])
def test_negative_estimate_after_bias_correction_comes_back(weighted):
    """0/255 checkerboard, KB, correct_bias: every term s res is 510 and every s bias is 3, so beta_hat = 510 - 510 * 3 = -1020 (to the
    float32 rounding of w * 510 and w * 3; exactly for the weights 1 and 5 + var): the clip comes before the correction, and what the
    correction makes negative stays negative"""
    x = _images("checker255", (2, 8, 9), np.random.default_rng(0))
    src = dict(pixel_filter=K2D["KB"])
    b_ref = _ref(x, src, 0, weighted, True, "AVG")[0]
    assert abs(float(b_ref) + 1020.0) <= 1020.0 * 1e-6 and (weighted == 1 or b_ref == np.float32(-1020.0)), b_ref
    _check(x, src, weighted, True, "AVG", "checkerboard KB correct_bias")
    beta, _ = _gpu(x, src, weighted, True, "AVG")
    assert (np.abs(beta.astype(np.float64) + 1020.0) <= 1020.0 * 1e-6).all() and (weighted == 1 or (beta == np.float32(-1020.0)).all()), beta


# ---- d: non-finite predictions ------------------------------------------------------------------------------------------------------------

ND_SHAPE = (3, 67, 259)
ND_PIXELS = {"first": (1, 1), "middle": (33, 130), "last": (65, 257)}


def _nd_case(seed):
    rng = np.random.default_rng(seed)
    x = _images("random", ND_SHAPE, rng)
    return x, rng


@pytest.mark.parametrize("where", list(ND_PIXELS))
@pytest.mark.parametrize("source", ["inner", "full"])
def test_nan_in_a_prediction_gives_nan_for_that_image_alone(source, where):
    """a NaN at one interior pixel of image 1's x_hat: beta_hat[1] is NaN as np.clip(nan, 0, None) is (not 0, 'no payload'); images 0 and 2
    keep their bits"""
    x, rng = _nd_case(1500)
    src = _source(source, x, rng)
    base_b, base_s = _gpu(x, src, 1, False, "AVG")
    assert np.isfinite(base_b).all()
    r, c = ND_PIXELS[where]
    bad = dict(src, x_hat=src["x_hat"].copy())
    bad["x_hat"][1][(r, c) if source == "full" else (r - 1, c - 1)] = np.nan
    b_ref, s_ref, _ = _ref(x, bad, 1, 1, False, "AVG")
    assert np.isnan(b_ref) and np.isnan(s_ref[1]) and np.isfinite(s_ref[0])
    beta, sums = _gpu(x, bad, 1, False, "AVG")
    assert np.isnan(sums[1, 1]) and _bits_equal(sums[1, 0], base_s[1, 0])
    assert np.isnan(beta[1]), f"beta_hat = {beta[1]} where numpy gives nan"
    for i in (0, 2):
        assert _bits_equal(beta[i], base_b[i]) and _bits_equal(sums[i], base_s[i]), i
    assert np.array_equal(beta, _finish_all(sums, False), equal_nan=True)


def test_nan_in_the_border_ring_of_a_full_frame_changes_nothing():
    x, rng = _nd_case(1501)
    src = _source("full", x, rng)
    bad = dict(src, x_hat=src["x_hat"].copy(), x_bias=src["x_bias"].copy())
    for a in (bad["x_hat"], bad["x_bias"]):
        a[:, 0, :] = a[:, -1, :] = a[:, :, 0] = a[:, :, -1] = np.nan
    for cb in (False, True):
        (b0, s0), (b1, s1) = _gpu(x, src, 1, cb, "AVG"), _gpu(x, bad, 1, cb, "AVG")
        assert np.isfinite(b0).all() and _bits_equal(b0, b1) and _bits_equal(s0, s1), cb


@pytest.mark.parametrize("value", [np.inf, -np.inf])
@pytest.mark.parametrize("parity", [0, 1])
def test_inf_in_a_prediction_follows_numpy(parity, value):
    """res = x - (+-inf), the term -+s inf: the statistic is +-inf, beta_hat inf or (clipped) 0, as ws_np gives"""
    x, rng = _nd_case(1502)
    r, c = ND_PIXELS["middle"]
    x[1, r, c] = (x[1, r, c] & 254) | parity
    src = _source("inner", x, rng)
    src["x_hat"][1, r - 1, c - 1] = value
    b_ref, s_ref, _ = _ref(x, src, 1, 1, False, "AVG")
    assert np.isinf(s_ref[1]) and b_ref == (np.inf if s_ref[1] > 0 else 0.0)
    beta, sums = _gpu(x, src, 1, False, "AVG")
    assert sums[1, 1] == s_ref[1] and beta[1] == b_ref, (beta[1], b_ref, sums[1], s_ref)
    assert np.isfinite(beta[[0, 2]]).all()
    assert np.array_equal(beta, _finish_all(sums, False), equal_nan=True)


@pytest.mark.parametrize("sign", [+1, -1])
def test_nan_in_the_bias_prediction_gives_nan(sign):
    """correct_bias with a NaN in image 1's x_bias: NaN, also where the raw statistic is negative (sign +1): 0 - 0 * nan"""
    x, rng = _nd_case(1503)
    d = rng.random((3, 65, 257), dtype=np.float32) + np.float32(0.5)
    src = dict(x_hat=_signed_hat(x, d, sign), x_bias=rng.standard_normal((3, 65, 257)).astype(np.float32), hat_scale=1.0)
    base_b, base_s = _gpu(x, src, 1, True, "AVG")
    assert np.isfinite(base_b).all() and ((base_s[:, 1] < 0) if sign > 0 else (base_s[:, 1] > 0)).all()
    src["x_bias"][1, 32, 129] = np.nan
    b_ref, s_ref, _ = _ref(x, src, 1, 1, True, "AVG")
    assert np.isnan(b_ref) and np.isnan(s_ref[2]) and ((s_ref[1] < 0) if sign > 0 else (s_ref[1] > 0))
    beta, sums = _gpu(x, src, 1, True, "AVG")
    assert np.isnan(sums[1, 2]) and _bits_equal(sums[1, :2], base_s[1, :2])
    assert np.isnan(beta[1]), f"beta_hat = {beta[1]} where numpy gives nan"
    for i in (0, 2):
        assert _bits_equal(beta[i], base_b[i]) and _bits_equal(sums[i], base_s[i]), i
    beta_off, _ = _gpu(x, src, 1, False, "AVG")                  # without correct_bias x_bias is not read
    assert np.isfinite(beta_off).all()


def test_driver_reports_nan_for_a_host_prediction_with_a_nan():
    """estimate._stat with a host estimator whose plane for the second image holds one NaN: NaN for that image, the others unchanged"""
    planes = formula.synthetic_images(3, 20, 24, seed=9)
    planes[1] = formula.lsbr_embed(planes[1], 0.6, seed=2)
    host = [p.astype(np.float32)[..., None] for p in planes]

    def cross_mean(xf):
        return ((xf[:-2, 1:-1] + xf[2:, 1:-1] + xf[1:-1, :-2] + xf[1:-1, 2:]) * np.float32(0.25))[..., :1]

    def with_nan(xf):
        y = cross_mean(xf).copy()
        if np.array_equal(xf, host[1]):
            y[7, 5, 0] = np.nan
        return y

    x_u8 = _dev(planes)
    avg = filters.NAMED_FILTERS_2D["AVG"]
    for weighted in (1, 0):
        good = estimate._stat(x_u8, cross_mean, avg, weighted, False, host_planes=host).cpu().numpy()
        got = estimate._stat(x_u8, with_nan, avg, weighted, False, host_planes=host).cpu().numpy()
        assert np.isfinite(good).all()
        assert np.isnan(got[1]), f"beta_hat = {got[1]} for a prediction with a NaN"
        assert _bits_equal(got[[0, 2]], good[[0, 2]])


# ---- e: the two small kernels -----------------------------------------------------------------------------------------------------------------

def _filter_ref(x, k):
    return np.stack([ws_ref.conv3x3_valid((p / np.float32(255.0)).astype(np.float32), k) * np.float32(255.0) for p in x])


@pytest.mark.parametrize("shape", [(1, 3, 3), (2, 5, 7), (1, 3, 258), (1, 4099, 4099)], ids=lambda s: "x".join(map(str, s)))
def test_filter3x3_valid_bit_for_bit(shape):
    """convolve(x / 255., K, 'valid') * 255. with an asymmetric K on arbitrary float32 planes; (1,4099,4099) has 4097^2 = 16 785 409 interior
    pixels, more than the 65536 * 256 threads of the largest grid: the grid-stride branch"""
    rng = np.random.default_rng(1600 + shape[2])
    x = (rng.random(shape, dtype=np.float32) * np.float32(300.0) - np.float32(20.0)).astype(np.float32)
    kernels = [(rng.standard_normal((3, 3)) * 0.3).astype(np.float32)] + ([K2D["KB"], K2D["AVG9"]] if shape[1] < 100 else [])
    xd = _dev(x)
    for k in kernels:
        got = ops.filter3x3_valid(xd, k).cpu().numpy()
        want = _filter_ref(x, k)
        assert got.shape == want.shape == (shape[0], shape[1] - 2, shape[2] - 2) and got.dtype == want.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


def _lsb_ref(u):
    return ((u ^ 1).astype(np.float32) - u.astype(np.float32)) / np.float32(255.0)


@pytest.mark.parametrize("count", [1, 255, 256, 257, 16777216 + 257])
def test_lsb_delta_unit_bit_for_bit(count):
    """((x ^ 1) - x) / 255. around one workgroup of 256 and past the 65536 * 256 threads of the largest grid (the grid-stride branch)"""
    u = np.random.default_rng(1700).integers(0, 256, count, dtype=np.uint8)
    got = ops.lsb_delta_unit(_dev(u))
    assert got.shape == (count,) and got.dtype == torch.float32
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), _lsb_ref(u).view(np.int32))


def test_lsb_delta_unit_on_a_view_one_byte_into_an_allocation():
    u = np.random.default_rng(1701).integers(0, 256, 1025, dtype=np.uint8)
    view = _dev(u)[1:]
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    np.testing.assert_array_equal(ops.lsb_delta_unit(view).cpu().numpy().view(np.int32), _lsb_ref(u[1:]).view(np.int32))


# ---- f: refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    kb, avg = K2D["KB"], K2D["AVG"]
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(Exception, match="weighted=2"):
        ops.ws_attack(x, None, pixel_filter=kb, mean_filter=avg, weighted=2)
    with pytest.raises(Exception, match="weighted=2"):
        ops.ws_attack(x, None, pixel_filter=np.stack([kb, kb]), mean_filter=avg, weighted=2)
    for shape in ((1, 2, 8), (1, 8, 2)):
        with pytest.raises(Exception, match="bad shape"):
            ops.ws_attack(torch.zeros(shape, dtype=torch.uint8, device=DEV), None, pixel_filter=kb, mean_filter=avg)
    many = torch.zeros((65536, 3, 3), dtype=torch.uint8, device=DEV)          # the grid's y extent ends at 65535
    with pytest.raises(Exception, match="bad shape n=65536"):
        ops.ws_attack(many, None, pixel_filter=kb, mean_filter=avg)
    beta = ops.ws_attack(many[:65535], None, pixel_filter=kb, mean_filter=avg)
    assert beta.shape == (65535,) and bool((beta == 0).all())
    for stack in (np.stack([kb]), np.stack([kb, kb, kb])):
        with pytest.raises(ValueError, match="filters for 2 images"):
            ops.ws_attack(x, None, pixel_filter=stack, mean_filter=avg)
