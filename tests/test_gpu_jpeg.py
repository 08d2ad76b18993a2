"""GPU: the JPEG-history kernels (K31 wsu_jpeg_energies, K32 wsu_jpeg_predict) bit for bit against numpy (jpeg_np): the energies as
int64, the quality found, the prediction as float32 bits and the recompressed uint8 planes; then the three WS statistics on that
prediction against their own restatements."""
import math

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import jpeg_np
import locate_np
import sequential_np
from ws_unet_amd import filters, ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import estimate, jpeg

pytestmark = pytest.mark.gpu

AVG = filters.NAMED_FILTERS_2D["AVG"]
AVG3 = np.asarray(AVG, dtype=np.float32).reshape(3, 3)
COVERS = (6, 7, 8, 9, 10)
MIXED = np.where((np.arange(64).reshape(8, 8) * 7 + np.arange(64).reshape(8, 8) // 8) % 3 == 0, 255, 1)       # 1 and 255, DC entry 255
TABLES = {"all 1 (q = 100)": jpeg_np.table(100), "all 255 (q = 1)": jpeg_np.table(1), "1 and 255 mixed": MIXED, "q = 50": jpeg_np.table(50),
          "q = 90": jpeg_np.table(90)}


def _contents(shape, seed):
    n, h, w = shape
    rr, cc = np.indices((h, w))
    full = lambda p: np.broadcast_to(p.astype(np.uint8), shape).copy()
    return {"all 0": np.zeros(shape, np.uint8), "all 255": np.full(shape, 255, np.uint8), "checkerboard": full((rr + cc) % 2 * 255),
            "vertical stripes": full(cc % 2 * 255), "random": np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _assert_predict_equal(x, tabs, use=None):
    hat, out = ops.jpeg_predict(_dev(x), tabs, use, want_u8=True)
    want_hat, want_out = jpeg_np.predict(x, tabs, use)
    assert hat.dtype == torch.float32 and out.dtype == torch.uint8 and hat.shape == x.shape == out.shape
    np.testing.assert_array_equal(_bits(hat.cpu().numpy()), _bits(want_hat))
    np.testing.assert_array_equal(out.cpu().numpy(), want_out)
    return hat


@pytest.mark.parametrize("shape", [(1, 8, 8), (1, 16, 24), (3, 64, 64), (2, 8, 1032)])
def test_energies_and_prediction_equal_numpy_bit_for_bit(shape):
    """one block; six blocks; 64 blocks of three images (half a workgroup's 128 slots, the others transform as zeros); 129 blocks in one
    block row (a second workgroup with one block).  All 0, all 255, a 0 / 255 checkerboard (the largest coefficient: Y[7][7]), vertical
    stripes, random pixels; tables of all 1, all 255, 1 and 255 mixed, two IJG tables."""
    tabs = np.stack(list(TABLES.values()))
    assert MIXED.min() == 1 and MIXED.max() == 255 and MIXED[0, 0] == 255
    for name, x in _contents(shape, sum(shape)).items():
        got = ops.jpeg_energies(_dev(x), tabs)
        assert got.dtype == torch.int64 and got.shape == (shape[0], len(tabs))
        np.testing.assert_array_equal(got.cpu().numpy(), jpeg_np.energies(x, tabs), err_msg=name)
        for tname, t in TABLES.items():
            _assert_predict_equal(x, np.stack([t] * shape[0]))
    # a plane of 128 is X = 0: every coefficient, residual and energy is 0, and the round trip gives it back
    flat = np.full(shape, 128, np.uint8)
    assert not ops.jpeg_energies(_dev(flat), tabs).any()
    np.testing.assert_array_equal(ops.jpeg_recompress(_dev(flat), 1).cpu().numpy(), flat)


def test_one_table_per_image_and_an_image_without_history():
    """N = 3 at 64 x 64: a different table per image, the second image predicted with KB (interior) and itself (border), its table unread"""
    x = _contents((3, 64, 64), 5)["random"]
    x[2] = jpeg_np.recompress(x[2:3], 60)[0]
    tabs = np.stack([jpeg_np.table(35), np.zeros((8, 8), np.int64), MIXED])
    use = np.array([1, 0, 1], dtype=np.uint8)
    hat = _assert_predict_equal(x, tabs, use).cpu().numpy()
    np.testing.assert_array_equal(hat[1][0], x[1][0].astype(np.float32))
    np.testing.assert_array_equal(hat[1][:, -1], x[1][:, -1].astype(np.float32))
    # K11 on that plane has the bits of K11 with the KB filter in the kernel, weighted or not
    xd = _dev(x[1:2])
    for weighted in (0, 1, -1):
        a = ops.ws_attack(xd, _dev(hat[1:2]), mean_filter=AVG, hat_scale=1.0, weighted=weighted)
        b = ops.ws_attack(xd, None, pixel_filter=filters.NAMED_FILTERS_2D["KB"], mean_filter=AVG, weighted=weighted)
        assert torch.equal(a, b), weighted
    # every image without history; x_hat alone; the recompressed planes alone
    _assert_predict_equal(x, tabs, np.zeros(3, np.uint8))
    np.testing.assert_array_equal(ops.jpeg_recompress(_dev(x), 35).cpu().numpy(), jpeg_np.recompress(x, 35))
    np.testing.assert_array_equal(_bits(ops.jpeg_predict(_dev(x), tabs, use).cpu().numpy()), _bits(jpeg_np.predict(x, tabs, use)[0]))


def test_more_images_and_tables_than_one_launch_takes():
    """33 tables and 33 images (a launch takes 32 of either), with dirty output buffers, twice"""
    x = np.random.default_rng(33).integers(0, 256, (33, 16, 8), dtype=np.uint8)
    tabs = jpeg_np.tables(range(40, 73))
    xd = _dev(x)
    want = jpeg_np.energies(x, tabs)
    lib = ops._lib.load()
    e = torch.full((33, 33), 7, dtype=torch.int64, device=DEV)
    t32 = np.ascontiguousarray(tabs, dtype=np.int32)
    for _ in range(2):
        ops.check(lib.wsu_jpeg_energies(xd.data_ptr(), t32.ctypes.data, 33, e.data_ptr(), 33, 16, 8, ops._stream()), "wsu_jpeg_energies")
        np.testing.assert_array_equal(e.cpu().numpy(), want)
    use = (np.arange(33) % 5 != 0).astype(np.uint8)
    _assert_predict_equal(x, tabs, use)


@pytest.fixture(scope="module")
def precompressed():
    """the five golden covers precompressed by the oracle at quality 75, then LSBR at alpha = 0.4 from numpy's generator"""
    covers = np.stack([np.ascontiguousarray(imread4_u8(GOLDEN / f"cover_{k}.png")[..., 3]) for k in COVERS])
    x = jpeg_np.lsbr(jpeg_np.recompress(covers, 75), 0.4, np.random.default_rng(75))
    return x


def test_golden_covers_against_all_95_tables(precompressed):
    x = precompressed
    tabs = jpeg_np.tables(range(1, 96))
    q, e = jpeg.estimate_quality(_dev(x), return_energies=True)
    want = jpeg_np.energies(x, tabs)
    np.testing.assert_array_equal(e.cpu().numpy(), want)
    want_q = [jpeg_np.quality(row, 512 * 512) for row in want]
    print(f"q_hat {q.tolist()}; energy per pixel at q_hat {[round(want[i][want_q[i] - 1] / 2 ** 38, 3) for i in range(5)]}")
    assert q.dtype == torch.int64 and q.tolist() == want_q and all(abs(v - 75) <= 2 for v in want_q)
    np.testing.assert_array_equal(jpeg_np.estimate_quality(x[:1]), want_q[:1])
    _assert_predict_equal(x, jpeg_np.tables(want_q))
    with pytest.raises(ValueError, match="multiples of 8"):
        jpeg.estimate_quality(_dev(x[:, :500]))
    with pytest.raises(ValueError, match="1..255"):
        ops.jpeg_energies(_dev(x[:1]), np.zeros((1, 8, 8), np.int32))
    with pytest.raises(ValueError, match="for 5 images"):
        ops.jpeg_predict(_dev(x), tabs[:5], np.ones(4))


def test_the_ws_statistics_on_the_recompression_prediction(precompressed):
    """K11 unweighted against the float64 formula on the ORACLE's prediction (the tolerance of the full-frame x_hat tests of
    test_gpu_ws_attack.py: rel 2e-6, abs 2e-7); K27 and K29 are exact integers: equal."""
    x = precompressed[:2]
    est = jpeg.JPEGEstimator()
    xd = _dev(x)
    hat = est.planes(xd)
    assert est.fallbacks == 0
    want_hat = jpeg_np.predict(x, jpeg_np.tables(jpeg_np.estimate_quality(x)))[0]
    np.testing.assert_array_equal(_bits(hat.cpu().numpy()), _bits(want_hat))
    beta = ops.ws_attack(xd, hat, hat_scale=1.0, weighted=0).cpu().numpy()
    for i in range(2):
        ref = max(jpeg_np.beta_unweighted(x[i], want_hat[i]), 0.)
        print(f"image {i}: beta_hat {beta[i]:.6f}, float64 {ref:.6f}")
        assert math.isclose(float(beta[i]), ref, rel_tol=2e-6, abs_tol=2e-7) and abs(ref - 0.2) <= 0.05
    for weighted in (0, 1):
        k, t_max, t_all = ops.ws_sequential(xd, hat, mean_filter=AVG, hat_scale=1.0, weighted=weighted, order="rows")
        num = torch.zeros((510, 510), dtype=torch.int64, device=DEV)
        den = torch.zeros_like(num)
        ops.ws_residual_accumulate(xd, num, den, hat, mean_filter=AVG, hat_scale=1.0, weighted=weighted)
        for i in range(2):
            wk, wmax, wall, _ = sequential_np.ws_sequential_np(x[i], "rows", x_hat=want_hat[i], hat_scale=1.0, mean_kernel=AVG3, weighted=weighted)
            assert (k[i].item(), t_max[i].item(), t_all[i].item()) == (wk, wmax, wall)
        wnum, wden = locate_np.accumulate(x, x_hats=want_hat, hat_scale=1.0, mean_kernel=AVG3, weighted=weighted)
        np.testing.assert_array_equal(num.cpu().numpy(), wnum)
        np.testing.assert_array_equal(den.cpu().numpy(), wden)


def test_estimator_fallbacks_and_fixed_quality(precompressed):
    x = np.stack([precompressed[0], np.ascontiguousarray(imread4_u8(GOLDEN / "cover_6.png")[..., 3])])
    xd = _dev(x)
    est = jpeg.JPEGEstimator()
    hat = est.planes(xd).cpu().numpy()
    assert est.fallbacks == 1
    np.testing.assert_array_equal(_bits(hat[1]), _bits(jpeg_np.kb_plane(x[1])))
    none = jpeg.JPEGEstimator(fallback=None)
    hat_none = none.planes(xd).cpu().numpy()
    assert none.fallbacks == 1 and np.isnan(hat_none[1]).all()
    np.testing.assert_array_equal(_bits(hat_none[0]), _bits(hat[0]))
    for placed in ({}, dict(placement="sequential", order="rows_up")):      # an image without a prediction has no estimate
        beta = estimate._stat(xd, jpeg.JPEGEstimator(fallback=None), AVG, 1, False, **placed).cpu().numpy()
        assert np.isnan(beta).tolist() == [False, True]
        np.testing.assert_array_equal(beta[:1], estimate._stat(xd[:1], jpeg.JPEGEstimator(), AVG, 1, False, **placed).cpu().numpy())
    fixed = jpeg.JPEGEstimator(quality=60)
    np.testing.assert_array_equal(_bits(fixed.planes(xd).cpu().numpy()), _bits(jpeg_np.predict(x, jpeg_np.tables([60, 60]))[0]))
    assert fixed.fallbacks == 0
    # the host call pattern of the reference's estimators: (H,W,C) float in, (H-2,W-2,1) out
    y = jpeg.JPEGEstimator()(x[0].astype(np.float32)[..., None])
    assert y.shape == (510, 510, 1) and y.dtype == np.float32
    np.testing.assert_array_equal(_bits(y[..., 0]), _bits(hat[0][1:-1, 1:-1]))
