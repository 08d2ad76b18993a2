"""GPU: the 5x5 least-squares predictors.  The moment kernel (K56) bit for bit against numpy and against K24 on the inner 3x3
variables; the prediction kernel (K57) bit for bit against the float32 restatement (ols5_np), bias plane and zero border included;
embedded KB through the WS statistic against the in-kernel KB filter; the adaptive predictors 'OLSa5x5' / 'OLSa5x5s' through
ws.estimate._stat against the statistic on the restated planes; the fallback of a flat image; the drivers, the data-set fit and its
command line.  Every comparison is exact unless it says otherwise."""
import json
import re
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import ols5_np
from ws_unet_amd import filters, ols5, ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import estimate

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
AVG2D, KB2D = filters.NAMED_FILTERS_2D["AVG"], filters.NAMED_FILTERS_2D["KB"]
_SRC = (GOLDEN.parent.parent / "ws_unet_amd" / "csrc" / "ols5.hip").read_text()
TR, TC = (int(re.search(rf"\b{name} = (\d+)", _SRC).group(1)) for name in ("O5_TR", "O5_TC"))      # K56's tile of windowed pixels


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


def _dev(x: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _moments(x: np.ndarray) -> np.ndarray:
    return ops.ols_moments5(_dev(x)).cpu().numpy()


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def stego():
    """{alpha: (planes (5,512,512) uint8, restated moments (5,325))} of the golden LSBR files, computed once"""
    out = {}
    for alpha in ("1.0", "0.1"):
        planes = np.stack([_plane(f"stego_LSBR_{alpha}_{k}.png") for k in COVERS])
        out[alpha] = (planes, ols5_np.moments(planes))
    return out


@pytest.fixture(scope="module")
def cover_moments():
    return np.stack([ols5_np.moments(_plane(f"cover_{k}.png")) for k in COVERS])


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the five golden covers and their LSBR alpha 1.0 twins as a data set"""
    root = tmp_path_factory.mktemp("ols5_data")
    (root / "images").mkdir()
    sdir = root / "stego_LSBR_alpha_1.0"
    sdir.mkdir()
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
        shutil.copy(GOLDEN / f"stego_LSBR_1.0_{k}.png", sdir / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    (sdir / "files.csv").write_text("name,height,width,stego_method,alpha\n" + "".join(
        f"stego_LSBR_alpha_1.0/{k}.png,512,512,LSBR,1.0\n" for k in COVERS))
    return root


@pytest.fixture
def registry():
    keep = dict(ols5.KERNELS)
    yield
    ols5.KERNELS.clear()
    ols5.KERNELS.update(keep)


# ---- K56 ----------------------------------------------------------------------------------------------------------------------------

def test_tile_constants():
    assert (TR, TC) == (64, 256)


@pytest.mark.parametrize("shape", [(2, 5, 5), (3, 6, 9), (1, 16, 300), (2, TR + 5, TC + 5), (2, 2 * TR + 7, 40)])
def test_moments_equal_numpy_bit_for_bit(shape):
    """one pixel; a few; a row length that is no multiple of the 256-column tile (two column tiles, the second ragged); one pixel past a
    full tile in both directions (four tiles); three row tiles"""
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    got = _moments(x)
    assert got.dtype == np.int64 and got.shape == (shape[0], 325)
    np.testing.assert_array_equal(got, ols5_np.moments(x))


@pytest.mark.parametrize("shape", [(1, TR + 4, TC + 4), (1, 512, 512)])
def test_moments_of_saturated_planes_do_not_overflow(shape):
    """all-255 planes: every product is 255 * 255.  The first shape is exactly one full tile, the most products a workgroup's 32-bit sums
    ever see (16 384 of the 66 051 they hold); 512 x 512 has full tiles too and the largest 64-bit totals."""
    count = (shape[1] - 4) * (shape[2] - 4)
    np.testing.assert_array_equal(_moments(np.full(shape, 255, dtype=np.uint8)), np.full((1, 325), 255 * 255 * count, dtype=np.int64))
    np.testing.assert_array_equal(_moments(np.zeros(shape, dtype=np.uint8)), np.zeros((1, 325), dtype=np.int64))


def test_moments_zero_their_output_and_are_deterministic():
    x = _dev(np.random.default_rng(2).integers(0, 256, (3, 70, 90), dtype=np.uint8))
    want = ols5_np.moments(x.cpu().numpy())
    lib = ops._lib.load()
    out = torch.full((3, 325), 12345, dtype=torch.int64, device=DEV)                # a dirty buffer, used twice
    for _ in range(2):
        ops.check(lib.wsu_ols_moments5(x.data_ptr(), out.data_ptr(), 3, 70, 90, ops._stream()), "wsu_ols_moments5")
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert torch.equal(ops.ols_moments5(x), ops.ols_moments5(x))
    assert torch.equal(ops.ols_moments5(x[1:2]), ops.ols_moments5(x)[1:2])           # the batch does not change an image's sums


def test_inner_3x3_moments_equal_the_3x3_kernel():
    """K56's sums over the inner ring and the centre are K24's on the plane without its outermost rows and columns"""
    x = np.random.default_rng(8).integers(0, 256, (2, 71, 300), dtype=np.uint8)
    full = np.zeros((2, 25, 25), dtype=np.int64)
    full[:, ols5_np.IU[0], ols5_np.IU[1]] = _moments(x)
    full = full + np.triu(full, 1).transpose(0, 2, 1)
    raster = [(a + 1) * 5 + (b + 1) for a, b in ops._RING] + [12]                     # K24's ring order, centre last, in the 5x5 raster
    var = [24 if r == 12 else r if r < 12 else r - 1 for r in raster]
    sub = full[:, var][:, :, var]
    iu = np.triu_indices(9)
    np.testing.assert_array_equal(sub[:, iu[0], iu[1]], ops.ols_moments(_dev(x[:, 1:-1, 1:-1])).cpu().numpy())


def test_moments_argument_errors():
    with pytest.raises(Exception, match="bad shape"):
        ops.ols_moments5(torch.zeros((1, 4, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(Exception, match="bad shape"):
        ops.ols_moments5(torch.zeros((1, 8, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(Exception, match="contiguous"):
        ops.ols_moments5(torch.zeros((1, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2])
    with pytest.raises(Exception, match="CPU tensor"):
        ops.ols_moments5(torch.zeros((1, 8, 8), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.ols_moments5(torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        ops.ols_moments5(torch.zeros((8, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="no images"):
        ops.ols_moments5(torch.zeros((0, 8, 8), dtype=torch.uint8, device=DEV))


# ---- K57 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 3, 3), (2, 5, 5), (3, 8, 12), (1, 67, 259)])
def test_prediction_equals_the_restatement_bit_for_bit(shape):
    """ring 1 only; one pixel with a full window; a few; five row tiles and two column tiles, both ragged"""
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    for taps in ((rng.normal(size=24) / 5.).astype(np.float32), (rng.normal(size=(shape[0], 24)) / 5.).astype(np.float32)):
        want_hat, want_bias = ols5_np.predict(x, taps)
        hat, bias = ops.predict5x5(_dev(x), _dev(taps), want_bias=True)
        assert hat.dtype == torch.float32 and tuple(hat.shape) == shape == tuple(bias.shape)
        np.testing.assert_array_equal(_bits(hat.cpu().numpy()), _bits(want_hat))
        np.testing.assert_array_equal(_bits(bias.cpu().numpy()), _bits(want_bias))
        for plane in (hat, bias):                                                     # the frame border is written, as zeros
            assert not plane[:, 0].any() and not plane[:, -1].any() and not plane[:, :, 0].any() and not plane[:, :, -1].any()
        alone = ops.predict5x5(_dev(x), _dev(taps))
        assert isinstance(alone, torch.Tensor) and torch.equal(alone, hat)


def test_prediction_argument_errors():
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    taps = torch.zeros(24, dtype=torch.float32, device=DEV)
    for bad in (torch.zeros(8, device=DEV), torch.zeros((3, 24), device=DEV), torch.zeros(24, dtype=torch.float64, device=DEV), np.zeros(24, dtype=np.float32)):
        with pytest.raises(ValueError, match="taps"):
            ops.predict5x5(x, bad)
    with pytest.raises(Exception, match="CPU tensor"):
        ops.predict5x5(x, taps.cpu())
    with pytest.raises(Exception, match="CPU tensor"):
        ops.predict5x5(x.cpu(), taps)
    with pytest.raises(Exception, match="contiguous"):
        ops.predict5x5(x, torch.zeros((2, 48), dtype=torch.float32, device=DEV)[:, ::2])
    with pytest.raises(Exception, match="contiguous"):
        ops.predict5x5(torch.zeros((2, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2], taps)
    with pytest.raises(ValueError):
        ops.predict5x5(x.to(torch.float32), taps)
    with pytest.raises(Exception, match="bad shape"):
        ops.predict5x5(torch.zeros((1, 2, 8), dtype=torch.uint8, device=DEV), taps)
    with pytest.raises(Exception, match="bad shape"):
        ops.predict5x5(torch.zeros((1, 8, 2), dtype=torch.uint8, device=DEV), taps)
    with pytest.raises(ValueError, match="5 x 5"):
        ols5.Predictor5x5(ols5_np.kb_taps()).planes(torch.zeros((1, 4, 8), dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("hw", [(5, 5), (20, 33)])
def test_embedded_kb_gives_the_bits_of_the_kb_filter(hw):
    x = _dev(np.random.default_rng(hw[1]).integers(0, 256, (3,) + hw, dtype=np.uint8))
    hat, bias = ops.predict5x5(x, _dev(ols5_np.kb_taps().astype(np.float32)), want_bias=True)
    for weighted in (-1, 0, 1):
        for correct_bias in (False, True):
            kw = dict(mean_filter=AVG2D, weighted=weighted, correct_bias=correct_bias, return_sums=True)
            beta, sums = ops.ws_attack(x, hat, x_bias=bias if correct_bias else None, hat_scale=1.0, **kw)
            beta_kb, sums_kb = ops.ws_attack(x, None, pixel_filter=KB2D, **kw)
            assert torch.equal(beta, beta_kb) and torch.equal(sums, sums_kb), (hw, weighted, correct_bias)


# ---- the adaptive predictors ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", ["1.0", "0.1"])
@pytest.mark.parametrize("name", ["OLSa5x5", "OLSa5x5s"])
def test_adaptive_predictors_match_the_statistic_on_the_restated_planes(stego, name, alpha):
    planes, moments = stego[alpha]
    x = _dev(planes)
    np.testing.assert_array_equal(ops.ols_moments5(x).cpu().numpy(), moments)
    taps, ok = ols5.fit(moments, symmetric=ols5.ADAPTIVE_NAMES[name])
    assert ok.all()
    hat, bias = (_dev(p) for p in ols5_np.predict(planes, taps.astype(np.float32)))
    for weighted, correct_bias in ((0, False), (1, False), (1, True), (-1, True)):
        est = ols5.estimator(name)
        beta = estimate._stat(x, est, AVG2D, weighted, correct_bias)
        ref = ops.ws_attack(x, hat, x_bias=bias if correct_bias else None, hat_scale=1.0, mean_filter=AVG2D, weighted=weighted,
                            correct_bias=correct_bias)
        print(f"{name} alpha {alpha} weighted {weighted} correct_bias {correct_bias}: beta_hat {beta.cpu().numpy()}")
        assert torch.equal(beta, ref), (weighted, correct_bias)
        assert est.fallbacks == 0
        if alpha == "1.0" and weighted == 0:
            b = beta.cpu().numpy()
            assert ((b >= 0.45) & (b <= 0.55)).all(), b


def test_a_flat_image_in_a_batch_falls_back_to_kb(caplog):
    x = _dev(np.stack([np.full((16, 16), 9, dtype=np.uint8), np.random.default_rng(4).integers(0, 256, (16, 16), dtype=np.uint8)]))
    kb = filters.FilterEstimator(KB2D)
    for name in ("OLSa5x5", "OLSa5x5s"):
        est = ols5.estimator(name)
        for weighted, correct_bias in ((0, False), (1, True)):
            beta = estimate._stat(x, est, AVG2D, weighted, correct_bias)
            assert torch.equal(beta[:1], estimate._stat(x[:1], kb, AVG2D, weighted, correct_bias))
        assert est.fallbacks == 2
        taps = est.image_taps(x).cpu().numpy()
        np.testing.assert_array_equal(taps[0], ols5_np.kb_taps().astype(np.float32))
        assert not np.array_equal(taps[1], taps[0])
    assert sum("OLS 5x5 fit" in r.getMessage() for r in caplog.records) == 2            # logged once per estimator, not per image
    # called like the reference's estimators: (H,W,C) float in, (H-2,W-2,1) out
    fixed = ols5.Predictor5x5(taps[1])
    y = fixed(x[1].cpu().numpy().astype(np.float32)[..., None])
    assert y.shape == (14, 14, 1) and y.dtype == np.float32
    np.testing.assert_array_equal(_bits(y[..., 0]), _bits(ols5_np.predict(x[1:2].cpu().numpy(), taps[1])[0][0][1:-1, 1:-1]))


# ---- drivers ------------------------------------------------------------------------------------------------------------------------------

def test_adaptive_predictors_through_ws_estimate(dataset, stego):
    fnames = [dataset / "stego_LSBR_alpha_1.0" / f"{k}.png" for k in COVERS]
    direct = estimate._stat(_dev(stego["1.0"][0]), ols5.estimator("OLSa5x5"), AVG2D, 1, True).cpu().numpy()
    rows = estimate.attack_batch(fnames, [{"name": f.name} for f in fnames], channels=(3,), pixel_estimator=ols5.estimator("OLSa5x5"),
                                 correct_bias=True, weighted=1)
    np.testing.assert_array_equal([r["beta_hat"] for r in rows], direct)
    for model_name in ("OLSa5x5", "OLSa5x5s"):
        resb = estimate.run(dataset, "LSBR", 1.0, model_name, None, (3,), correct_bias=False, weighted=0, batched=True, batch_size=2)
        res = estimate.run(dataset, "LSBR", 1.0, model_name, None, (3,), correct_bias=False, weighted=0, progress_on=False)
        assert resb["name"].tolist() == [f"stego_LSBR_alpha_1.0/{k}.png" for k in (10, 6, 7, 8, 9)] == res["name"].tolist()
        assert resb["model_name"].tolist() == [model_name] * 5
        np.testing.assert_allclose(resb["beta_hat"].to_numpy(float), res["beta_hat"].to_numpy(float), rtol=1e-6, atol=0)
        assert resb["beta_hat"].between(0.45, 0.55).all()
    for placed in (dict(placement="sequential", order="rows"), dict(placement="adaptive")):
        res = estimate.run(dataset, "LSBR", 1.0, "OLSa5x5", None, (3,), correct_bias=False, weighted=1, batched=True, **placed)
        assert len(res) == 5 and res["model_name"].tolist() == ["OLSa5x5"] * 5 and res["placement"].tolist() == [placed["placement"]] * 5


def test_olsa5x5_is_a_row_of_the_roc_scores(dataset):
    from ws_unet_amd.ws import roc
    res = roc.collect_ws_scores(dataset, ["LSBR"], [1.0], ["KB", "OLSa5x5"])
    assert res["model_name"].unique().tolist() == ["KB", "OLSa5x5"] and len(res) == 2 * 10
    run = estimate.run(dataset, "LSBR", 1.0, "OLSa5x5", None, (3,), correct_bias=False, weighted=0, batched=True)
    got = res[(res.model_name == "OLSa5x5") & (res.stego_method == "LSBR")]
    assert got["name"].tolist() == run["name"].tolist()
    np.testing.assert_array_equal(got["beta_hat"].to_numpy(np.float32), run["beta_hat"].to_numpy(np.float32))


def test_locate_and_keysearch_accept_the_name(dataset):
    from ws_unet_amd.ws import keysearch, locate
    plain = locate.run(dataset, "LSBR", 1.0, "OLSa5x5", None, (3,), weighted=1)
    assert len(plain) == 1 and plain["images"].tolist() == [5] and plain["model_name"].tolist() == ["OLSa5x5"]
    found = keysearch.run(dataset, "LSBR", 1.0, "OLSa5x5s", None, (3,), first=0, count=16, top=3)
    assert len(found) == 3 and found["model_name"].tolist() == ["OLSa5x5s"] * 3 and found["images"].tolist() == [5] * 3


def test_fit_dataset_and_command_line(dataset, cover_moments, tmp_path, capsys, registry):
    import pandas as pd
    total = cover_moments.sum(axis=0)
    count = 5 * 508 * 508
    for symmetric in (False, True):
        res = ols5.fit_dataset(dataset, symmetric=symmetric, batch_size=2)                # three chunks, the last of one image
        assert res.moments.dtype == np.int64 and res.count == count and res.ok
        np.testing.assert_array_equal(res.moments, total)
        np.testing.assert_array_equal(res.taps, ols5.fit(total, symmetric)[0])
    out = tmp_path / "kernels5.json"
    out.write_text(json.dumps({"mine": [0.0] * 24}))
    ols5.main(["--data", str(dataset), "--out", str(out)])
    ols5.main(["--data", str(dataset), "--symmetric", "--out", str(out)])
    text = capsys.readouterr().out
    assert "OLS5x5 taps" in text and "OLS5x5s residual mse" in text and "KB residual mse" in text
    saved = json.loads(out.read_text())
    assert list(saved) == ["mine", "OLS5x5", "OLS5x5s"]                                  # the file's other entry stays
    np.testing.assert_array_equal(saved["OLS5x5"], ols5.fit(total)[0])
    np.testing.assert_array_equal(saved["OLS5x5s"], ols5.fit(total, symmetric=True)[0])
    mse = [ols5.residual_mse(total, t, count) for t in (saved["OLS5x5"], saved["OLS5x5s"], ols5_np.kb_taps())]
    print(f"residual mse OLS5x5 {mse[0]:.6f} OLS5x5s {mse[1]:.6f} KB {mse[2]:.6f}")
    assert mse[0] <= mse[1] <= mse[2]
    # --kernels5 makes OLS5x5 a filter name of ws.estimate
    assert ols5.estimator("OLS5x5") is None
    estimate.main(["--data", str(dataset), "--kernels5", str(out), "--out", str(tmp_path / "ws.csv"), "--alphas", "1.0",
                   "--filters", "KB", "OLS5x5", "--losses"])
    ws = pd.read_csv(tmp_path / "ws.csv")
    assert ws["model_name"].unique().tolist() == ["KB", "OLS5x5"] and len(ws) == 2 * 10
    fixed = estimate._stat(_dev(np.stack([_plane(f"stego_LSBR_1.0_{k}.png") for k in (10, 6, 7, 8, 9)])),
                           ols5.Predictor5x5(saved["OLS5x5"]), AVG2D, 0, False).cpu().numpy()
    assert ols5.estimator("OLS5x5") is not None
    # (the table went through text: the float32 estimates to 1e-6)
    np.testing.assert_allclose(ws[(ws.model_name == "OLS5x5") & (ws.stego_method == "LSBR")]["beta_hat"].to_numpy(float), fixed, rtol=1e-6, atol=0)
