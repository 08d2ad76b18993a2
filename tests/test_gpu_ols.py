"""GPU: the moment kernel of the least-squares predictors (K24) bit for bit against numpy, the WS statistic with one filter per image
against the single-filter path, the adaptive estimator (OLSa) through the WS drivers, the data-set fit and its command line, and a
fitted filter as a column of the prediction-error table."""
import json
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import hill_np
import ols_np
from ws_unet_amd import error_boxes, filters, ols, ops, prediction_error
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import estimate

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
AVG2D, KB2D = filters.NAMED_FILTERS_2D["AVG"], filters.NAMED_FILTERS_2D["KB"]


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


def _moments(x: np.ndarray) -> np.ndarray:
    return ops.ols_moments(torch.from_numpy(x).to(DEV)).cpu().numpy()


@pytest.fixture(scope="module")
def cover_moments():
    """numpy moments (5,45) of the golden covers, computed once"""
    return np.stack([ols_np.moments(_plane(f"cover_{k}.png")) for k in COVERS])


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the five golden covers and their LSBR alpha 1.0 twins as a data set"""
    root = tmp_path_factory.mktemp("ols_data")
    (root / "images").mkdir()
    sdir = root / "stego_LSBR_alpha_1.0"
    sdir.mkdir()
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
        shutil.copy(GOLDEN / f"stego_LSBR_1.0_{k}.png", sdir / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    (sdir / "files.csv").write_text("name,height,width,stego_method,alpha\n" + "".join(
        f"stego_LSBR_alpha_1.0/{k}.png,512,512,LSBR,1.0\n" for k in COVERS))
    (root / "split_te.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    return root


@pytest.fixture
def registry():
    keep = dict(filters.NAMED_FILTERS), dict(filters.NAMED_FILTERS_2D)
    yield
    for table, saved in zip((filters.NAMED_FILTERS, filters.NAMED_FILTERS_2D), keep):
        table.clear()
        table.update(saved)


# ---- moments ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 3, 3), (3, 5, 7), (1, 16, 300), (2, 64, 64), (1, 67, 259), (2, 131, 40)])
def test_moments_equal_numpy_bit_for_bit(shape):
    """one interior pixel; a few; a row length that is no multiple of the 256-column tile (two column tiles, the second ragged); one
    tile; one pixel past a full tile in both directions (four tiles); three row tiles"""
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    got = _moments(x)
    assert got.dtype == np.int64 and got.shape == (shape[0], 45)
    np.testing.assert_array_equal(got, ols_np.moments(x))


@pytest.mark.parametrize("shape", [(1, 512, 512), (1, 66, 258)])
def test_moments_of_saturated_planes_do_not_overflow(shape):
    """all-255 planes: every product is 255 * 255.  (1,66,258) is exactly one full tile of 64 x 256 interior pixels, the most products a
    workgroup's 32-bit sums ever see (16 384 of the 66 051 they hold); 512 x 512 has full tiles too and the largest 64-bit totals."""
    count = (shape[1] - 2) * (shape[2] - 2)
    np.testing.assert_array_equal(_moments(np.full(shape, 255, dtype=np.uint8)), np.full((1, 45), 255 * 255 * count, dtype=np.int64))
    np.testing.assert_array_equal(_moments(np.zeros(shape, dtype=np.uint8)), np.zeros((1, 45), dtype=np.int64))


def test_moments_zero_their_output_and_are_deterministic():
    x = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (3, 70, 90), dtype=np.uint8)).to(DEV)
    lib = ops._lib.load()
    out = torch.full((3, 45), 12345, dtype=torch.int64, device=DEV)                # a dirty buffer, used twice
    for _ in range(2):
        ops.check(lib.wsu_ols_moments(x.data_ptr(), out.data_ptr(), 3, 70, 90, ops._stream()), "wsu_ols_moments")
        np.testing.assert_array_equal(out.cpu().numpy(), ols_np.moments(x.cpu().numpy()))
    assert torch.equal(ops.ols_moments(x), ops.ols_moments(x))


def test_moments_argument_errors():
    with pytest.raises(Exception, match="bad shape"):
        ops.ols_moments(torch.zeros((1, 2, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(Exception, match="bad shape"):
        ops.ols_moments(torch.zeros((1, 8, 2), dtype=torch.uint8, device=DEV))
    with pytest.raises(Exception, match="contiguous"):
        ops.ols_moments(torch.zeros((1, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2])
    with pytest.raises(Exception, match="CPU tensor"):
        ops.ols_moments(torch.zeros((1, 8, 8), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.ols_moments(torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV))
    lib = ops._lib.load()
    assert lib.wsu_ols_moments(None, None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()


# ---- the statistic with one filter per image --------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(8, 12), (64, 64)])
def test_per_image_filters_equal_single_filter_calls_bit_for_bit(hw):
    rng = np.random.default_rng(hw[0])
    x = torch.from_numpy(rng.integers(0, 256, (3,) + hw, dtype=np.uint8)).to(DEV)
    kernels = np.stack([KB2D, AVG2D, (rng.normal(size=(3, 3, 1)) / 3.).astype(np.float32)])
    for weighted in (-1, 0, 1):
        for correct_bias in (False, True):
            kw = dict(mean_filter=AVG2D, weighted=weighted, correct_bias=correct_bias, return_sums=True)
            beta, sums = ops.ws_attack(x, None, pixel_filter=kernels, **kw)
            assert beta.shape == (3,) and sums.shape == (3, 3)
            for i in range(3):
                b1, s1 = ops.ws_attack(x[i:i + 1], None, pixel_filter=kernels[i], **kw)
                assert torch.equal(beta[i:i + 1], b1) and torch.equal(sums[i:i + 1], s1), (hw, weighted, correct_bias, i)
    assert torch.equal(ops.ws_attack(x, None, pixel_filter=kernels[..., 0], weighted=0), ops.ws_attack(x, None, pixel_filter=kernels, weighted=0))
    with pytest.raises(ValueError, match="filters for"):
        ops.ws_attack(x, None, pixel_filter=kernels[:2], weighted=0)
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_attack(x, torch.zeros((3,) + hw, device=DEV), pixel_filter=kernels, weighted=0)


# ---- the adaptive estimator -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", ["1.0", "0.1"])
def test_adaptive_estimator_matches_the_float32_restatement(alpha):
    planes = np.stack([_plane(f"stego_LSBR_{alpha}_{k}.png") for k in COVERS])
    x = torch.from_numpy(planes).to(DEV)
    taps, ok = ols.fit(ols_np.moments(planes))
    assert ok.all()
    for weighted in (0, 1):
        est = ols.AdaptiveOLSEstimator()
        beta = estimate._stat(x, est, AVG2D, weighted, False).cpu().numpy()
        ref = np.array([ols_np.ws_beta(planes[i], taps[i], weighted) for i in range(len(planes))])
        print(f"alpha {alpha} weighted {weighted}: beta_hat {beta} restated {ref}")
        np.testing.assert_allclose(beta, ref, rtol=1e-6, atol=0)
        assert est.fallbacks == 0
        if alpha == "1.0" and weighted == 0:
            assert ((beta >= 0.45) & (beta <= 0.55)).all(), beta
    # the symmetric fit is another predictor; bias correction runs on the same taps
    sym = estimate._stat(x, ols.AdaptiveOLSEstimator(symmetric=True), AVG2D, 0, False).cpu().numpy()
    taps2, _ = ols.fit(ols_np.moments(planes), symmetric=True)
    np.testing.assert_allclose(sym, [ols_np.ws_beta(planes[i], taps2[i], 0) for i in range(len(planes))], rtol=1e-6, atol=0)
    k2d = np.stack([filters.kernel_2d(t) for t in taps])
    assert torch.equal(estimate._stat(x, ols.AdaptiveOLSEstimator(), AVG2D, 1, True),
                       ops.ws_attack(x, None, pixel_filter=k2d, mean_filter=AVG2D, weighted=1, correct_bias=True))


def test_adaptive_estimator_falls_back_to_kb_on_a_flat_image(caplog):
    x = torch.from_numpy(np.stack([np.full((16, 16), 9, dtype=np.uint8), np.random.default_rng(4).integers(0, 256, (16, 16), dtype=np.uint8)])).to(DEV)
    est = ols.AdaptiveOLSEstimator()
    kernels = est.kernels(x)
    est.kernels(x)
    np.testing.assert_array_equal(kernels[0], KB2D)
    assert not np.array_equal(kernels[1], KB2D) and est.fallbacks == 2
    assert sum("OLS fit" in r.getMessage() for r in caplog.records) == 1               # logged once, not per image
    host = est(x[1].cpu().numpy().astype(np.float32)[..., None])                       # called like the reference's estimators
    np.testing.assert_array_equal(host, filters.infere_single(x[1].cpu().numpy().astype(np.float32)[..., None], kernels[1]))


def test_adaptive_estimator_through_the_ws_drivers(dataset):
    fnames = [dataset / "stego_LSBR_alpha_1.0" / f"{k}.png" for k in COVERS]
    planes = np.stack([_plane(f"stego_LSBR_1.0_{k}.png") for k in COVERS])
    direct = estimate._stat(torch.from_numpy(planes).to(DEV), ols.AdaptiveOLSEstimator(), AVG2D, 1, True).cpu().numpy()
    rows = estimate.attack_batch(fnames, [{"name": f.name} for f in fnames], channels=(3,), pixel_estimator=ols.AdaptiveOLSEstimator(),
                                 correct_bias=True, weighted=1)
    np.testing.assert_array_equal([r["beta_hat"] for r in rows], direct)
    assert rows[0]["name"] == "6.png" and rows[0]["weighted"] == 1 and rows[0]["correct_bias"] is True
    for model_name in ("OLSa", "OLSa2"):
        resb = estimate.run(dataset, "LSBR", 1.0, model_name, None, (3,), correct_bias=False, weighted=0, batched=True, batch_size=2)
        res = estimate.run(dataset, "LSBR", 1.0, model_name, None, (3,), correct_bias=False, weighted=0, progress_on=False)
        assert resb["name"].tolist() == [f"stego_LSBR_alpha_1.0/{k}.png" for k in (10, 6, 7, 8, 9)] == res["name"].tolist()
        assert resb["model_name"].tolist() == [model_name] * 5
        np.testing.assert_allclose(resb["beta_hat"].to_numpy(float), res["beta_hat"].to_numpy(float), rtol=1e-6, atol=0)
        if model_name == "OLSa":
            assert resb["beta_hat"].between(0.45, 0.55).all()
    cov = estimate.run(dataset, None, None, "OLSa", None, (3,), correct_bias=False, weighted=0, batched=True)
    assert len(cov) == 5 and cov["model_name"].tolist() == ["OLSa"] * 5 and (cov["beta_hat"] >= 0).all()


def test_olsa_is_a_row_of_the_roc_scores(dataset):
    from ws_unet_amd.ws import roc
    res = roc.collect_ws_scores(dataset, ["LSBR"], [1.0], ["KB", "OLSa"])
    assert res["model_name"].unique().tolist() == ["KB", "OLSa"] and len(res) == 2 * 10
    run = estimate.run(dataset, "LSBR", 1.0, "OLSa", None, (3,), correct_bias=False, weighted=0, batched=True)
    got = res[(res.model_name == "OLSa") & (res.stego_method == "LSBR")]
    assert got["name"].tolist() == run["name"].tolist()
    np.testing.assert_array_equal(got["beta_hat"].to_numpy(np.float32), run["beta_hat"].to_numpy(np.float32))
    with pytest.raises(ValueError, match="unknown filter"):
        roc.collect_ws_scores(dataset, ["LSBR"], [1.0], ["OLS"])


# ---- one fit for the data set, and the fitted filter in a table ------------------------------------------------------------------------

def test_fit_dataset_and_command_line(dataset, cover_moments, tmp_path, capsys):
    total = cover_moments.sum(axis=0)
    for symmetric in (False, True):
        res = ols.fit_dataset(dataset, symmetric=symmetric, batch_size=2)                 # three chunks, the last of one image
        assert res.moments.dtype == np.int64 and res.count == 5 * 510 * 510 and res.ok
        np.testing.assert_array_equal(res.moments, total)
        if not symmetric:
            np.testing.assert_allclose(res.taps, ols_np.solve(total), rtol=0, atol=1e-12)
    first = ols.fit_dataset(dataset, take_num_images=2)                                   # fabrika's order: 10, 6
    np.testing.assert_array_equal(first.moments, cover_moments[[4, 0]].sum(axis=0))
    out = tmp_path / "kernels.json"
    ols.main(["--data", str(dataset), "--out", str(out)])
    ols.main(["--data", str(dataset), "--symmetric", "--out", str(out)])
    text = capsys.readouterr().out
    assert "OLS taps" in text and "KB residual mse" in text
    saved = json.loads(out.read_text())
    assert list(saved) == ["OLS", "OLS2"]
    np.testing.assert_array_equal(saved["OLS"], ols.fit(total)[0])
    np.testing.assert_array_equal(saved["OLS2"], ols.fit(total, symmetric=True)[0])
    assert ols.residual_mse(total, saved["OLS"], 5 * 510 * 510) <= ols.residual_mse(total, saved["OLS2"], 5 * 510 * 510) \
        <= ols.residual_mse(total, filters.NAMED_FILTERS["KB"], 5 * 510 * 510)


def test_prediction_error_table_with_the_fitted_filter(dataset, cover_moments, tmp_path, registry):
    import pandas as pd
    taps = ols.fit(cover_moments.sum(axis=0))[0]
    kernels = tmp_path / "kernels.json"
    ols.save_kernels(kernels, {"OLS": taps})
    prediction_error.main(["--data", str(dataset), "--out", str(tmp_path / "plain.csv")])
    prediction_error.main(["--data", str(dataset), "--out", str(tmp_path / "ols.csv"), "--kernels", str(kernels),
                           "--filters", "AVG", "KB", "OLS"])
    plain_lines, lines = (tmp_path / "plain.csv").read_text().splitlines(), (tmp_path / "ols.csv").read_text().splitlines()
    assert len(plain_lines) == 1 + 10 and len(lines) == 1 + 15
    assert lines[0] == plain_lines[0] + ",mae_3_OLS,wmae_3_OLS"
    assert lines[1:11] == [ln + ",," for ln in plain_lines[1:]]                          # the AVG and KB rows, character for character
    table = pd.read_csv(tmp_path / "ols.csv")
    rows = table[~table["mae_3_OLS"].isna()]
    assert rows["name"].tolist() == [f"images/{k}.png" for k in (10, 6, 7, 8, 9)]
    for _, row in rows.iterrows():
        x = _plane(f"cover_{row['name'].split('/')[1].split('.')[0]}.png")
        cost = ops.hill_cost(torch.from_numpy(x)[None].to(DEV))[0].cpu().numpy().astype(np.float64)[1:-1, 1:-1]
        r = np.abs(x[1:-1, 1:-1].astype(np.float64) - hill_np.filter_hat(x, taps))
        assert abs(row["mae_3_OLS"] - r.mean()) <= 1e-12 * r.mean()
        assert abs(row["wmae_3_OLS"] - hill_np.wmae(r, cost)[0]) <= 1e-6 * hill_np.wmae(r, cost)[0]


def test_fitted_and_adaptive_filters_in_the_other_four_drivers(dataset, cover_moments, tmp_path, registry):
    """--kernels registers the file's names; OLS becomes a column / row of each table and the AVG / KB entries stay what they are"""
    import pandas as pd
    from ws_unet_amd import correlation
    from ws_unet_amd.ws import roc
    kernels = tmp_path / "kernels.json"
    ols.save_kernels(kernels, {"OLS": ols.fit(cover_moments.sum(axis=0))[0]})
    data, k = ["--data", str(dataset)], ["--kernels", str(kernels)]
    # correlation: one column per model
    sel = ["--stego-method", "LSBR", "--alpha", "1.0"]
    correlation.main(data + sel + ["--out", str(tmp_path / "c0.csv"), "--filters", "AVG", "KB"])
    correlation.main(data + sel + k + ["--out", str(tmp_path / "c1.csv"), "--filters", "AVG", "KB", "OLS"])
    c0, c1 = pd.read_csv(tmp_path / "c0.csv", index_col=0), pd.read_csv(tmp_path / "c1.csv", index_col=0)
    assert list(c1.columns) == ["AVG", "KB", "OLS"] and c1[["AVG", "KB"]].equals(c0) and c1["OLS"].notna().all()
    # error boxes: rows per predictor and KB slice
    error_boxes.main(data + ["--out", str(tmp_path / "b0.csv")])
    error_boxes.main(data + k + ["--out", str(tmp_path / "b1.csv"), "--filters", "KB", "AVG", "OLS"])
    b0, b1 = (pd.read_csv(tmp_path / f, float_precision="round_trip") for f in ("b0.csv", "b1.csv"))
    assert sorted(b1["Type"].unique()) == ["AVG", "KB", "OLS"]
    # the OLS rows: float64 AE rounded to float32 (monotone, so every order statistic is the rounded exact one; a float64 sum order
    # other than numpy's moves a float32 rounding by one unit at the most: rtol 2^-23, atol 9 terms * 510 * 2^-53 = 5e-13 -> 1e-12)
    import boxes_np
    names = pd.DataFrame({"name": sorted(f"images/{c}.png" for c in COVERS)}).sample(frac=1., random_state=12345)["name"]
    planes = [_plane(f"cover_{n.split('/')[1].split('.')[0]}.png") for n in names]
    ae = lambda taps: np.stack([np.abs(p[1:-1, 1:-1].astype(np.float64) - hill_np.filter_hat(p, taps)) for p in planes])
    want = boxes_np.table_numpy({"KB": ae(filters.NAMED_FILTERS["KB"]),
                                 "OLS": ae(filters.NAMED_FILTERS["OLS"]).astype(np.float32).astype(np.float64)}, "KB")
    stats = list(error_boxes.STATS)
    for t in ("KB", "OLS"):
        g, w = (d[d["Type"] == t].sort_values("edge_interval") for d in (b1, want))
        assert g["edge_interval"].tolist() == w["edge_interval"].tolist()
        np.testing.assert_allclose(g[stats].to_numpy(float), w[stats].to_numpy(float), rtol=2.0 ** -23 if t == "OLS" else 0, atol=1e-12 if t == "OLS" else 0)
    with pytest.raises(ValueError, match="anchor"):
        error_boxes.run(dataset, {"KB": "OLS", "AVG": "AVG"}, anchor="KB")
    order = ["Type", "edge_interval"]
    assert b1[b1["Type"] != "OLS"].sort_values(order).reset_index(drop=True).equals(b0.sort_values(order).reset_index(drop=True))
    # ROC / AUC: the fitted and the adaptive filter beside AVG and KB
    roc.main(data + k + ["--out-dir", str(tmp_path / "roc"), "--alphas", "1.0", "--filters", "AVG", "KB", "OLS", "OLSa"])
    auc = pd.read_csv(tmp_path / "roc" / "auc_1.0.csv")
    assert sorted(auc["model_name"]) == ["AVG", "KB", "OLS", "OLSa"] and auc["auc"].between(0.5, 1.0).all()
    # WS estimates
    estimate.main(data + k + ["--out", str(tmp_path / "ws.csv"), "--alphas", "1.0", "--filters", "AVG", "KB", "OLS", "OLSa", "--losses"])
    ws = pd.read_csv(tmp_path / "ws.csv")
    assert ws["model_name"].unique().tolist() == ["AVG", "KB", "OLS", "OLSa"] and len(ws) == 4 * 10
    assert ws[(ws.model_name == "OLSa") & (ws.stego_method == "LSBR")]["beta_hat"].between(0.45, 0.55).all()
