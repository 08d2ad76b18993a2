"""GPU: the recompression predictor 'JPEG' through the drivers (ws.estimate, ws.roc, ws.locate) and the data-set tool of ws.jpeg, on a
temporary data set: the five golden covers, their twins precompressed at quality 75 by `python -m ws_unet_amd.ws.jpeg --recompress 75
--write`, and LSBR alpha 0.4 twins of those made by embed."""
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import jpeg_np
from ws_unet_amd import embed, ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import estimate, jpeg, locate, roc

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
ORDER = (10, 6, 7, 8, 9)                                  # the iterators sort by name
STEGO = "stego_LSBR_alpha_0.4_independent_images"


def _plane(path):
    return np.ascontiguousarray(imread4_u8(path)[..., 3])


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    """(raw, twin): the golden covers as a data set, and the tool's precompressed twin of it with LSBR 0.4 stegos"""
    raw = tmp_path_factory.mktemp("jpeg_raw")
    (raw / "images").mkdir()
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", raw / "images" / f"{k}.png")
    (raw / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    twin = tmp_path_factory.mktemp("jpeg_twin")
    jpeg.main(["--data", str(raw), "--recompress", "75", "--write", str(twin)])
    folder, = embed.write_dataset(twin, "LSBR", 0.4)
    assert folder.name == STEGO
    return raw, twin


def test_the_tool_writes_the_history_and_the_twin(datasets):
    raw, twin = datasets
    hist = pd.read_csv(raw / "history.csv")
    assert hist["name"].tolist() == [f"images/{k}.png" for k in ORDER] and hist["q_hat"].tolist() == [0] * 5
    assert hist["energy_q_hat"].isna().all() and hist["energy_below"].isna().all() and (hist["energy_max_quality"] > 1.0).all()
    print(hist.to_string())
    files = pd.read_csv(twin / "images" / "files.csv")
    assert files.columns.tolist() == ["name", "height", "width"] and files["name"].tolist() == hist["name"].tolist()
    for k in COVERS:
        np.testing.assert_array_equal(_plane(twin / "images" / f"{k}.png"), jpeg_np.recompress(_plane(GOLDEN / f"cover_{k}.png")[None], 75)[0])
    again = jpeg.history(twin, take_num_images=2)
    assert len(again) == 2 and (abs(again["q_hat"] - 75) <= 2).all() and (again["energy_q_hat"] <= 1.0).all()
    assert (again["energy_below"] > 1.0).all()           # q_hat is the LOWEST quality that passes
    with pytest.raises(ValueError, match="together"):
        jpeg.history(twin, recompress=75)


@pytest.mark.parametrize("placement", ["random", "sequential"])
def test_rows_of_ws_estimate_batched_and_per_image(datasets, placement):
    _, twin = datasets
    placed = {} if placement == "random" else dict(placement="sequential", order="rows")
    for weighted in (0, 1):
        common = dict(correct_bias=False, weighted=weighted, **placed)
        resb = estimate.run(twin, "LSBR", 0.4, "JPEG", None, (3,), batched=True, **common)
        res = estimate.run(twin, "LSBR", 0.4, "JPEG", None, (3,), progress_on=False, **common)
        assert resb["name"].tolist() == [f"{STEGO}/{k}.png" for k in ORDER] == res["name"].tolist()
        assert resb["model_name"].tolist() == ["JPEG"] * 5 == res["model_name"].tolist()
        np.testing.assert_array_equal(resb["beta_hat"].to_numpy(np.float32), res["beta_hat"].to_numpy(np.float32))
        assert resb.columns.tolist() == res.columns.tolist() and ("placement" in resb.columns) == (placement == "sequential")
        # the rows are the statistic on the estimator's planes
        x = torch.from_numpy(np.stack([_plane(twin / STEGO / f"{k}.png") for k in ORDER])).to(DEV)
        want = estimate._stat(x, jpeg.JPEGEstimator(), estimate.NAMED_FILTERS["AVG"], weighted, False, **placed).cpu().numpy()
        np.testing.assert_array_equal(resb["beta_hat"].to_numpy(np.float32), want)
        print(f"{placement} weighted {weighted}: beta_hat {want.tolist()}")
        if placement == "random":
            assert np.abs(want - 0.2).max() <= 0.05
    if placement == "random":                            # the weights 5 + var, and the covers
        r = estimate.run(twin, "LSBR", 0.4, "JPEG", None, (3,), batched=True, correct_bias=False, weighted=-1)
        assert len(r) == 5 and np.isfinite(r["beta_hat"].to_numpy(np.float64)).all()
        cov = estimate.run(twin, None, None, "JPEG", None, (3,), batched=True, correct_bias=False, weighted=0)
        assert len(cov) == 5 and cov["model_name"].tolist() == ["JPEG"] * 5 and np.abs(cov["beta_hat"].to_numpy(np.float64)).max() <= 0.05


def test_correct_bias_raises(datasets):
    _, twin = datasets
    for batched in (True, False):
        with pytest.raises(ValueError, match="correct_bias"):
            estimate.run(twin, "LSBR", 0.4, "JPEG", None, (3,), batched=batched, correct_bias=True, weighted=0)
    x = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="correct_bias"):
        estimate.predictor_arguments(x, jpeg.JPEGEstimator(), correct_bias=True)


def test_raw_covers_fall_back_and_their_rows_are_kbs(datasets):
    raw, _ = datasets
    for weighted in (0, 1):
        for batched in (True, False):
            a = estimate.run(raw, None, None, "JPEG", None, (3,), batched=batched, correct_bias=False, weighted=weighted)
            b = estimate.run(raw, None, None, "KB", None, (3,), batched=batched, correct_bias=False, weighted=weighted)
            assert a["name"].tolist() == b["name"].tolist() and len(a) == 5 and a["model_name"].tolist() == ["JPEG"] * 5
            np.testing.assert_array_equal(a["beta_hat"].to_numpy(np.float32), b["beta_hat"].to_numpy(np.float32))
    x = torch.from_numpy(np.stack([_plane(raw / "images" / f"{k}.png") for k in COVERS])).to(DEV)
    est = jpeg.JPEGEstimator()
    estimate.predictor_arguments(x, est)
    assert est.fallbacks == 5
    none = estimate._stat(x, jpeg.JPEGEstimator(fallback=None), estimate.NAMED_FILTERS["AVG"], 0, False)
    assert torch.isnan(none).all()                       # no estimate: `run` drops such rows


@pytest.mark.parametrize("name", ["KB", "OLSa2", "OLSa5x5s", "JPEG"])
def test_the_three_drivers_resolve_a_name_to_one_predictor(datasets, name):
    """ws.estimate.run, ws.roc.collect_ws_scores and ws.locate.pixel_predictor's estimator (which ws.keysearch uses too) give the same
    bits for the same files: one name table (ws/predictors.py), one mapping to the kernels' arguments (`device_arguments`)"""
    _, twin = datasets
    run = estimate.run(twin, "LSBR", 0.4, name, None, (3,), weighted=0, correct_bias=False, batched=True)
    assert run["name"].tolist() == [f"{STEGO}/{k}.png" for k in ORDER] and run["model_name"].tolist() == [name] * 5
    beta = run["beta_hat"].to_numpy(np.float32)
    res = roc.collect_ws_scores(twin, ["LSBR"], [0.4], (name,))
    got = res[(res.model_name == name) & (res.stego_method == "LSBR")]
    assert got["name"].tolist() == run["name"].tolist()
    np.testing.assert_array_equal(got["beta_hat"].to_numpy(np.float32).view(np.uint32), beta.view(np.uint32))
    est, label = locate.pixel_predictor(name, None, (3,))
    assert label == name
    x = torch.from_numpy(np.stack([_plane(twin / STEGO / f"{k}.png") for k in ORDER])).to(DEV)
    stat = estimate._stat(x, est, estimate.NAMED_FILTERS["AVG"], 0, False).cpu().numpy()
    print(f"{name}: beta_hat {beta.tolist()}")
    assert stat.dtype == np.float32
    np.testing.assert_array_equal(stat.view(np.uint32), beta.view(np.uint32))


def test_filters_jpeg_kb_in_roc_and_locate(datasets, tmp_path):
    _, twin = datasets
    roc.main(["--data", str(twin), "--out-dir", str(tmp_path / "roc"), "--alphas", "0.4", "--filters", "JPEG", "KB"])
    auc = pd.read_csv(tmp_path / "roc" / "auc_0.4.csv")
    assert sorted(auc["model_name"]) == ["JPEG", "KB"] and auc["auc"].between(0., 1.).all()
    res = roc.collect_ws_scores(twin, ["LSBR"], [0.4], ("JPEG", "KB"))
    assert res["model_name"].unique().tolist() == ["JPEG", "KB"] and len(res) == 2 * 10
    run = estimate.run(twin, "LSBR", 0.4, "JPEG", None, (3,), correct_bias=False, weighted=0, batched=True)
    got = res[(res.model_name == "JPEG") & (res.stego_method == "LSBR")]
    assert got["name"].tolist() == run["name"].tolist()
    np.testing.assert_array_equal(got["beta_hat"].to_numpy(np.float32), run["beta_hat"].to_numpy(np.float32))
    labels = roc.produce_roc(res)[["model_name", "label"]].drop_duplicates()
    assert dict(zip(labels["model_name"], labels["label"])) == {"JPEG": "WS-JPEG", "KB": "WS-KB"}
    seq = roc.collect_ws_scores(twin, ["LSBR"], [0.4], ("JPEG",), placement="sequential")
    assert len(seq) == 10 and (seq["placement"] == "sequential").all()
    with pytest.raises(ValueError, match="unknown filter") as e:
        roc.collect_ws_scores(twin, ["LSBR"], [0.4], ("JPG",))
    assert "JPEG" in str(e.value)
    locate.main(["--data", str(twin), "--out-dir", str(tmp_path / "loc"), "--stego-method", "LSBR", "--alpha", "0.4", "--filters", "JPEG", "KB"])
    loc = pd.read_csv(tmp_path / "loc" / "locate.csv")
    assert loc["model_name"].tolist() == ["JPEG", "KB"] and loc["images"].tolist() == [5, 5]
    # the accumulator holds the sums of K29 on the estimator's planes
    x = torch.from_numpy(np.stack([_plane(twin / STEGO / f"{k}.png") for k in ORDER])).to(DEV)
    _, state = locate.run(twin, "LSBR", 0.4, "JPEG", None, (3,), return_state=True)
    num, den = torch.zeros_like(state.acc.num), torch.zeros_like(state.acc.den)
    ops.ws_residual_accumulate(x, num, den, jpeg.JPEGEstimator().planes(x), mean_filter=np.asarray(estimate.NAMED_FILTERS["AVG"])[..., ::-1],
                               hat_scale=1.0, weighted=1)
    assert torch.equal(state.acc.num, num) and torch.equal(state.acc.den, den)
