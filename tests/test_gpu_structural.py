"""GPU: the sample-pairs table (K25) and the RS group counts (K26) bit for bit against numpy (structural_np), the device solve of
StructuralEstimator against the restated estimates, and 'SPA' / 'RS' as rows of the WS drivers and curves of the ROC tables."""
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import structural_np
from ws_unet_amd import ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import estimate, roc, structural

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


def _tables(x: np.ndarray) -> np.ndarray:
    return ops.spa_tables(torch.from_numpy(x).to(DEV)).cpu().numpy()


def _counts(x: np.ndarray) -> np.ndarray:
    return ops.rs_counts(torch.from_numpy(x).to(DEV)).cpu().numpy()


def _patterns(shape):
    n, h, w = shape
    rr, cc = np.indices((h, w))
    return {"constant": np.full(shape, 77, dtype=np.uint8), "all 255": np.full(shape, 255, dtype=np.uint8), "all 0": np.zeros(shape, dtype=np.uint8),
            "checkerboard": np.broadcast_to(((rr + cc) % 2 * 255).astype(np.uint8), shape).copy(),
            "columns 2k / 2k+1": np.broadcast_to((2 * (rr % 128) + cc % 2).astype(np.uint8), shape).copy()}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the five golden covers and their LSBR alpha 0.1 twins as a data set"""
    root = tmp_path_factory.mktemp("structural_data")
    (root / "images").mkdir()
    sdir = root / "stego_LSBR_alpha_0.1"
    sdir.mkdir()
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
        shutil.copy(GOLDEN / f"stego_LSBR_0.1_{k}.png", sdir / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    (sdir / "files.csv").write_text("name,height,width,stego_method,alpha\n" + "".join(
        f"stego_LSBR_alpha_0.1/{k}.png,512,512,LSBR,0.1\n" for k in COVERS))
    (root / "split_te.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    return root


# ---- K25 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 2), (1, 2, 1), (1, 1, 1), (2, 3, 5), (1, 16, 300), (1, 67, 259), (2, 131, 40)])
def test_spa_tables_equal_numpy_bit_for_bit(shape):
    """one pair (horizontal, vertical); no pair; a few; a ragged last strip; an odd width (every second row off the 16-byte grid), rows
    one past two row tiles; five row tiles, the last of three rows"""
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    got = _tables(x)
    assert got.dtype == np.int64 and got.shape == (shape[0], 3, 128)
    np.testing.assert_array_equal(got, structural_np.spa_table(x))
    n, h, w = shape
    assert (got.sum(axis=(1, 2)) == h * (w - 1) + (h - 1) * w).all()


@pytest.mark.parametrize("shape", [(1, 512, 512), (1, 66, 258)])
def test_spa_tables_of_value_patterns(shape):
    """a constant 512 x 512 plane puts all 523 264 pairs into E[0]; all 255; a 0 / 255 checkerboard (every pair in Y[127]); columns
    alternating 2k / 2k+1 with k the row (horizontal pairs d = 1 with an odd maximum, vertical pairs d = 2)"""
    for name, x in _patterns(shape).items():
        got = _tables(x)
        np.testing.assert_array_equal(got, structural_np.spa_table(x), err_msg=name)
    n, h, w = shape
    assert _tables(np.full(shape, 77, dtype=np.uint8))[0, 0, 0] == h * (w - 1) + (h - 1) * w


def test_spa_tables_of_natural_images():
    x = np.stack([_plane("cover_6.png"), _plane("stego_LSBR_1.0_7.png")])
    np.testing.assert_array_equal(_tables(x), structural_np.spa_table(x))


# ---- K26 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 4), (1, 3, 3), (2, 5, 7), (1, 16, 300), (1, 67, 259), (2, 131, 42)])
def test_rs_counts_equal_numpy_bit_for_bit(shape):
    """one group; w < 4: none; three ignored tail columns; a ragged last strip; an odd width over three row tiles; w % 4 == 2"""
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    got = _counts(x)
    assert got.dtype == np.int64 and got.shape == (shape[0], 8)
    np.testing.assert_array_equal(got, structural_np.rs_counts(x))
    if shape[2] < 4:
        assert not got.any()


def test_rs_counts_where_the_negative_flip_leaves_the_byte_range():
    for shape in ((1, 66, 258), (1, 512, 512)):
        for name, x in _patterns(shape).items():
            np.testing.assert_array_equal(_counts(x), structural_np.rs_counts(x), err_msg=f"{shape} {name}")
    x = np.stack([_plane("cover_9.png"), _plane("stego_LSBR_0.05_10.png")])
    np.testing.assert_array_equal(_counts(x), structural_np.rs_counts(x))


# ---- both entry points ----------------------------------------------------------------------------------------------------------------

def test_outputs_are_zeroed_by_the_call_and_repeat_bit_for_bit():
    xn = np.random.default_rng(3).integers(0, 256, (3, 70, 90), dtype=np.uint8)
    x = torch.from_numpy(xn).to(DEV)
    lib = ops._lib.load()
    tables = torch.ones((3, 3, 128), dtype=torch.int64, device=DEV)                # dirty buffers, used twice
    counts = torch.ones((3, 8), dtype=torch.int64, device=DEV)
    for _ in range(2):
        ops.check(lib.wsu_spa_tables(x.data_ptr(), tables.data_ptr(), 3, 70, 90, ops._stream()), "wsu_spa_tables")
        ops.check(lib.wsu_rs_counts(x.data_ptr(), counts.data_ptr(), 3, 70, 90, ops._stream()), "wsu_rs_counts")
        np.testing.assert_array_equal(tables.cpu().numpy(), structural_np.spa_table(xn))
        np.testing.assert_array_equal(counts.cpu().numpy(), structural_np.rs_counts(xn))
    assert torch.equal(ops.spa_tables(x), ops.spa_tables(x)) and torch.equal(ops.rs_counts(x), ops.rs_counts(x))


def test_argument_errors():
    lib = ops._lib.load()
    for fn, entry in ((ops.spa_tables, lib.wsu_spa_tables), (ops.rs_counts, lib.wsu_rs_counts)):
        with pytest.raises(ValueError, match="no images"):
            fn(torch.zeros((0, 8, 8), dtype=torch.uint8, device=DEV))
        with pytest.raises(Exception, match="contiguous"):
            fn(torch.zeros((1, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2])
        with pytest.raises(Exception, match="CPU tensor"):
            fn(torch.zeros((1, 8, 8), dtype=torch.uint8))
        with pytest.raises(ValueError):
            fn(torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV))
        assert entry(None, None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
        assert entry(1, 1, 1, 0, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
        assert entry(1, 1, 0, 8, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()


# ---- the estimator ------------------------------------------------------------------------------------------------------------------

def test_estimator_on_the_device_batch_equals_the_restated_estimates():
    planes = np.stack([_plane(f"cover_{k}.png") for k in COVERS] + [_plane(f"stego_LSBR_0.05_{k}.png") for k in COVERS])
    x = torch.from_numpy(planes).to(DEV)
    tables, counts = structural_np.spa_table(planes), structural_np.rs_counts(planes)
    for est, want in ((structural.StructuralEstimator("SPA"), [structural_np.spa_p(t, 30) / 2 for t in tables]),
                      (structural.StructuralEstimator("SPA", j=127), [structural_np.spa_p(t, 127) / 2 for t in tables]),
                      (structural.StructuralEstimator("RS"), [structural_np.rs_p(c) / 2 for c in counts])):
        beta = est.beta(x)
        assert beta.is_cuda and beta.dtype == torch.float64 and beta.shape == (10,)
        got = beta.cpu().numpy()
        print(f"{est.name}{f' j={est.j}' if est.name == 'SPA' else ''}: beta_hat {got}")
        assert np.isfinite(want).all() and np.abs(got - np.asarray(want)).max() <= 1e-9
    # a plane without an answer (a 0 / 255 checkerboard: every pair in Y[127]) is NaN in its own row only
    x2 = torch.cat([x[:1], torch.from_numpy(_patterns((1, 512, 512))["checkerboard"]).to(DEV)])
    got = structural.StructuralEstimator("SPA").beta(x2).cpu().numpy()
    assert np.isfinite(got[0]) and np.isnan(got[1])


# ---- the drivers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model_name", structural.NAMES)
def test_structural_rows_of_ws_estimate(dataset, model_name):
    planes = {k: _plane(f"stego_LSBR_0.1_{k}.png") for k in COVERS}
    p = structural_np.spa_p if model_name == "SPA" else structural_np.rs_p
    table = structural_np.spa_table if model_name == "SPA" else structural_np.rs_counts
    resb = estimate.run(dataset, "LSBR", 0.1, model_name, None, (3,), correct_bias=False, weighted=0, batched=True, batch_size=2)
    res = estimate.run(dataset, "LSBR", 0.1, model_name, None, (3,), correct_bias=False, weighted=0, progress_on=False)
    assert resb["name"].tolist() == [f"stego_LSBR_alpha_0.1/{k}.png" for k in (10, 6, 7, 8, 9)] == res["name"].tolist()
    assert resb["model_name"].tolist() == [model_name] * 5 == res["model_name"].tolist()
    np.testing.assert_array_equal(resb["beta_hat"].to_numpy(np.float32), res["beta_hat"].to_numpy(np.float32))
    want = np.array([p(table(planes[k])) / 2 for k in (10, 6, 7, 8, 9)])
    # the rows hold float32: the solve's 1e-9 and half a float32 step of a value below 1/8
    assert np.abs(resb["beta_hat"].to_numpy(np.float64) - want).max() <= 1e-9 + 2.0 ** -28
    assert (resb["weighted"] == 0).all() and not resb["correct_bias"].any()
    cov = estimate.run(dataset, None, None, model_name, None, (3,), correct_bias=False, weighted=0, batched=True)
    assert len(cov) == 5 and cov["model_name"].tolist() == [model_name] * 5
    with pytest.raises(ValueError, match="weighted=0"):
        estimate.run(dataset, "LSBR", 0.1, model_name, None, (3,), correct_bias=False, weighted=1, batched=True)
    with pytest.raises(ValueError, match="weighted=0"):
        estimate.run(dataset, "LSBR", 0.1, model_name, None, (3,), correct_bias=True, weighted=0)
    x = torch.from_numpy(planes[6])[None].to(DEV)
    with pytest.raises(ValueError, match="weighted=0"):
        estimate._stat(x, structural.StructuralEstimator(model_name), estimate.NAMED_FILTERS["AVG"], 1, False)


def test_structural_curves_of_the_roc_tables(dataset):
    res = roc.collect_ws_scores(dataset, ["LSBR"], [0.1], ("AVG", "SPA", "RS"))
    assert res["model_name"].unique().tolist() == ["AVG", "SPA", "RS"] and len(res) == 3 * 10
    for name in structural.NAMES:
        run = estimate.run(dataset, "LSBR", 0.1, name, None, (3,), correct_bias=False, weighted=0, batched=True)
        got = res[(res.model_name == name) & (res.stego_method == "LSBR")]
        assert got["name"].tolist() == run["name"].tolist()
        np.testing.assert_array_equal(got["beta_hat"].to_numpy(np.float32), run["beta_hat"].to_numpy(np.float32))
    df = roc.produce_roc(res)
    labels = df[["model_name", "label"]].drop_duplicates()
    assert dict(zip(labels["model_name"], labels["label"])) == {"AVG": "WS-AVG", "SPA": "SPA", "RS": "RS"}
    alone = roc.produce_roc(roc.collect_ws_scores(dataset, ["LSBR"], [0.1], ("AVG",)))
    assert df[df.model_name == "AVG"].reset_index(drop=True).equals(alone.reset_index(drop=True))
    auc = roc.auc_table(df)
    assert sorted(auc["model_name"]) == ["AVG", "RS", "SPA"] and auc["auc"].between(0., 1.).all()
    with pytest.raises(ValueError, match="unknown filter") as e:
        roc.collect_ws_scores(dataset, ["LSBR"], [0.1], ("AVG", "SPAM"))
    assert "SPA" in str(e.value) and "RS" in str(e.value)
