"""GPU: the SPAM counts (K36, ops.spam_counts) bit for bit against numpy (spam_np) in every case, their totals, batch and output
handling; the features and the Fisher discriminant on device counts against the restatement on crops of the golden covers; the drivers
(`fit`, `score`, `--simulate`) and the detector's row in the ROC tables."""
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import spam_np
from ws_unet_amd import embed, ops, spam
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import roc

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
CONFIGS = [(2, 3), (1, 4), (2, 1), (2, 4), (1, 8)]                          # (order, T)
TILE_ROWS, TILE_COLS = 32, 512                                              # K36's tile (csrc/wsu_count.h CT_ROWS, CT_COLS)
SHAPES = [(1, 1, 1), (1, 1, 4), (1, 4, 1), (1, 4, 4), (2, 3, 5), (1, 16, 300), (1, 67, 259), (2, 131, 40), (1, TILE_ROWS + 1, TILE_COLS + 1)]


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


def _counts(x: np.ndarray, order, T, **kw) -> np.ndarray:
    return ops.spam_counts(torch.from_numpy(x).to(DEV), order, T, **kw).cpu().numpy()


def _totals(shape, order):
    n, h, w = shape
    k = order + 1
    return [h * max(w - k, 0), max(h - k, 0) * w, max(h - k, 0) * max(w - k, 0), max(h - k, 0) * max(w - k, 0)]


def _patterns(shape):
    n, h, w = shape
    rr, cc = np.indices((h, w))
    return {"constant": np.full(shape, 77, dtype=np.uint8), "all 0": np.zeros(shape, dtype=np.uint8), "all 255": np.full(shape, 255, dtype=np.uint8),
            "checkerboard": np.broadcast_to(((rr + cc) % 2 * 255).astype(np.uint8), shape).copy(),
            "horizontal ramp": np.broadcast_to((cc % 256).astype(np.uint8), shape).copy()}


# ---- K36 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order,T", CONFIGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_counts_equal_numpy_bit_for_bit(shape, order, T):
    """no run at all; one run per direction or none (w = 4 and h = 4 hold exactly one run at order 2, two at order 1); a few; a ragged last
    strip; an odd width with rows off the 16-byte grid over three row tiles; five row tiles, the last of three rows; one row and one
    column past the tile (a second tile in both directions whose only positions have no complete run)"""
    x = np.random.default_rng(sum(shape) + 7 * order + T).integers(0, 256, shape, dtype=np.uint8)
    if shape[1] * shape[2] >= 64:
        x[:, : shape[1] // 2, : shape[2] // 3] //= 64                       # a smooth corner: small differences, the centre bin among them
    got = _counts(x, order, T)
    assert got.dtype == np.int64 and got.shape == (shape[0], 4, spam_np.bins(order, T))
    np.testing.assert_array_equal(got, spam_np.counts(x, order, T))
    assert (got.sum(axis=2) == np.array(_totals(shape, order))).all()


@pytest.mark.parametrize("order,T", CONFIGS)
@pytest.mark.parametrize("shape", [(1, 66, 258), (1, 512, 512)])
def test_counts_of_value_patterns(shape, order, T):
    """a constant plane puts every run into the centre bin (the register path, nothing else); a 0 / 255 checkerboard clips every axis
    difference to +-T and leaves every diagonal one 0; a ramp has one horizontal difference, -1, and the wrap 255 -> 0"""
    nb = spam_np.bins(order, T)
    for name, x in _patterns(shape).items():
        got = _counts(x, order, T)
        np.testing.assert_array_equal(got, spam_np.counts(x, order, T), err_msg=name)
        if name in ("constant", "all 0", "all 255"):
            assert got[0, :, nb // 2].tolist() == _totals(shape, order) and got.sum() == sum(_totals(shape, order)), name
        if name == "checkerboard":
            assert got[0, 2:, nb // 2].tolist() == _totals(shape, order)[2:] and not got[0, :2, nb // 2].any()
            assert np.count_nonzero(got[0, 0]) == 2 == np.count_nonzero(got[0, 1])


def test_counts_of_natural_images():
    x = np.stack([_plane("cover_6.png"), _plane("stego_LSBR_1.0_7.png")])
    for order, T in ((2, 3), (1, 4)):
        np.testing.assert_array_equal(_counts(x, order, T), spam_np.counts(x, order, T))


def test_batch_output_and_repeat():
    xn = np.random.default_rng(3).integers(0, 256, (3, 70, 90), dtype=np.uint8)
    xn[1] //= 32
    x = torch.from_numpy(xn).to(DEV)
    want = spam_np.counts(xn)
    got = ops.spam_counts(x)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    for i in range(3):                                                       # a batch is its images one by one
        assert torch.equal(ops.spam_counts(x[i:i + 1])[0], got[i])
    out = torch.full((3, 4, 343), 7, dtype=torch.int64, device=DEV)          # a dirty buffer, used twice: the entry point zeroes it
    for _ in range(2):
        assert ops.spam_counts(x, out=out) is out
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert torch.equal(ops.spam_counts(x), ops.spam_counts(x))
    lib = ops._lib.load()
    raw = torch.full((3, 4, 81), 7, dtype=torch.int64, device=DEV)
    ops.check(lib.wsu_spam_counts(x.data_ptr(), raw.data_ptr(), 3, 70, 90, 1, 4, ops._stream()), "wsu_spam_counts")
    np.testing.assert_array_equal(raw.cpu().numpy(), spam_np.counts(xn, 1, 4))


def test_argument_errors():
    with pytest.raises(ValueError, match="no images"):
        ops.spam_counts(torch.zeros((0, 8, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(Exception, match="contiguous"):
        ops.spam_counts(torch.zeros((1, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2])
    with pytest.raises(ValueError):
        ops.spam_counts(torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV))
    x = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    for order, T in ((3, 1), (2, 5), (1, 9), (2, 0)):
        with pytest.raises(ValueError, match="order"):
            ops.spam_counts(x, order, T)
    for out in (torch.zeros((1, 4, 81), dtype=torch.int64, device=DEV), torch.zeros((1, 4, 343), dtype=torch.int32, device=DEV),
                torch.zeros((2, 4, 343), dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match="out must be"):
            ops.spam_counts(x, out=out)
    lib = ops._lib.load()
    assert lib.wsu_spam_counts(x.data_ptr(), None, 1, 8, 8, 2, 3, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_spam_counts(x.data_ptr(), x.data_ptr(), 1, 8, 8, 2, 5, None) == -1 and b"T=5" in lib.wsu_last_error()
    with pytest.raises(ValueError, match="image 0"):                         # three rows: no vertical run of four pixels
        spam.features(ops.spam_counts(torch.zeros((1, 3, 9), dtype=torch.uint8, device=DEV)))


# ---- the detector on crops of the golden covers --------------------------------------------------------------------------------------

def _crops(ks):
    return np.stack([p[r:r + 64, c:c + 64] for p in (_plane(f"cover_{k}.png") for k in ks) for r in range(0, 512, 64) for c in range(0, 512, 64)])


@pytest.fixture(scope="module")
def crop_sets():
    """64 x 64 crops of covers 6-8 (192, training) and of covers 9-10 (128, held out) with their full-payload LSBR twins made on the device:
    (cover, stego) planes on the host, per set"""
    sets = []
    for ks, seed0 in (((6, 7, 8), 1000), ((9, 10), 5000)):
        cover = _crops(ks)
        stego, changes = embed.simulate(torch.from_numpy(cover).to(DEV), "LSBR", 1.0, [seed0 + i for i in range(len(cover))])
        assert (changes > 1500).all()                                        # about half of 4096 pixels each
        sets.append((cover, stego.cpu().numpy()))
    assert len(sets[0][0]) == 192 and len(sets[1][0]) == 128
    return sets


@pytest.mark.parametrize("order,T,normalise", [(2, 3, "joint"), (1, 4, "transition")])
def test_device_features_equal_the_restated_ones(crop_sets, order, T, normalise):
    for cover, stego in crop_sets:
        for x in (cover, stego):
            got = spam.features(ops.spam_counts(torch.from_numpy(x).to(DEV), order, T), order, T, normalise)
            np.testing.assert_array_equal(got, spam_np.features(spam_np.counts(x, order, T), order, T, normalise))


def test_detector_on_crops_equals_the_restatement_and_detects(crop_sets):
    """FLD(ridge 0.1) on SPAM-686 of 192 crops and their twins, scored on 128 held-out crops and theirs.  The device features are the
    restated ones exactly, so outputs and AUC agree to 1e-12.  The restatement's own AUC must be >= 0.8: a condition on the inputs (numpy
    with a numpy-random embedding of the same crops reached 0.925 at ridge 0.1, 0.811 at 1e-3; with these Philox twins 0.933)."""
    dev = lambda x: spam.features(ops.spam_counts(torch.from_numpy(x).to(DEV)))
    ref = lambda x: spam_np.features(spam_np.counts(x))
    (c_tr, s_tr), (c_te, s_te) = crop_sets
    model = spam.FLD(ridge=0.1).fit(dev(c_tr), dev(s_tr))
    w, b = spam_np.fld_fit(ref(c_tr), ref(s_tr), 0.1)
    got0, got1 = model.output(dev(c_te)), model.output(dev(s_te))
    want0, want1 = spam_np.fld_output(ref(c_te), w, b), spam_np.fld_output(ref(s_te), w, b)
    auc_got, auc_want = spam_np.auc(got0, got1), spam_np.auc(want0, want1)
    print(f"held-out AUC: device {auc_got:.6f}, restatement {auc_want:.6f}; max |output difference| {max(np.abs(got0 - want0).max(), np.abs(got1 - want1).max()):.3e}")
    assert auc_want >= 0.8
    assert np.abs(got0 - want0).max() <= 1e-12 and np.abs(got1 - want1).max() <= 1e-12
    assert abs(auc_got - auc_want) <= 1e-12
    assert ((got0 >= 0) & (got0 <= 1)).all() and ((got1 >= 0) & (got1 <= 1)).all()


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the five golden covers and their LSBR alpha 0.1 twins as a data set"""
    root = tmp_path_factory.mktemp("spam_data")
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


ORDER = (10, 6, 7, 8, 9)                                                    # fabrika sorts names lexically


def test_extract_covers_stegos_and_simulated_twins(dataset):
    rows, F = spam.extract(dataset)
    assert rows["name"].tolist() == [f"images/{k}.png" for k in ORDER] and rows["stego_method"].isna().all() and rows["alpha"].isna().all()
    covers = np.stack([_plane(f"cover_{k}.png") for k in ORDER])
    np.testing.assert_array_equal(F, spam_np.features(spam_np.counts(covers)))
    rows2, F2 = spam.extract(dataset, split="split_te.csv", batch_size=2)    # chunks of 2, 2, 1
    assert rows2.equals(rows) and np.array_equal(F2, F)
    rows, F = spam.extract(dataset, "LSBR", 0.1, order=1, T=4, normalise="transition")
    assert rows["name"].tolist() == [f"stego_LSBR_alpha_0.1/{k}.png" for k in ORDER] and (rows["stego_method"] == "LSBR").all() and (rows["alpha"] == 0.1).all()
    stegos = np.stack([_plane(f"stego_LSBR_0.1_{k}.png") for k in ORDER])
    np.testing.assert_array_equal(F, spam_np.features(spam_np.counts(stegos, 1, 4), 1, 4, "transition"))
    x = torch.from_numpy(covers).to(DEV)
    for method, stream in (("LSBR", 3), ("HILLR", 0)):
        rows, F = spam.extract(dataset, method, 0.4, simulate=True, stream=stream, batch_size=3)
        assert rows["name"].tolist() == [f"{embed.folder_name(method, 0.4)}/{k}.png" for k in ORDER] and (rows["stego_method"] == method).all()
        twins = embed.simulate(x, method, 0.4, [embed.image_seed(f"{k}.png", stream) for k in ORDER])[0].cpu().numpy()
        assert (twins != covers).any()
        np.testing.assert_array_equal(F, spam_np.features(spam_np.counts(twins)))
    with pytest.raises(ValueError, match="LSBR / HILLR"):
        spam.extract(dataset, "LSBRS", 0.4, simulate=True)
    with pytest.raises(ValueError, match="lists no stego rows"):
        spam.extract(dataset, "LSBR", 0.1, split="split_te.csv")


def test_fit_score_and_the_roc_row(dataset, tmp_path):
    model_path, csv, sim = tmp_path / "spam_fld.npz", tmp_path / "spam.csv", tmp_path / "spam_sim.csv"
    spam.main(["fit", "--data", str(dataset), "--stego-methods", "LSBR", "--alphas", "0.1", "--out", str(model_path)])
    model = spam.FLD.load(model_path)
    assert (model.order, model.T, model.normalise, model.ridge, model.stego_methods, model.alphas) == (2, 3, "joint", 0.1, ["LSBR"], [0.1])
    assert model.w.shape == (686,)
    spam.main(["score", "--data", str(dataset), "--model", str(model_path), "--stego-methods", "LSBR", "--alphas", "0.1", "--out", str(csv)])
    df = pd.read_csv(csv, float_precision="round_trip")
    assert list(df.columns) == ["name", "height", "width", "output", "prediction", "stego_method", "alpha"] == list(pd.read_csv(GOLDEN / "b0.csv").columns)
    assert df["name"].tolist() == [f"images/{k}.png" for k in ORDER] + [f"stego_LSBR_alpha_0.1/{k}.png" for k in ORDER]
    assert df["stego_method"][:5].isna().all() and df["alpha"][:5].isna().all()
    assert (df["stego_method"][5:] == "LSBR").all() and (df["alpha"][5:] == 0.1).all() and (df["height"] == 512).all() and (df["width"] == 512).all()
    assert df["output"].between(0., 1.).all() and df["prediction"].dtype == bool and (df["prediction"] == (df["output"] > 0.5)).all()
    # the scores are the model's outputs on the restated features of the same files
    planes = np.stack([_plane(f"cover_{k}.png") for k in ORDER] + [_plane(f"stego_LSBR_0.1_{k}.png") for k in ORDER])
    want = model.output(spam_np.features(spam_np.counts(planes)))
    assert np.abs(df["output"].to_numpy() - want).max() <= 1e-12
    w, b = spam_np.fld_fit(spam_np.features(spam_np.counts(planes[:5])), spam_np.features(spam_np.counts(planes[5:])), 0.1)
    np.testing.assert_array_equal(model.w, w)
    # ws.roc reads the file as a detector
    scores = roc.load_scores(csv, "B0_SPAM", ["LSBR"], [.1])
    assert len(scores) == 10 and (scores["model_name"] == "B0_SPAM").all() and np.array_equal(scores["score"].to_numpy(), df["output"].to_numpy())
    with pytest.raises(ValueError, match="B0"):
        roc.load_scores(csv, "SPAM", ["LSBR"], [.1])
    out = tmp_path / "roc"
    roc.main(["--data", str(dataset), "--out-dir", str(out), "--stego-methods", "LSBR", "--alphas", "0.1", "--filters", "AVG", "KB",
              "--scores", str(csv), "B0_SPAM"])
    auc = pd.read_csv(out / "auc_0.1.csv")
    assert sorted(auc["model_name"]) == ["AVG", "B0_SPAM", "KB"] and auc["auc"].between(0., 1.).all()
    got = float(auc[auc.model_name == "B0_SPAM"]["auc"].iloc[0])
    print(f"AUC of B0_SPAM on its own five training pairs: {got}")
    assert any(c.endswith("LSBR_B0_SPAM") for c in pd.read_csv(out / "roc_0.1.csv").columns)
    # --simulate: the covers are read as before, the twins are made on the device
    spam.main(["score", "--data", str(dataset), "--model", str(model_path), "--stego-methods", "LSBR", "--alphas", "0.1", "--simulate", "--out", str(sim)])
    ds = pd.read_csv(sim, float_precision="round_trip")
    assert ds[:5].equals(df[:5]) and len(ds) == 10
    assert ds["name"][5:].tolist() == [f"{embed.folder_name('LSBR', 0.1)}/{k}.png" for k in ORDER] and (ds["stego_method"][5:] == "LSBR").all()
    # `features` writes the matrices `extract` returns
    fz = tmp_path / "F.npz"
    spam.main(["features", "--data", str(dataset), "--stego-methods", "LSBR", "--alphas", "0.1", "--out", str(fz)])
    with np.load(fz, allow_pickle=False) as z:
        assert z["cover"].shape == (5, 686) and z["LSBR_0.1"].shape == (5, 686) and z["cover_names"].tolist() == [f"images/{k}.png" for k in ORDER]
        np.testing.assert_array_equal(z["LSBR_0.1"], spam_np.features(spam_np.counts(planes[5:])))
