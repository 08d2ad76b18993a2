"""GPU: the counts of the linear SRM submodels (K49, ops.srm_counts) bit for bit against numpy (srm_np) in every case, their totals, batch
and output handling; the features and the Fisher discriminant on device counts against the restatement on crops of the golden covers;
the drivers (`fit`, `score`, `simulate=True` with the +-1 and the wavelet-cost senders) and the detector's row in the ROC tables."""
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import srm_np
from ws_unet_amd import costs, embed, embed_pm1, ops, spam, srm
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import roc

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
SHAPES = [(1, 1, 1), (1, 4, 4), (1, 5, 8), (1, 8, 5), (1, 8, 8), (2, 9, 21), (1, 16, 300), (1, 67, 259), (2, 131, 40), (1, 33, 513)]


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


def _counts(x: np.ndarray, **kw) -> np.ndarray:
    return ops.srm_counts(torch.from_numpy(x).to(DEV), **kw).cpu().numpy()


def _patterns(shape):
    n, h, w = shape
    rr, cc = np.indices((h, w))
    return {"constant": np.full(shape, 77, dtype=np.uint8), "all 0": np.zeros(shape, dtype=np.uint8), "all 255": np.full(shape, 255, dtype=np.uint8),
            "checkerboard": np.broadcast_to(((rr + cc) % 2 * 255).astype(np.uint8), shape).copy(),
            "horizontal ramp": np.broadcast_to((cc % 256).astype(np.uint8), shape).copy(),
            "noise in 0..3": np.random.default_rng(h + w).integers(0, 4, shape, dtype=np.uint8)}


# ---- K49 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_counts_equal_numpy_bit_for_bit(shape):
    """no run; runs of the differences only; exactly one horizontal / one vertical / one of each 5x5 run; a strip edge inside a run; a
    ragged last strip; an odd width with rows off the 16-byte grid over several row tiles; a narrow image; one row and one column past
    32 x 512 pixels"""
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    if shape[1] * shape[2] >= 64:
        x[:, : shape[1] // 2, : shape[2] // 3] //= 64                       # a smooth corner: small residuals, the centre bins among them
    got = _counts(x)
    assert got.dtype == np.int64 and got.shape == (shape[0], 44, 625)
    np.testing.assert_array_equal(got, srm_np.counts(x))
    assert (got.sum(axis=2) == np.array(srm_np.totals(*shape[1:]))).all()
    assert srm_np.totals(*shape[1:]) == [max(shape[1] - t[4], 0) * max(shape[2] - t[5], 0) for t in ops.SRM_TABLES]


@pytest.mark.parametrize("shape", [(1, 66, 258), (1, 512, 512)])
def test_counts_of_value_patterns(shape):
    """a constant plane puts every run into the centre bin of its table (the register path, nothing else); on a 0 / 255 checkerboard every
    digit is -2 or 2; a ramp has one horizontal difference and the wrap 255 -> 0; noise in 0..3 sits on the rounding ties of every integer q"""
    tot = srm_np.totals(*shape[1:])
    for name, x in _patterns(shape).items():
        got = _counts(x)
        np.testing.assert_array_equal(got, srm_np.counts(x), err_msg=name)
        if name in ("constant", "all 0", "all 255"):
            assert got[0, :, 312].tolist() == tot and got.sum() == sum(tot), name
        if name == "checkerboard":
            saturated = [b for b in range(625) if all(b // 5 ** k % 5 in (0, 4) for k in range(4))]
            assert (got[0][:, saturated].sum(axis=1) == np.array(tot)).all()


def test_counts_of_natural_images():
    x = np.stack([_plane("cover_6.png"), _plane("stego_LSBR_1.0_7.png")])
    np.testing.assert_array_equal(_counts(x), srm_np.counts(x))


def test_batch_output_and_repeat():
    xn = np.random.default_rng(3).integers(0, 256, (3, 70, 90), dtype=np.uint8)
    xn[1] //= 32
    x = torch.from_numpy(xn).to(DEV)
    want = srm_np.counts(xn)
    got = ops.srm_counts(x)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    for i in range(3):                                                       # a batch is its images one by one
        assert torch.equal(ops.srm_counts(x[i:i + 1])[0], got[i])
    out = torch.full((3, 44, 625), 7, dtype=torch.int64, device=DEV)         # a dirty buffer, used twice: the entry point zeroes it
    for _ in range(2):
        assert ops.srm_counts(x, out=out) is out
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert torch.equal(ops.srm_counts(x), ops.srm_counts(x))
    lib = ops._lib.load()
    raw = torch.full((3, 44, 625), 7, dtype=torch.int64, device=DEV)
    ops.check(lib.wsu_srm_counts(x.data_ptr(), raw.data_ptr(), 3, 70, 90, ops._stream()), "wsu_srm_counts")
    np.testing.assert_array_equal(raw.cpu().numpy(), want)


def test_argument_errors():
    with pytest.raises(ValueError, match="no images"):
        ops.srm_counts(torch.zeros((0, 8, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(Exception, match="contiguous"):
        ops.srm_counts(torch.zeros((1, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2])
    with pytest.raises(ValueError):
        ops.srm_counts(torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV))
    x = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    for out in (torch.zeros((1, 4, 625), dtype=torch.int64, device=DEV), torch.zeros((1, 44, 625), dtype=torch.int32, device=DEV),
                torch.zeros((2, 44, 625), dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match="out must be"):
            ops.srm_counts(x, out=out)
    lib = ops._lib.load()
    assert lib.wsu_srm_counts(x.data_ptr(), None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_srm_counts(None, x.data_ptr(), 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert srm.features(ops.srm_counts(x)).shape == (1, 3718)               # 8 x 8 has one run of each 5x5 table
    with pytest.raises(ValueError, match="image 0"):                         # four rows: no run of the 3x3 or the 5x5 kernel
        srm.features(ops.srm_counts(torch.zeros((1, 4, 30), dtype=torch.uint8, device=DEV)))


# ---- the detector on crops of the golden covers --------------------------------------------------------------------------------------

def _crops(ks):
    return np.stack([p[r:r + 64, c:c + 64] for p in (_plane(f"cover_{k}.png") for k in ks) for r in range(0, 512, 64) for c in range(0, 512, 64)])


@pytest.fixture(scope="module")
def crop_sets():
    """64 x 64 crops of covers 6-8 (192, training) and of covers 9-10 (128, held out) with their LSBM twins at alpha 1.0 made on the device,
    and the restated features of all four sets: ((cover, stego planes), (cover, stego features)) per set"""
    sets = []
    for ks, seed0 in (((6, 7, 8), 1000), ((9, 10), 5000)):
        cover = _crops(ks)
        stego = embed_pm1.simulate(torch.from_numpy(cover).to(DEV), "LSBM", 1.0, [seed0 + i for i in range(len(cover))])[0].cpu().numpy()
        assert ((stego != cover).sum(axis=(1, 2)) > 1500).all()              # about half of 4096 pixels each
        sets.append(((cover, stego), tuple(srm_np.features(srm_np.counts(x)) for x in (cover, stego))))
    assert len(sets[0][0][0]) == 192 and len(sets[1][0][0]) == 128
    return sets


def test_device_features_equal_the_restated_ones(crop_sets):
    for planes, restated in crop_sets:
        for x, want in zip(planes, restated):
            got = srm.features(ops.srm_counts(torch.from_numpy(x).to(DEV)))
            assert got.shape == (len(x), 3718)
            np.testing.assert_array_equal(got, want)


def test_detector_on_crops_equals_the_restatement_and_detects(crop_sets):
    """FLD(ridge 0.1) on the 3 718 features of 192 crops and their LSBM twins, scored on 128 held-out crops and theirs.  The device
    features are the restated ones exactly, so outputs and AUC agree to 1e-12.  The restatement's own AUC must be >= 0.75: a condition on
    the inputs (a numpy prototype with numpy LSBM twins of the same crops reached 0.836, SPAM-686 0.826)."""
    dev = lambda x: srm.features(ops.srm_counts(torch.from_numpy(x).to(DEV)))
    ((c_tr, s_tr), (rc_tr, rs_tr)), ((c_te, s_te), (rc_te, rs_te)) = crop_sets
    model = srm.FLD(ridge=0.1).fit(dev(c_tr), dev(s_tr))
    w, b = srm_np.fld_fit(rc_tr, rs_tr, 0.1)
    got0, got1 = model.output(dev(c_te)), model.output(dev(s_te))
    want0, want1 = srm_np.fld_output(rc_te, w, b), srm_np.fld_output(rs_te, w, b)
    auc_got, auc_want = srm_np.auc(got0, got1), srm_np.auc(want0, want1)
    print(f"held-out AUC: device {auc_got:.6f}, restatement {auc_want:.6f}; max |output difference| {max(np.abs(got0 - want0).max(), np.abs(got1 - want1).max()):.3e}")
    assert auc_want >= 0.75
    assert np.abs(got0 - want0).max() <= 1e-12 and np.abs(got1 - want1).max() <= 1e-12
    assert abs(auc_got - auc_want) <= 1e-12
    assert ((got0 >= 0) & (got0 <= 1)).all() and ((got1 >= 0) & (got1 <= 1)).all()


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the five golden covers and their LSBR alpha 0.1 twins as a data set"""
    root = tmp_path_factory.mktemp("srm_data")
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


@pytest.fixture(scope="module")
def file_features():
    """the restated features of the data set's files in fabrika's order: (cover planes, covers' features, stegos' features)"""
    covers = np.stack([_plane(f"cover_{k}.png") for k in ORDER])
    stegos = np.stack([_plane(f"stego_LSBR_0.1_{k}.png") for k in ORDER])
    return covers, srm_np.features(srm_np.counts(covers)), srm_np.features(srm_np.counts(stegos))


def test_extract_covers_stegos_and_simulated_twins(dataset, file_features):
    covers, F_cover, F_stego = file_features
    rows, F = srm.extract(dataset)
    assert rows["name"].tolist() == [f"images/{k}.png" for k in ORDER] and rows["stego_method"].isna().all() and rows["alpha"].isna().all()
    np.testing.assert_array_equal(F, F_cover)
    rows2, F2 = srm.extract(dataset, split="split_te.csv", batch_size=2)     # chunks of 2, 2, 1
    assert rows2.equals(rows) and np.array_equal(F2, F)
    rows, F = srm.extract(dataset, "LSBR", 0.1)
    assert rows["name"].tolist() == [f"stego_LSBR_alpha_0.1/{k}.png" for k in ORDER] and (rows["stego_method"] == "LSBR").all() and (rows["alpha"] == 0.1).all()
    np.testing.assert_array_equal(F, F_stego)
    x = torch.from_numpy(covers).to(DEV)
    for maker, method, stream in ((embed_pm1, "LSBM", 3), (costs, "SUNIWARD", 0)):
        rows, F = srm.extract(dataset, method.lower(), 0.4, simulate=True, stream=stream, batch_size=3)
        assert rows["name"].tolist() == [f"{maker.folder_name(method, 0.4)}/{k}.png" for k in ORDER] and (rows["stego_method"] == method).all()
        twins = maker.simulate(x, method, 0.4, [embed.image_seed(f"{k}.png", stream) for k in ORDER])[0].cpu().numpy()
        assert (twins != covers).any()
        np.testing.assert_array_equal(F, srm_np.features(srm_np.counts(twins)))
    with pytest.raises(ValueError, match="SUNIWARD / WOW"):
        srm.extract(dataset, "LSBRS", 0.4, simulate=True)
    with pytest.raises(ValueError, match="lists no stego rows"):
        srm.extract(dataset, "LSBR", 0.1, split="split_te.csv")


def test_fit_score_and_the_roc_row(dataset, file_features, tmp_path):
    _, F_cover, F_stego = file_features
    model_path, csv = tmp_path / "srm_fld.npz", tmp_path / "srm.csv"
    srm.main(["fit", "--data", str(dataset), "--stego-methods", "LSBR", "--alphas", "0.1", "--out", str(model_path)])
    model = srm.load(model_path)
    assert (model.order, model.T, model.ridge, model.stego_methods, model.alphas) == (4, 2, 0.1, ["LSBR"], [0.1]) and model.w.shape == (3718,)
    w, b = srm_np.fld_fit(F_cover, F_stego, 0.1)
    np.testing.assert_array_equal(model.w, w)
    srm.main(["score", "--data", str(dataset), "--model", str(model_path), "--stego-methods", "LSBR", "--alphas", "0.1", "--out", str(csv)])
    df = pd.read_csv(csv, float_precision="round_trip")
    assert list(df.columns) == ["name", "height", "width", "output", "prediction", "stego_method", "alpha"] == list(pd.read_csv(GOLDEN / "b0.csv").columns)
    assert df["name"].tolist() == [f"images/{k}.png" for k in ORDER] + [f"stego_LSBR_alpha_0.1/{k}.png" for k in ORDER]
    assert df["stego_method"][:5].isna().all() and df["alpha"][:5].isna().all()
    assert (df["stego_method"][5:] == "LSBR").all() and (df["alpha"][5:] == 0.1).all() and (df["height"] == 512).all() and (df["width"] == 512).all()
    assert df["output"].between(0., 1.).all() and df["prediction"].dtype == bool and (df["prediction"] == (df["output"] > 0.5)).all()
    want = srm_np.fld_output(np.concatenate([F_cover, F_stego]), w, b)      # the scores are the model's outputs on the restated features
    assert np.abs(df["output"].to_numpy() - want).max() <= 1e-12
    # ws.roc reads the file as a detector
    scores = roc.load_scores(csv, "B0_SRM", ["LSBR"], [.1])
    assert len(scores) == 10 and (scores["model_name"] == "B0_SRM").all() and np.array_equal(scores["score"].to_numpy(), df["output"].to_numpy())
    out = tmp_path / "roc"
    roc.main(["--data", str(dataset), "--out-dir", str(out), "--stego-methods", "LSBR", "--alphas", "0.1", "--filters", "AVG", "KB",
              "--scores", str(csv), "B0_SRM"])
    auc = pd.read_csv(out / "auc_0.1.csv")
    assert sorted(auc["model_name"]) == ["AVG", "B0_SRM", "KB"] and auc["auc"].between(0., 1.).all()
    assert any(c.endswith("LSBR_B0_SRM") for c in pd.read_csv(out / "roc_0.1.csv").columns)
    # neither loader takes the other's model
    with pytest.raises(Exception):
        spam.FLD.load(model_path)
    spam_path = tmp_path / "spam_fld.npz"
    rng = np.random.default_rng(0)
    spam.FLD().fit(rng.random((6, 686)), rng.random((6, 686))).save(spam_path)
    with pytest.raises(ValueError, match="srm-linear"):
        srm.load(spam_path)
