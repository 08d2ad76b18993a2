"""GPU: the counts of the SRM min/max submodels (K50, ops.srm_minmax_counts) bit for bit against numpy (srm_minmax_np) in every case, their
totals, batch and output handling; `features_minmax` of device counts against the restatement; the Fisher discriminant on the 13 000
and the 16 718 features on crops of the golden covers; the drivers with `submodels=` and the detector's row in the ROC tables."""
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import srm_minmax_np as mm_np
import srm_np
from ws_unet_amd import costs, embed, embed_pm1, ops, srm
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import roc

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
# K50's tile is 64 rows x 512 columns: the last shape is one row and one column past it
SHAPES = [(1, 1, 1), (1, 4, 7), (1, 5, 8), (1, 8, 5), (2, 9, 21), (1, 16, 300), (1, 67, 259), (2, 131, 40), (1, 65, 513)]
AT = {t: i for i, t in enumerate(mm_np.TABLES)}


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


def _counts(x: np.ndarray, **kw) -> np.ndarray:
    return ops.srm_minmax_counts(torch.from_numpy(x).to(DEV), **kw).cpu().numpy()


def _pattern(name, shape):
    n, h, w = shape
    rr, cc = np.indices((h, w))
    if name == "constant":
        return np.full(shape, 77, dtype=np.uint8)
    if name == "all 0":
        return np.zeros(shape, dtype=np.uint8)
    if name == "all 255":
        return np.full(shape, 255, dtype=np.uint8)
    if name == "checkerboard":
        return np.broadcast_to(((rr + cc) % 2 * 255).astype(np.uint8), shape).copy()
    if name == "horizontal ramp":
        return np.broadcast_to((cc % 256).astype(np.uint8), shape).copy()
    if name == "noise in 0..3":
        return np.random.default_rng(h + w).integers(0, 4, shape, dtype=np.uint8)
    assert name == "impulses"                                              # single pixels +-9 on a flat ground, about one in 40
    rng = np.random.default_rng(h * w)
    return (128 + 9 * rng.choice([-1, 1], shape) * (rng.random(shape) < 0.025)).astype(np.uint8)


PATTERNS = ("constant", "all 0", "all 255", "checkerboard", "horizontal ramp", "noise in 0..3", "impulses")


# ---- K50 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_counts_equal_numpy_bit_for_bit(shape):
    """no run; the third-order sets mostly empty; exactly one run of S3 WENS scanned h / scanned v; a strip edge inside a run; a ragged
    last strip; an odd width with rows off the 16-byte grid over several row tiles; a narrow image; one row and one column past the
    tile of 64 x 512 pixels"""
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    if shape[1] * shape[2] >= 64:
        x[:, : shape[1] // 2, : shape[2] // 3] //= 64                       # a smooth corner: small residuals, the centre bins among them
    got = _counts(x)
    assert got.dtype == np.int64 and got.shape == (shape[0], 118, 625)
    tot = mm_np.totals(*shape[1:])
    assert (got.sum(axis=2) == np.array(tot)).all()
    np.testing.assert_array_equal(got, mm_np.counts(x))
    assert tot == [2 * max(shape[1] - t[4], 0) * max(shape[2] - t[5], 0) for t in ops.SRM_MINMAX_TABLES]
    if shape == (1, 1, 1):
        assert not got.any()
    if shape in ((1, 5, 8), (1, 8, 5)):
        scans = "hv" if shape == (1, 5, 8) else "vh"
        assert [int(got[0, AT["S3", q2, "WENS", s]].sum()) for q2 in (6, 9, 12) for s in scans] == [2, 0] * 3


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", [(1, 66, 258), (1, 512, 512)])
def test_counts_of_value_patterns(shape, pattern):
    """a constant plane puts every update into the centre bin of its table (the register path, nothing else); on a 0 / 255 checkerboard
    every digit is -2, 0 or 2; a ramp has one horizontal difference and the wrap 255 -> 0; noise in 0..3 sits on the rounding ties of
    every integer q; around a single-pixel impulse lo and hi of every set differ most"""
    x = _pattern(pattern, shape)
    tot = mm_np.totals(*shape[1:])
    got = _counts(x)
    assert (got.sum(axis=2) == np.array(tot)).all(), pattern
    np.testing.assert_array_equal(got, mm_np.counts(x), err_msg=pattern)
    if pattern in ("constant", "all 0", "all 255"):
        assert got[0, :, 312].tolist() == tot and got.sum() == sum(tot)
    if pattern == "checkerboard":
        saturated = [b for b in range(625) if all(b // 5 ** k % 5 in (0, 2, 4) for k in range(4))]
        assert (got[0][:, saturated].sum(axis=1) == np.array(tot)).all()
    if pattern == "impulses":
        assert (got[0, :, 312] < np.array(tot)).all()


def test_counts_of_natural_images():
    x = np.stack([_plane("cover_6.png"), _plane("stego_LSBR_1.0_7.png")])
    np.testing.assert_array_equal(_counts(x), mm_np.counts(x))


def test_batch_output_and_repeat():
    xn = np.random.default_rng(3).integers(0, 256, (3, 70, 90), dtype=np.uint8)
    xn[1] //= 32
    x = torch.from_numpy(xn).to(DEV)
    want = mm_np.counts(xn)
    got = ops.srm_minmax_counts(x)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    for i in range(3):                                                       # a batch is its images one by one
        assert torch.equal(ops.srm_minmax_counts(x[i:i + 1])[0], got[i])
    out = torch.full((3, 118, 625), 7, dtype=torch.int64, device=DEV)        # a dirty buffer, used twice: the entry point zeroes it
    for _ in range(2):
        assert ops.srm_minmax_counts(x, out=out) is out
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert torch.equal(ops.srm_minmax_counts(x), ops.srm_minmax_counts(x))
    lib = ops._lib.load()
    raw = torch.full((3, 118, 625), 7, dtype=torch.int64, device=DEV)
    ops.check(lib.wsu_srm_minmax_counts(x.data_ptr(), raw.data_ptr(), 3, 70, 90, ops._stream()), "wsu_srm_minmax_counts")
    np.testing.assert_array_equal(raw.cpu().numpy(), want)


def test_plane_off_the_16_byte_grid():
    """planes of 37 x 53 cut out of a byte buffer at offsets 1, 2 and 7: no row and no strip starts on a multiple of 16 or of 4"""
    rng = np.random.default_rng(12)
    buf = torch.from_numpy(rng.integers(0, 256, 64 + 2 * 37 * 53, dtype=np.uint8)).to(DEV)
    for off in (1, 2, 7):
        x = buf[off:off + 2 * 37 * 53].view(2, 37, 53)
        assert x.data_ptr() % 16 == off and x.is_contiguous()
        np.testing.assert_array_equal(ops.srm_minmax_counts(x).cpu().numpy(), mm_np.counts(x.cpu().numpy()))


def test_argument_errors():
    with pytest.raises(ValueError, match="no images"):
        ops.srm_minmax_counts(torch.zeros((0, 8, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(Exception, match="contiguous"):
        ops.srm_minmax_counts(torch.zeros((1, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2])
    with pytest.raises(ValueError):
        ops.srm_minmax_counts(torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV))
    x = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    for out in (torch.zeros((1, 44, 625), dtype=torch.int64, device=DEV), torch.zeros((1, 118, 625), dtype=torch.int32, device=DEV),
                torch.zeros((2, 118, 625), dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match="out must be"):
            ops.srm_minmax_counts(x, out=out)
    lib = ops._lib.load()
    assert lib.wsu_srm_minmax_counts(x.data_ptr(), None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_srm_minmax_counts(None, x.data_ptr(), 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert srm.features_minmax(ops.srm_minmax_counts(x)).shape == (1, 13000)  # 8 x 8 has a run of every table
    with pytest.raises(ValueError, match="image 0"):                         # four rows: no vertical run of a third-order set
        srm.features_minmax(ops.srm_minmax_counts(torch.zeros((1, 4, 30), dtype=torch.uint8, device=DEV)))


# ---- the detector on crops of the golden covers --------------------------------------------------------------------------------------

def _crops(ks):
    return np.stack([p[r:r + 64, c:c + 64] for p in (_plane(f"cover_{k}.png") for k in ks) for r in range(0, 512, 64) for c in range(0, 512, 64)])


@pytest.fixture(scope="module")
def crop_sets():
    """the fixture of test_gpu_srm.py: 64 x 64 crops of covers 6-8 (192, training) and of covers 9-10 (128, held out) with their LSBM twins
    at alpha 1.0 made on the device: (cover, stego) planes per set"""
    sets = []
    for ks, seed0 in (((6, 7, 8), 1000), ((9, 10), 5000)):
        cover = _crops(ks)
        stego = embed_pm1.simulate(torch.from_numpy(cover).to(DEV), "LSBM", 1.0, [seed0 + i for i in range(len(cover))])[0].cpu().numpy()
        assert ((stego != cover).sum(axis=(1, 2)) > 1500).all()
        sets.append((cover, stego))
    assert len(sets[0][0]) == 192 and len(sets[1][0]) == 128
    return sets


def test_device_features_equal_the_restated_ones(crop_sets):
    """every twelfth crop of the four sets (16 + 16 + 11 + 11): the restatement of all 640 would take a quarter of a minute"""
    for planes in crop_sets:
        for x in planes:
            x = x[::12]
            got = srm.features_minmax(ops.srm_minmax_counts(torch.from_numpy(x).to(DEV)))
            assert got.shape == (len(x), 13000)
            np.testing.assert_array_equal(got, mm_np.features(mm_np.counts(x)))


def test_detectors_on_crops_detect(crop_sets):
    """FLD(ridge 0.1), fitted in the dual, on the 13 000 min/max features and on all 16 718 of 192 crops and their LSBM twins at alpha
    1.0, scored on 128 held-out crops and theirs: the held-out AUC must be >= 0.75, the condition of the linear features' test (a numpy
    prototype with numpy twins reached 0.8505 and 0.8514, the linear features 0.838; on the device twins 0.8388 and 0.8289, linear
    0.8356).  Five images show that the features work, not how well."""
    (c_tr, s_tr), (c_te, s_te) = crop_sets
    dev = lambda x: torch.from_numpy(x).to(DEV)
    feats = {"linear": lambda x: srm.features(ops.srm_counts(dev(x))), "minmax": lambda x: srm.features_minmax(ops.srm_minmax_counts(dev(x)))}
    F = {k: [f(x) for x in (c_tr, s_tr, c_te, s_te)] for k, f in feats.items()}
    F["all"] = [np.concatenate([a, b], axis=1) for a, b in zip(F["linear"], F["minmax"])]
    aucs = {}
    for sub in ("linear", "minmax", "all"):
        model = srm.FLD(0.1, sub).fit(F[sub][0], F[sub][1])
        out0, out1 = model.output(F[sub][2]), model.output(F[sub][3])
        assert ((out0 >= 0) & (out0 <= 1)).all() and ((out1 >= 0) & (out1 <= 1)).all()
        aucs[sub] = srm_np.auc(out0, out1)
    print("held-out AUC, LSBM alpha 1.0: " + ", ".join(f"{k} {v:.4f}" for k, v in aucs.items()))
    assert aucs["minmax"] >= 0.75 and aucs["all"] >= 0.75


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the five golden covers and their LSBR alpha 0.1 twins as a data set"""
    root = tmp_path_factory.mktemp("srm_minmax_data")
    (root / "images").mkdir()
    sdir = root / "stego_LSBR_alpha_0.1"
    sdir.mkdir()
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
        shutil.copy(GOLDEN / f"stego_LSBR_0.1_{k}.png", sdir / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    (sdir / "files.csv").write_text("name,height,width,stego_method,alpha\n" + "".join(
        f"stego_LSBR_alpha_0.1/{k}.png,512,512,LSBR,0.1\n" for k in COVERS))
    return root


ORDER = (10, 6, 7, 8, 9)                                                    # fabrika sorts names lexically


def _all_features(x: torch.Tensor) -> np.ndarray:
    return np.concatenate([srm.features(ops.srm_counts(x)), srm.features_minmax(ops.srm_minmax_counts(x))], axis=1)


def test_extract_with_submodels(dataset):
    covers = torch.from_numpy(np.stack([_plane(f"cover_{k}.png") for k in ORDER])).to(DEV)
    stegos = torch.from_numpy(np.stack([_plane(f"stego_LSBR_0.1_{k}.png") for k in ORDER])).to(DEV)
    want = _all_features(covers)
    rows, F = srm.extract(dataset, submodels="all", batch_size=2)            # chunks of 2, 2, 1
    assert rows["name"].tolist() == [f"images/{k}.png" for k in ORDER] and F.shape == (5, 16718)
    np.testing.assert_array_equal(F, want)
    rows_l, F_l = srm.extract(dataset)                                       # the default: the linear features as they were
    assert rows_l.equals(rows) and F_l.tobytes() == want[:, :3718].tobytes()
    np.testing.assert_array_equal(srm.extract(dataset, submodels="minmax")[1], want[:, 3718:])
    rows, F = srm.extract(dataset, "LSBR", 0.1, submodels="minmax")
    assert rows["name"].tolist() == [f"stego_LSBR_alpha_0.1/{k}.png" for k in ORDER]
    np.testing.assert_array_equal(F, srm.features_minmax(ops.srm_minmax_counts(stegos)))
    rows, F = srm.extract(dataset, "suniward", 0.4, simulate=True, submodels="all", batch_size=3)
    assert rows["name"].tolist() == [f"{costs.folder_name('SUNIWARD', 0.4)}/{k}.png" for k in ORDER] and (rows["stego_method"] == "SUNIWARD").all()
    twins = costs.simulate(covers, "SUNIWARD", 0.4, [embed.image_seed(f"{k}.png", 0) for k in ORDER])[0]
    assert (twins != covers).any()
    np.testing.assert_array_equal(F, _all_features(twins))


def test_fit_score_with_all_submodels_and_the_roc_row(dataset, tmp_path):
    model_path, csv = tmp_path / "srm_all.npz", tmp_path / "srm_all.csv"
    common = ["--data", str(dataset), "--stego-methods", "SUNIWARD", "--alphas", "0.4", "--submodels", "all", "--simulate"]
    srm.main(["fit", *common, "--out", str(model_path)])
    model = srm.load(model_path, "all")
    assert (model.submodels, model.ridge, model.stego_methods, model.alphas) == ("all", 0.1, ["SUNIWARD"], [0.4]) and model.w.shape == (16718,)
    covers = torch.from_numpy(np.stack([_plane(f"cover_{k}.png") for k in ORDER])).to(DEV)
    twins = costs.simulate(covers, "SUNIWARD", 0.4, [embed.image_seed(f"{k}.png", 0) for k in ORDER])[0]
    F0, F1 = _all_features(covers), _all_features(twins)
    np.testing.assert_array_equal(model.w, srm.FLD(0.1, "all").fit(F0, F1).w)
    srm.main(["score", *common, "--model", str(model_path), "--out", str(csv)])
    df = pd.read_csv(csv, float_precision="round_trip")
    assert list(df.columns) == list(pd.read_csv(GOLDEN / "b0.csv").columns)
    folder = costs.folder_name("SUNIWARD", 0.4)
    assert df["name"].tolist() == [f"images/{k}.png" for k in ORDER] + [f"{folder}/{k}.png" for k in ORDER]
    assert df["stego_method"][:5].isna().all() and (df["stego_method"][5:] == "SUNIWARD").all() and (df["alpha"][5:] == 0.4).all()
    assert np.abs(df["output"].to_numpy() - model.output(np.concatenate([F0, F1]))).max() <= 1e-12
    assert df["output"].between(0., 1.).all() and (df["prediction"] == (df["output"] > 0.5)).all()
    with pytest.raises(ValueError, match="not a model on the 'srm-linear' features but on 'srm-all'"):
        srm.main(["score", "--data", str(dataset), "--model", str(model_path), "--alphas", "0.1", "--out", str(tmp_path / "no.csv")])
    # ws.roc reads such a file as a detector: the same model on the data set's LSBR files, beside two WS filters
    csv = tmp_path / "srm_all_lsbr.csv"
    srm.main(["score", "--data", str(dataset), "--model", str(model_path), "--stego-methods", "LSBR", "--alphas", "0.1", "--submodels", "all",
              "--out", str(csv)])
    df = pd.read_csv(csv, float_precision="round_trip")
    scores = roc.load_scores(csv, "B0_SRM", ["LSBR"], [.1])
    assert len(scores) == 10 and (scores["model_name"] == "B0_SRM").all() and np.array_equal(scores["score"].to_numpy(), df["output"].to_numpy())
    out = tmp_path / "roc"
    roc.main(["--data", str(dataset), "--out-dir", str(out), "--stego-methods", "LSBR", "--alphas", "0.1", "--filters", "AVG", "KB",
              "--scores", str(csv), "B0_SRM"])
    auc = pd.read_csv(out / "auc_0.1.csv")
    assert sorted(auc["model_name"]) == ["AVG", "B0_SRM", "KB"] and auc["auc"].between(0., 1.).all()
    assert any(c.endswith("LSBR_B0_SRM") for c in pd.read_csv(out / "roc_0.1.csv").columns)
