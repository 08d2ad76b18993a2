"""GPU: the counts of the SRM fan submodels (K54, ops.srm_fan_counts) and of the EDGE classes (K55, ops.srm_edge_counts) bit for bit
against numpy (srm_fans_np, srm_edge_np) in every case, their totals, batch and output handling; `features_fans` / `features_edge` of
device counts against the restatements; the Fisher discriminant on the three new feature sets on crops of the golden covers; the
drivers with `submodels='full'`."""
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import srm_edge_np as edge_np
import srm_fans_np as fans_np
import srm_np
from test_gpu_srm_minmax import PATTERNS, _pattern
from ws_unet_amd import costs, embed, embed_pm1, ops, srm
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import roc

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
# the kernels' tile is 64 rows x 512 columns: the last shape is one row and one column past it.  (1,5,8) and (1,8,5) have exactly one run
# of the widest sets in one scan and none in the other
SHAPES = [(1, 1, 1), (1, 4, 7), (1, 5, 8), (1, 8, 5), (1, 8, 8), (1, 7, 8), (1, 8, 7), (2, 9, 21), (1, 16, 300), (1, 67, 259), (2, 131, 40),
          (1, 65, 513)]
# per kernel: the op, the restatement, ops' table list, the C entry, and the widest sets (reach 2 every way)
KERNELS = {
    "fans": (ops.srm_fan_counts, fans_np, ops.SRM_FAN_TABLES, "wsu_srm_fan_counts", [("S3", q2, s) for q2 in (6, 9, 12) for s in fans_np.FAN5]),
    "edge": (ops.srm_edge_counts, edge_np, ops.SRM_EDGE_TABLES, "wsu_srm_edge_counts",
             [("E5", q2, s) for q2 in (24, 36, 48) for s in ("UD", "LR", "UDLR")]),
}


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


def _counts(kernel, x: np.ndarray, **kw) -> np.ndarray:
    return KERNELS[kernel][0](torch.from_numpy(x).to(DEV), **kw).cpu().numpy()


# ---- K54, K55 -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_counts_equal_numpy_bit_for_bit(kernel, shape):
    """no run; the third-order / 5x5 sets mostly empty; exactly one run of the widest sets scanned h, resp. v; 8 x 8: one column of four
    runs scanned h and one row of four scanned v (the widest sets take 5 x 8 pixels per run scanned h), eight updates each; 7 x 8 and
    8 x 7: those sets empty in one scan; a strip edge inside a run; a ragged last strip; an odd width with rows off the 16-byte grid over
    several row tiles; a narrow image; one row and one column past the tile of 64 x 512 pixels"""
    _, ref, tables, _, widest = KERNELS[kernel]
    at = {t: i for i, t in enumerate(ref.TABLES)}
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    if shape[1] * shape[2] >= 64:
        x[:, : shape[1] // 2, : shape[2] // 3] //= 64                       # a smooth corner: small residuals, the centre bins among them
    got = _counts(kernel, x)
    assert got.dtype == np.int64 and got.shape == (shape[0], len(tables), 625)
    tot = ref.totals(*shape[1:])
    assert (got.sum(axis=2) == np.array(tot)).all()
    np.testing.assert_array_equal(got, ref.counts(x))
    assert tot == [2 * max(shape[1] - t[4], 0) * max(shape[2] - t[5], 0) for t in tables]
    if shape == (1, 1, 1):
        assert not got.any()
    sums = [[int(got[0, at[cls, q2, s, scan]].sum()) for scan in "hv"] for cls, q2, s in widest]
    expected = {(1, 5, 8): [2, 0], (1, 8, 5): [0, 2], (1, 8, 8): [8, 8], (1, 7, 8): [6, 0], (1, 8, 7): [0, 6]}
    if shape in expected:
        assert sums == [expected[shape]] * len(widest)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_counts_of_value_patterns(kernel, pattern):
    """test_gpu_srm_minmax's seven value patterns: a constant plane puts every update into the centre bin (the register path, nothing
    else); a 0 / 255 checkerboard saturates every digit; a ramp with its wrap; noise in 0..3 on the rounding ties; single-pixel impulses"""
    shape = (1, 66, 258)
    ref = KERNELS[kernel][1]
    x = _pattern(pattern, shape)
    tot = ref.totals(*shape[1:])
    got = _counts(kernel, x)
    assert (got.sum(axis=2) == np.array(tot)).all(), pattern
    np.testing.assert_array_equal(got, ref.counts(x), err_msg=pattern)
    if pattern in ("constant", "all 0", "all 255"):
        assert got[0, :, 312].tolist() == tot and got.sum() == sum(tot)
    if pattern == "checkerboard":
        saturated = [b for b in range(625) if all(b // 5 ** k % 5 in (0, 2, 4) for k in range(4))]
        assert (got[0][:, saturated].sum(axis=1) == np.array(tot)).all()
    if pattern == "impulses":
        assert (got[0, :, 312] < np.array(tot)).all()


@pytest.mark.parametrize("kernel", KERNELS)
def test_counts_of_natural_images(kernel):
    x = np.stack([_plane("cover_6.png")[100:292, 50:250], _plane("stego_LSBR_1.0_7.png")[100:292, 50:250]])
    assert x.shape == (2, 192, 200)
    np.testing.assert_array_equal(_counts(kernel, x), KERNELS[kernel][1].counts(x))


@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_output_and_repeat(kernel):
    op, ref, tables, entry, _ = KERNELS[kernel]
    xn = np.random.default_rng(3).integers(0, 256, (3, 70, 90), dtype=np.uint8)
    xn[1] //= 32
    x = torch.from_numpy(xn).to(DEV)
    want = ref.counts(xn)
    got = op(x)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    for i in range(3):                                                       # a batch is its images one by one
        assert torch.equal(op(x[i:i + 1])[0], got[i])
    out = torch.full((3, len(tables), 625), 7, dtype=torch.int64, device=DEV)   # a dirty buffer, used twice: the entry point zeroes it
    for _ in range(2):
        assert op(x, out=out) is out
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert torch.equal(op(x), op(x))
    lib = ops._lib.load()
    raw = torch.full((3, len(tables), 625), 7, dtype=torch.int64, device=DEV)
    ops.check(getattr(lib, entry)(x.data_ptr(), raw.data_ptr(), 3, 70, 90, ops._stream()), entry)
    np.testing.assert_array_equal(raw.cpu().numpy(), want)


@pytest.mark.parametrize("kernel", KERNELS)
def test_plane_off_the_16_byte_grid(kernel):
    """planes of 37 x 53 cut out of a byte buffer at offsets 1, 2 and 7: no row and no strip starts on a multiple of 16 or of 4"""
    op, ref = KERNELS[kernel][:2]
    rng = np.random.default_rng(12)
    buf = torch.from_numpy(rng.integers(0, 256, 64 + 2 * 37 * 53, dtype=np.uint8)).to(DEV)
    for off in (1, 2, 7):
        x = buf[off:off + 2 * 37 * 53].view(2, 37, 53)
        assert x.data_ptr() % 16 == off and x.is_contiguous()
        np.testing.assert_array_equal(op(x).cpu().numpy(), ref.counts(x.cpu().numpy()))


@pytest.mark.parametrize("kernel", KERNELS)
def test_argument_errors(kernel):
    op, _, tables, entry, _ = KERNELS[kernel]
    T = len(tables)
    with pytest.raises(ValueError, match="no images"):
        op(torch.zeros((0, 8, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(Exception, match="contiguous"):
        op(torch.zeros((1, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2])
    with pytest.raises(ValueError):
        op(torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV))
    x = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    for out in (torch.zeros((1, 118, 625), dtype=torch.int64, device=DEV), torch.zeros((1, T, 625), dtype=torch.int32, device=DEV),
                torch.zeros((2, T, 625), dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match="out must be"):
            op(x, out=out)
    lib = ops._lib.load()
    fn = getattr(lib, entry)
    assert fn(x.data_ptr(), None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert fn(None, x.data_ptr(), 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    features = srm.features_fans if kernel == "fans" else srm.features_edge
    assert features(op(x)).shape == (1, 8125 if kernel == "fans" else 9828)  # 8 x 8 has a run of every table
    with pytest.raises(ValueError, match="image 0"):                         # four rows: no vertical run of a wide set
        features(op(torch.zeros((1, 4, 30), dtype=torch.uint8, device=DEV)))


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
    """every twelfth crop of the four sets (16 + 16 + 11 + 11)"""
    for planes in crop_sets:
        for x in planes:
            x = x[::12]
            dev = torch.from_numpy(x).to(DEV)
            got = srm.features_fans(ops.srm_fan_counts(dev))
            assert got.shape == (len(x), 8125)
            np.testing.assert_array_equal(got, fans_np.features(fans_np.counts(x)))
            got = srm.features_edge(ops.srm_edge_counts(dev))
            assert got.shape == (len(x), 9828)
            np.testing.assert_array_equal(got, edge_np.features(edge_np.counts(x)))


def test_detectors_on_crops_detect(crop_sets):
    """FLD(ridge 0.1), fitted in the dual, on the 8 125 fan features, the 9 828 EDGE features and all 34 671 of 192 crops and their LSBM
    twins at alpha 1.0, scored on 128 held-out crops and theirs: the held-out AUC must be >= 0.75, the condition of the other sets'
    tests (DESIGN.md 4-srmfull has the figures of the numpy prototype and of the device).  Five images show that the features work, not
    how well."""
    (c_tr, s_tr), (c_te, s_te) = crop_sets
    dev = lambda x: torch.from_numpy(x).to(DEV)
    feats = {"linear": lambda x: srm.features(ops.srm_counts(dev(x))), "minmax": lambda x: srm.features_minmax(ops.srm_minmax_counts(dev(x))),
             "fans": lambda x: srm.features_fans(ops.srm_fan_counts(dev(x))), "edge": lambda x: srm.features_edge(ops.srm_edge_counts(dev(x)))}
    F = {k: [f(x) for x in (c_tr, s_tr, c_te, s_te)] for k, f in feats.items()}
    F["full"] = [np.concatenate(parts, axis=1) for parts in zip(F["linear"], F["minmax"], F["fans"], F["edge"])]
    assert F["full"][0].shape == (192, 34671)
    aucs = {}
    for sub in ("linear", "fans", "edge", "full"):
        model = srm.FLD(0.1, sub).fit(F[sub][0], F[sub][1])
        out0, out1 = model.output(F[sub][2]), model.output(F[sub][3])
        assert ((out0 >= 0) & (out0 <= 1)).all() and ((out1 >= 0) & (out1 <= 1)).all()
        aucs[sub] = srm_np.auc(out0, out1)
    print("held-out AUC, LSBM alpha 1.0: " + ", ".join(f"{k} {v:.4f}" for k, v in aucs.items()))
    assert aucs["fans"] >= 0.75 and aucs["edge"] >= 0.75 and aucs["full"] >= 0.75


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the five golden covers and their LSBR alpha 0.1 twins as a data set"""
    root = tmp_path_factory.mktemp("srm_full_data")
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


def _full_features(x: torch.Tensor) -> np.ndarray:
    return np.concatenate([srm.features(ops.srm_counts(x)), srm.features_minmax(ops.srm_minmax_counts(x)),
                           srm.features_fans(ops.srm_fan_counts(x)), srm.features_edge(ops.srm_edge_counts(x))], axis=1)


def test_extract_with_the_full_set(dataset):
    covers = torch.from_numpy(np.stack([_plane(f"cover_{k}.png") for k in ORDER])).to(DEV)
    want = _full_features(covers)
    rows, F = srm.extract(dataset, submodels="full", batch_size=2)           # chunks of 2, 2, 1
    assert rows["name"].tolist() == [f"images/{k}.png" for k in ORDER] and F.shape == (5, 34671)
    np.testing.assert_array_equal(F, want)
    assert srm.extract(dataset, submodels="all")[1].tobytes() == want[:, :16718].tobytes()
    np.testing.assert_array_equal(srm.extract(dataset, submodels="fans")[1], want[:, 16718:16718 + 8125])
    np.testing.assert_array_equal(srm.extract(dataset, "LSBR", 0.1, submodels="edge")[1], srm.features_edge(ops.srm_edge_counts(
        torch.from_numpy(np.stack([_plane(f"stego_LSBR_0.1_{k}.png") for k in ORDER])).to(DEV))))


def test_fit_score_with_the_full_set_and_the_roc_row(dataset, tmp_path):
    model_path, csv = tmp_path / "srm_full.npz", tmp_path / "srm_full.csv"
    common = ["--data", str(dataset), "--stego-methods", "SUNIWARD", "--alphas", "0.4", "--submodels", "full", "--simulate"]
    srm.main(["fit", *common, "--out", str(model_path)])
    model = srm.load(model_path, "full")
    assert (model.submodels, model.ridge, model.stego_methods, model.alphas) == ("full", 0.1, ["SUNIWARD"], [0.4]) and model.w.shape == (34671,)
    covers = torch.from_numpy(np.stack([_plane(f"cover_{k}.png") for k in ORDER])).to(DEV)
    twins = costs.simulate(covers, "SUNIWARD", 0.4, [embed.image_seed(f"{k}.png", 0) for k in ORDER])[0]
    F0, F1 = _full_features(covers), _full_features(twins)
    np.testing.assert_array_equal(model.w, srm.FLD(0.1, "full").fit(F0, F1).w)
    srm.main(["score", *common, "--model", str(model_path), "--out", str(csv)])
    df = pd.read_csv(csv, float_precision="round_trip")
    assert list(df.columns) == list(pd.read_csv(GOLDEN / "b0.csv").columns)
    folder = costs.folder_name("SUNIWARD", 0.4)
    assert df["name"].tolist() == [f"images/{k}.png" for k in ORDER] + [f"{folder}/{k}.png" for k in ORDER]
    assert np.abs(df["output"].to_numpy() - model.output(np.concatenate([F0, F1]))).max() <= 1e-12
    assert df["output"].between(0., 1.).all() and (df["prediction"] == (df["output"] > 0.5)).all()
    with pytest.raises(ValueError, match="not a model on the 'srm-all' features but on 'srm-full'"):
        srm.main(["score", *common[:-3], "--submodels", "all", "--simulate", "--model", str(model_path), "--out", str(tmp_path / "no.csv")])
    # ws.roc reads such a file as a detector: the same model on the data set's LSBR files, beside two WS filters
    csv = tmp_path / "srm_full_lsbr.csv"
    srm.main(["score", "--data", str(dataset), "--model", str(model_path), "--stego-methods", "LSBR", "--alphas", "0.1", "--submodels", "full",
              "--out", str(csv)])
    df = pd.read_csv(csv, float_precision="round_trip")
    scores = roc.load_scores(csv, "B0_SRM", ["LSBR"], [.1])
    assert len(scores) == 10 and (scores["model_name"] == "B0_SRM").all() and np.array_equal(scores["score"].to_numpy(), df["output"].to_numpy())
    out = tmp_path / "roc"
    roc.main(["--data", str(dataset), "--out-dir", str(out), "--stego-methods", "LSBR", "--alphas", "0.1", "--filters", "AVG", "KB",
              "--scores", str(csv), "B0_SRM"])
    auc = pd.read_csv(out / "auc_0.1.csv")
    assert sorted(auc["model_name"]) == ["AVG", "B0_SRM", "KB"] and auc["auc"].between(0., 1.).all()
    # once with the ensemble in the discriminant's place
    ens_path, csv = tmp_path / "srm_full_ens.npz", tmp_path / "srm_full_ens.csv"
    srm.main(["fit", *common, "--classifier", "ensemble", "--learners", "5", "--d-sub", "200", "--out", str(ens_path)])
    ens = srm.load_model(ens_path, "full")
    assert isinstance(ens, srm.Ensemble) and ens.submodels == "full"
    srm.main(["score", *common, "--model", str(ens_path), "--out", str(csv)])
    assert pd.read_csv(csv)["output"].between(0., 1.).all()
