"""GPU: the segment histograms (K58), the adjacency histogram (K59) and the 2 x 2 calibration image (K60) bit for bit against numpy
(histogram_np), and the drivers of ws_unet_amd.histogram -- the five detectors, the chi-square curve and its length estimate, the score file
and its row in the ROC tables -- against the restated statistics on the five fixture covers."""
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import histogram_np
from ws_unet_amd import embed, embed_pm1, histogram, ops, spam
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import roc

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
ORDER = (10, 6, 7, 8, 9)                  # the order in which fabrika lists the files


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


def _dev(x):
    return torch.from_numpy(np.array(x, order="C", copy=True)).to(DEV)                  # (a copy: a flipped view has negative strides)


def _seg(x, segments=1, order="rows"):
    return ops.hist_segments(_dev(x), segments, order).cpu().numpy()


def _adj(x):
    return ops.adjacency_hist(_dev(x)).cpu().numpy()


def _down(x):
    return ops.downsample2x2(_dev(x)).cpu().numpy()


def _random(shape):
    return np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)


def _checkerboard(shape):
    rr, cc = np.indices(shape[1:])
    return np.broadcast_to(((rr + cc) % 2 * 255).astype(np.uint8), shape).copy()


@pytest.fixture(scope="module")
def covers():
    """the five covers in fabrika's order"""
    return np.stack([_plane(f"cover_{k}.png") for k in ORDER])


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the five golden covers and their LSBR alpha 1.0 stegos as a data set"""
    root = tmp_path_factory.mktemp("histogram_data")
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


# ---- K58 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", histogram_np.ORDERS)
@pytest.mark.parametrize("shape,segments", [((1, 1, 1), 1), ((1, 1, 5), 3), ((1, 2, 3), 8), ((2, 3, 5), 4), ((1, 16, 300), 7), ((1, 67, 259), 100),
                                            ((2, 131, 40), 256)])
def test_hist_segments_equal_numpy_bit_for_bit(shape, segments, order):
    """one pixel; segments of unequal length; empty segments (S > H W); a batch; a ragged last strip; an odd width (rows off the 16-byte
    grid) with rows one past two row tiles and two chunks' worth of segments; segments of 20.5 pixels, many to a workgroup"""
    x = _random(shape)
    got = _seg(x, segments, order)
    n, h, w = shape
    assert got.dtype == np.int64 and got.shape == (n, segments, 256)
    np.testing.assert_array_equal(got, histogram_np.seg_hist(x, segments, order))
    np.testing.assert_array_equal(got.sum(axis=2), np.broadcast_to(histogram_np.seg_lengths(h, w, segments), (n, segments)))
    np.testing.assert_array_equal(_seg(x, segments, "rows_up"), _seg(x[:, ::-1], segments, "rows"))


@pytest.mark.parametrize("segments", [1, 100])
def test_hist_segments_of_value_patterns(segments):
    """a constant plane sends every update of a workgroup to one bin; so do all 0 and all 255, the ends of the table; a 0 / 255
    checkerboard alternates between them"""
    shape = (1, 512, 512)
    for name, x in (("constant 77", np.full(shape, 77, dtype=np.uint8)), ("all 0", np.zeros(shape, dtype=np.uint8)),
                    ("all 255", np.full(shape, 255, dtype=np.uint8)), ("checkerboard", _checkerboard(shape))):
        for order in histogram_np.ORDERS:
            np.testing.assert_array_equal(_seg(x, segments, order), histogram_np.seg_hist(x, segments, order), err_msg=f"{name} {order}")
    got = _seg(np.full(shape, 77, dtype=np.uint8), segments)
    np.testing.assert_array_equal(got[0, :, 77], histogram_np.seg_lengths(512, 512, segments))


def test_hist_segments_of_natural_images_and_the_largest_table():
    x = np.stack([_plane("cover_6.png"), _plane("stego_LSBR_1.0_7.png")])
    for order in histogram_np.ORDERS:
        np.testing.assert_array_equal(_seg(x, 100, order), histogram_np.seg_hist(x, 100, order))
    np.testing.assert_array_equal(_seg(x[:1, :70, :90], 4096), histogram_np.seg_hist(x[:1, :70, :90], 4096))
    np.testing.assert_array_equal(_seg(x, 100).cumsum(1)[:, -1], _seg(x)[:, 0])          # the last prefix is the plain histogram


def test_hist_segments_argument_errors():
    x = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="outside 1..4096"):
            ops.hist_segments(x, bad)
    with pytest.raises(ValueError, match="unknown order"):
        ops.hist_segments(x, 4, "columns")
    with pytest.raises(ValueError, match="no images"):
        ops.hist_segments(x[:0], 4)
    with pytest.raises(Exception, match="contiguous"):
        ops.hist_segments(torch.zeros((1, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2])


# ---- K59 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 2), (2, 3, 5), (1, 16, 300), (1, 67, 259), (2, 131, 40)])
def test_adjacency_hist_equals_numpy_bit_for_bit(shape):
    """no pair: all zero; one pair; a batch; a ragged last strip; an odd width; rows past one row tile in a batch"""
    x = _random(shape)
    got = _adj(x)
    n, h, w = shape
    assert got.dtype == np.int64 and got.shape == (n, 256, 256)
    np.testing.assert_array_equal(got, histogram_np.adjacency(x))
    assert (got.sum(axis=(1, 2)) == h * (w - 1)).all()
    np.testing.assert_array_equal(_adj(x[..., ::-1]), got.transpose(0, 2, 1))
    if w == 1:
        assert not got.any()


def test_adjacency_hist_of_value_patterns():
    """a constant (1,130,512) plane: 66 430 pairs in one bin, past any 16-bit field; a constant 512 x 512 plane; a 0 / 255 checkerboard:
    two bins far from the diagonal; the ramp x[r,c] = c mod 256: the bins (v, v+1) and (255, 0); uniform noise: no two neighbouring updates
    share a bin"""
    const = np.full((1, 130, 512), 77, dtype=np.uint8)
    got = _adj(const)
    assert got[0, 77, 77] == 130 * 511 == 66430 and got.sum() == 66430
    big = _adj(np.full((1, 512, 512), 200, dtype=np.uint8))
    assert big[0, 200, 200] == 512 * 511 == big.sum()
    board = _checkerboard((1, 512, 512))
    got = _adj(board)
    np.testing.assert_array_equal(got, histogram_np.adjacency(board))
    assert got[0, 0, 255] + got[0, 255, 0] == 512 * 511 and abs(int(got[0, 0, 255]) - int(got[0, 255, 0])) <= 512
    ramp = np.broadcast_to((np.arange(600) % 256).astype(np.uint8), (1, 40, 600)).copy()
    got = _adj(ramp)
    np.testing.assert_array_equal(got, histogram_np.adjacency(ramp))
    assert got[0, 255, 0] == 2 * 40 and got[0, 3, 4] == 3 * 40 and got[0, 100, 101] == 2 * 40
    noise = np.random.default_rng(59).integers(0, 256, (1, 512, 512), dtype=np.uint8)
    np.testing.assert_array_equal(_adj(noise), histogram_np.adjacency(noise))


def test_adjacency_hist_of_natural_images_and_a_mixed_batch():
    """two fixture planes; then a constant, a noise and a natural plane in one batch: a workgroup of one image must not leak into the next"""
    x = np.stack([_plane("cover_9.png"), _plane("stego_LSBR_1.0_10.png")])
    np.testing.assert_array_equal(_adj(x), histogram_np.adjacency(x))
    mixed = np.stack([np.full((512, 512), 77, dtype=np.uint8), np.random.default_rng(60).integers(0, 256, (512, 512), dtype=np.uint8), x[0]])
    got = _adj(mixed)
    np.testing.assert_array_equal(got, histogram_np.adjacency(mixed))
    assert got[0].sum() == got[0, 77, 77] == 512 * 511


def test_tables_are_zeroed_by_the_call_and_repeat_bit_for_bit():
    xn = _random((3, 70, 90))
    x = _dev(xn)
    lib = ops._lib.load()
    seg = torch.ones((3, 5, 256), dtype=torch.int64, device=DEV)                      # dirty buffers, used twice
    adj = torch.ones((3, 256, 256), dtype=torch.int64, device=DEV)
    for _ in range(2):
        ops.check(lib.wsu_hist_segments(x.data_ptr(), seg.data_ptr(), 3, 70, 90, 5, 1, ops._stream()), "wsu_hist_segments")
        ops.check(lib.wsu_adjacency_hist(x.data_ptr(), adj.data_ptr(), 3, 70, 90, ops._stream()), "wsu_adjacency_hist")
        np.testing.assert_array_equal(seg.cpu().numpy(), histogram_np.seg_hist(xn, 5, "rows_up"))
        np.testing.assert_array_equal(adj.cpu().numpy(), histogram_np.adjacency(xn))
    assert lib.wsu_hist_segments(x.data_ptr(), seg.data_ptr(), 3, 70, 90, 4097, 0, ops._stream()) == -1 and b"segments=4097" in lib.wsu_last_error()


# ---- K60 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 2, 2), (1, 3, 3), (2, 5, 7), (1, 66, 258), (1, 67, 259)])
def test_downsample2x2_equals_numpy(shape):
    """one block; an odd row and column dropped; a batch with both; more than one workgroup across and down; the same with odd sizes, so
    that no row starts on the 8-byte grid"""
    x = _random(shape)
    got = _down(x)
    assert got.dtype == np.uint8 and got.shape == (shape[0], shape[1] // 2, shape[2] // 2)
    np.testing.assert_array_equal(got, histogram_np.downsample(x))


def test_downsample2x2_rounds_down_and_keeps_the_range():
    assert _down(np.array([[[255, 255], [255, 254]]], dtype=np.uint8)).tolist() == [[[254]]]
    assert (_down(np.full((1, 64, 64), 255, dtype=np.uint8)) == 255).all()
    x = _plane("cover_8.png")[None]
    np.testing.assert_array_equal(_down(x), histogram_np.downsample(x))
    np.testing.assert_array_equal(_down(x[:, 1:, 3:]), histogram_np.downsample(x[:, 1:, 3:]))
    for shape in ((1, 1, 5), (1, 5, 1)):
        with pytest.raises(ValueError, match="too small"):
            ops.downsample2x2(torch.zeros(shape, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="no images"):
        ops.downsample2x2(torch.zeros((0, 4, 4), dtype=torch.uint8, device=DEV))


# ---- the detectors ------------------------------------------------------------------------------------------------------------------

def test_outputs_equal_the_restated_scores(covers):
    x = _dev(covers)
    for detector in histogram.DETECTORS:
        got = histogram.outputs(x, detector)
        want = np.array([histogram_np.output(p, detector) for p in covers])
        print(f"{detector}: device {got}, restated {want}")
        assert got.dtype == np.float64 and got.shape == (5,)
        assert (np.abs(got - want) <= 1e-9 * np.abs(want)).all(), detector


def test_chi2_tells_full_lsb_replacement_from_the_covers(covers):
    """the whole-image p-value: below 1e-9 on the five covers (restated: at most 1.05e-12), above 0.99 on the five golden full-payload
    LSBR stegos (restated: at least 0.99997)"""
    stegos = np.stack([_plane(f"stego_LSBR_1.0_{k}.png") for k in ORDER])
    p0, p1 = histogram.outputs(_dev(covers), "CHI2"), histogram.outputs(_dev(stegos), "CHI2")
    print(f"CHI2 covers {p0}, LSBR 1.0 {p1}")
    assert (p0 < 1e-9).all() and (p1 > 0.99).all()


def test_hcf_falls_under_lsb_matching(covers):
    """C(h) of the plain histogram falls under LSBM at alpha 1 on at least four of the five covers (a numpy prototype gave four: cover 6
    rises by 0.02)"""
    x = _dev(covers)
    twins = embed_pm1.simulate(x, "LSBM", 1.0, [embed.image_seed(f"{k}.png", 0) for k in ORDER])[0]
    c0, c1 = -histogram.outputs(x, "HCF"), -histogram.outputs(twins, "HCF")
    print(f"C(h) covers {c0}, LSBM 1.0 {c1}")
    np.testing.assert_allclose(c1, [histogram_np.com(histogram_np.seg_hist(p)[0]) for p in twins.cpu().numpy()], rtol=1e-9)
    assert (c1 < c0).sum() >= 4


# ---- the drivers ------------------------------------------------------------------------------------------------------------------

def test_curves_and_the_length_estimate(dataset, covers):
    """order 'rows', S = 100: the covers have length <= 0.05 (restated: 0 to 0.04); LSBRS twins at alpha 0.1 / 0.3 / 0.6 have
    length >= alpha - 0.01 (the attack overestimates, which is known).  The bounds are checked on the restatement first."""
    cov = histogram.curves(dataset)
    pcols = [f"p_{j}" for j in range(100)]
    assert list(cov.columns) == ["name", "height", "width", "stego_method", "alpha", "length"] + pcols
    assert cov["name"].tolist() == [f"images/{k}.png" for k in ORDER] and cov["stego_method"].isna().all()
    want = np.stack([histogram_np.curve(p) for p in covers])
    want_len = histogram_np.length(want)
    print(f"covers: length device {cov['length'].tolist()}, restated {want_len.tolist()}")
    assert (want_len <= 0.05).all()
    np.testing.assert_allclose(cov[pcols].to_numpy(), want, rtol=1e-9, atol=1e-300)
    np.testing.assert_array_equal(cov["length"].to_numpy(), want_len)
    seeds = [embed.image_seed(f"{k}.png", 0) for k in ORDER]
    for alpha in (0.1, 0.3, 0.6):
        twins = embed.simulate(_dev(covers), "LSBRS", alpha, seeds, order="rows")[0].cpu().numpy()
        want = np.stack([histogram_np.curve(p) for p in twins])
        want_len = histogram_np.length(want)
        res = histogram.curves(dataset, "LSBRS", alpha, simulate=True)
        print(f"LSBRS {alpha}: length device {res['length'].tolist()}, restated {want_len.tolist()}")
        assert (want_len >= alpha - 0.01).all()
        assert res["name"].tolist() == [f"{embed.folder_name('LSBRS', alpha)}/{k}.png" for k in ORDER]
        assert (res["stego_method"] == "LSBRS").all() and (res["alpha"] == alpha).all()
        np.testing.assert_allclose(res[pcols].to_numpy(), want, rtol=1e-9, atol=1e-300)
        np.testing.assert_array_equal(res["length"].to_numpy(), want_len)
    # the stego folder of the data set, read from its files, bottom-up and with fewer segments
    res = histogram.curves(dataset, "LSBR", 1.0, segments=7, order="rows_up", batch_size=2)
    want = np.stack([histogram_np.curve(_plane(f"stego_LSBR_1.0_{k}.png"), 7, "rows_up") for k in ORDER])
    assert res["name"].tolist() == [f"stego_LSBR_alpha_1.0/{k}.png" for k in ORDER] and len(res.columns) == 6 + 7
    np.testing.assert_allclose(res[[f"p_{j}" for j in range(7)]].to_numpy(), want, rtol=1e-9, atol=1e-300)
    assert (res["length"] == 1.0).all()
    with pytest.raises(ValueError, match="simulate=True makes"):
        histogram.curves(dataset, "LSBRK", 0.1, simulate=True)


def test_score_file_and_its_row_in_the_roc_tables(dataset, covers, tmp_path):
    csv = tmp_path / "scores.csv"
    histogram.main(["score", "--data", str(dataset), "--detector", "HCF2C", "--stego-methods", "LSBM", "--alphas", "1.0", "--simulate", "--out", str(csv)])
    df = pd.read_csv(csv, float_precision="round_trip")
    assert list(df.columns) == spam.CSV_COLUMNS == list(pd.read_csv(GOLDEN / "b0.csv").columns)
    assert len(df) == 10 and df["stego_method"][:5].isna().all() and (df["stego_method"][5:] == "LSBM").all() and (df["alpha"][5:] == 1.0).all()
    assert df["name"].tolist() == [f"images/{k}.png" for k in ORDER] + [f"{embed_pm1.folder_name('LSBM', 1.0)}/{k}.png" for k in ORDER]
    twins = embed_pm1.simulate(_dev(covers), "LSBM", 1.0, [embed.image_seed(f"{k}.png", 0) for k in ORDER])[0].cpu().numpy()
    want = np.array([histogram_np.output(p, "HCF2C") for p in list(covers) + list(twins)])
    print(f"HCF2C covers {df['output'][:5].tolist()}, LSBM 1.0 {df['output'][5:].tolist()}")
    np.testing.assert_allclose(df["output"].to_numpy(), want, rtol=1e-9)
    assert (df["prediction"] == (df["output"] > 1.0)).all()
    scores = roc.load_scores(csv, "B0_HCF2C", ["LSBM"], [1.0])
    assert len(scores) == 10
    scores["stego_method"] = scores["stego_method"].fillna("Cover")
    frame = roc.produce_roc(scores)                                         # what ws.roc's main makes of a --scores file
    auc = roc.auc_table(frame)
    assert len(frame) == len(roc.TAUS) and auc["model_name"].tolist() == ["B0_HCF2C"] and auc["stego_method"].tolist() == ["LSBM"]
    # the stego folder read from its files, and the conventions of `prediction`
    df = histogram.score(dataset, "CHI2", ["LSBR"], [1.0], batch_size=3)
    assert list(df.columns) == spam.CSV_COLUMNS and df["name"].tolist()[5:] == [f"stego_LSBR_alpha_1.0/{k}.png" for k in ORDER]
    assert df["prediction"].tolist() == [False] * 5 + [True] * 5 and (df["output"][:5] < 1e-9).all() and (df["output"][5:] > 0.99).all()
    df = histogram.score(dataset, "HCF", ["LSBR"], [1.0])
    assert not df["prediction"].any() and (df["output"] < 0).all()


def test_curves_read_lsbrs_files_from_the_folder_of_their_order(dataset, tmp_path):
    """top-down and bottom-up LSBRS twins differ in their folder only: `curves` reads the one written for its order, and gets what
    simulate=True gets"""
    root = tmp_path / "data"
    shutil.copytree(dataset, root)
    for order in histogram_np.ORDERS:
        embed.write_dataset(root, "LSBRS", [0.3], order=order)
    pcols = [f"p_{j}" for j in range(20)]
    for order in histogram_np.ORDERS:
        res = histogram.curves(root, "LSBRS", 0.3, segments=20, order=order)
        sim = histogram.curves(root, "LSBRS", 0.3, segments=20, order=order, simulate=True)
        assert res["name"].tolist() == [f"{embed.folder_name('LSBRS', 0.3, order)}/{k}.png" for k in ORDER] == sim["name"].tolist()
        np.testing.assert_array_equal(res[pcols].to_numpy(), sim[pcols].to_numpy())
        assert (res["length"] >= 0.29).all()
