"""CPU: the host side of the SRM min/max submodels (K50, ws_unet_amd/srm.py `features_minmax`): the table layout and its totals, the
restatement (srm_minmax_np) at its edges, the 325 orbits, the 13 000 / 16 718 layouts, the invariances the features have by
construction, the dual fit of the discriminant against the primal one, the model file's feature-set tag, the C entry's argument errors
(no GPU call is made) and the CLI parser."""
import itertools

import numpy as np
import pytest
import torch

import srm_minmax_np as mm_np
import srm_np
from ws_unet_amd import _lib, ops, spam, srm


def _bin(t):
    return sum((d + 2) * 5 ** (3 - k) for k, d in enumerate(t))


def _plane(h=24, w=31, seed=7):
    x = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    x[3:14, 5:20] //= 32                                                    # a smooth patch: small residuals, ties of the rounding
    x[16:22, 2:12] = 201
    return x


# ---- the table layout as data ---------------------------------------------------------------------------------------------------------

def test_table_layout_and_dimensions():
    assert len(ops.SRM_MINMAX_TABLES) == 118 == len(mm_np.TABLES)
    assert [t[:4] for t in ops.SRM_MINMAX_TABLES] == mm_np.TABLES
    assert [t[4:] for t in ops.SRM_MINMAX_TABLES] == [mm_np.ab(cls, name, scan) for cls, _, name, scan in mm_np.TABLES]
    first = {cls: min(i for i, t in enumerate(ops.SRM_MINMAX_TABLES) if t[0] == cls) for cls in ops.SRM_MINMAX_Q2}
    assert first == {"S1": 0, "S2": 28, "S3": 76}
    assert ops.SRM_MINMAX_Q2 == {"S1": (2, 4), "S2": (4, 6, 8), "S3": (6, 9, 12)}
    assert ops.SRM_MINMAX_TABLES[0] == ("S1", 2, "WE", "h", 0, 5) and ops.SRM_MINMAX_TABLES[1] == ("S1", 2, "WE", "v", 3, 2)
    assert ops.SRM_MINMAX_TABLES[7] == ("S1", 2, "WNE", "v", 4, 2) and ops.SRM_MINMAX_TABLES[28] == ("S2", 4, "hv", "h", 2, 5)
    assert ops.SRM_MINMAX_TABLES[80] == ("S3", 6, "WENS", "h", 4, 7) and ops.SRM_MINMAX_TABLES[117] == ("S3", 12, "NES", "v", 7, 3)
    # the stated reaches are those of the members' taps
    for cls, (_, _, sets) in mm_np.CLASSES.items():
        assert list(sets) == list(ops.SRM_MINMAX_SETS[cls])
        for name in sets:
            assert mm_np.reach(cls, name) == mm_np.REACH[cls][name] == ops.SRM_MINMAX_SETS[cls][name]
    assert srm.MINMAX_ORBITS == 325 == mm_np.ORBITS == (625 + 25) // 2 and len(srm.MINMAX_BLOCKS) == 40
    assert srm.MINMAX_DIM == 13000 == mm_np.DIM and srm.DIMS == {"linear": 3718, "minmax": 13000, "all": 16718}
    assert [b[:3] for b in srm.MINMAX_BLOCKS[:6]] == [("S1", 2, "22h"), ("S1", 2, "22v"), ("S1", 2, "24"), ("S1", 2, "34h"), ("S1", 2, "34v"),
                                                       ("S1", 4, "22h")]
    assert srm.MINMAX_BLOCKS[0][3] == (0, 3) and srm.MINMAX_BLOCKS[1][3] == (1, 2) and srm.MINMAX_BLOCKS[3][3] == (6, 8, 11, 13)
    assert srm.MINMAX_BLOCKS[10] == ("S2", 4, "21", (28, 29)) and srm.MINMAX_BLOCKS[12] == ("S2", 4, "32", (32, 33, 34, 35))
    assert srm.MINMAX_SUBMODELS == mm_np.SUBMODELS
    assert sorted(i for b in srm.MINMAX_BLOCKS for i in b[3]) == list(range(118))          # every table in exactly one submodel


def test_restatement_totals_small_images_and_hand_made_runs():
    for h, w in ((13, 17), (1, 1), (4, 7), (5, 8), (8, 5), (8, 8), (7, 30), (3, 40)):
        x = np.random.default_rng(h * w).integers(0, 256, (2, h, w), dtype=np.uint8)
        c = mm_np.counts(x)
        assert c.shape == (2, 118, 625) and c.dtype == np.int64
        assert c.sum(axis=2).tolist() == [mm_np.totals(h, w)] * 2
        assert mm_np.totals(h, w) == [2 * max(h - t[4], 0) * max(w - t[5], 0) for t in ops.SRM_MINMAX_TABLES]
        # brute force: a run counts when every pixel its set reads at its four positions lies in the image
        for k, (cls, _, name, scan) in enumerate(mm_np.TABLES):
            taps = [t for member in mm_np.CLASSES[cls][2][name] for t in mm_np.CLASSES[cls][1][member]]
            step = (0, 1) if scan == "h" else (1, 0)
            runs = sum(all(0 <= r + i * step[0] + dr < h and 0 <= cc + i * step[1] + dc < w for i in range(4) for dr, dc in taps)
                       for r in range(h) for cc in range(w))
            assert mm_np.totals(h, w)[k] == 2 * runs, (h, w, cls, name, scan)
    at = {t: i for i, t in enumerate(mm_np.TABLES)}
    t58, t85 = mm_np.totals(5, 8), mm_np.totals(8, 5)                         # exactly one run of S3 WENS scanned h, resp. v
    assert (t58[at["S3", 6, "WENS", "h"]], t58[at["S3", 6, "WENS", "v"]]) == (2, 0)
    assert (t85[at["S3", 6, "WENS", "h"]], t85[at["S3", 6, "WENS", "v"]]) == (0, 2)
    assert not any(mm_np.totals(1, 1)) and sum(1 for t in mm_np.totals(4, 7) if t) > 0
    # a constant plane: lo = hi = 0 everywhere, both updates in the centre bin
    c = mm_np.counts(np.full((1, 9, 11), 200, dtype=np.uint8))[0]
    assert c[:, 312].tolist() == mm_np.totals(9, 11) and c.sum() == sum(mm_np.totals(9, 11))
    # one bright pixel, S1 at q2 = 2, set WE scanned h in its row: around it E, W = (1, 0), (-1, -1), (0, 1): lo 0, -1, 0 and hi 1, -1, 1
    x = np.zeros((1, 1, 9), dtype=np.uint8)
    x[0, 0, 4] = 1
    c = mm_np.counts(x)[0, at["S1", 2, "WE", "h"]]
    want = np.zeros(625, dtype=np.int64)
    lo, hi = [0, 0, 0, -1, 0, 0, 0], [0, 0, 1, -1, 1, 0, 0]                    # columns 1 .. 7
    for i in range(4):
        want[_bin(lo[i:i + 4])] += 1
        want[_bin([-d for d in hi[i:i + 4]])] += 1
    np.testing.assert_array_equal(c, want)


def test_digit_of_the_minimum_is_the_minimum_of_the_digits():
    R = np.random.default_rng(0).integers(-800, 801, (4, 5000))
    R[:, :200] = np.random.default_rng(1).integers(-14, 15, (4, 200))         # around the ties
    for q2 in sorted({q for steps in ops.SRM_MINMAX_Q2.values() for q in steps}):
        D = srm_np.digit(R, q2)
        np.testing.assert_array_equal(srm_np.digit(R.min(axis=0), q2), D.min(axis=0))
        np.testing.assert_array_equal(srm_np.digit(R.max(axis=0), q2), D.max(axis=0))
        np.testing.assert_array_equal(srm_np.digit(-R, q2), -D)                # the digit is odd


# ---- orbits and features ------------------------------------------------------------------------------------------------------------------

def test_reversal_orbits():
    orbits = mm_np.orbits()
    assert len(orbits) == 325 and sorted(b for o in orbits for b in o) == list(range(625))
    assert [min(o) for o in orbits] == sorted(min(o) for o in orbits)
    for k, o in enumerate(orbits):
        for b in o:
            assert srm._MINMAX_ORBIT[b] == k
    assert sorted(len(o) for o in orbits).count(1) == 25
    assert srm._MINMAX_FOLD.shape == (625, 325) and (srm._MINMAX_FOLD.sum(axis=1) == 1).all()
    assert srm._MINMAX_FOLD.sum(axis=0).tolist() == [len(o) for o in orbits]


def test_features_against_the_restatement():
    c = np.random.default_rng(2).integers(0, 1000, (3, 118, 625)).astype(np.int64)
    c[1, :, :300] = 0
    c[2] = 0
    c[2, :, 312] = 777
    want = mm_np.features(c)
    for got in (srm.features_minmax(c), srm.features_minmax(torch.from_numpy(c))):
        assert got.dtype == np.float64 and got.shape == (3, 13000)
        np.testing.assert_array_equal(got, want)
    blocks = want.reshape(3, 40, 325)
    np.testing.assert_allclose(blocks.sum(axis=2), 1., rtol=0, atol=1e-12)
    assert (blocks[2, :, srm._MINMAX_ORBIT[312]] == 1.).all() and np.count_nonzero(blocks[2]) == 40
    cx = mm_np.counts(np.stack([_plane(), _plane(seed=8)]))
    np.testing.assert_array_equal(srm.features_minmax(cx), mm_np.features(cx))
    for bad in (c[0], c[:, :117], c[:, :, :624], np.zeros((1, 44, 625), dtype=np.int64)):
        with pytest.raises(ValueError, match="expected"):
            srm.features_minmax(bad)


def test_features_are_invariant_under_d4_and_negation_of_the_image():
    """transposing the image, mirroring it left-right or top-bottom and x -> 255 - x permute the sets, swap lo with hi and reverse the
    runs, all of which the tables' symmetrisation, the submodels' sums and the fold over reversal absorb: exactly equal features"""
    x = _plane()
    F = srm.features_minmax(mm_np.counts(x[None]))
    assert F.shape == (1, 13000)
    for name, y in (("transpose", x.T), ("left-right", x[:, ::-1]), ("top-bottom", x[::-1]), ("negation", 255 - x), ("rot180", x[::-1, ::-1]),
                    ("rot90", x.T[::-1])):
        G = srm.features_minmax(mm_np.counts(np.ascontiguousarray(y)[None]))
        np.testing.assert_array_equal(G, F, err_msg=name)
    assert not np.array_equal(srm.features_minmax(mm_np.counts(np.roll(x, 1, axis=1)[None])), F)


def test_features_refuse_a_submodel_without_a_run():
    c = np.ones((2, 118, 625), dtype=np.int64)
    c[1, [76, 79]] = 0                                                       # S3 q2 = 6, 22h = WE.h + NS.v
    with pytest.raises(ValueError, match="image 1.*S3.*22h"):
        srm.features_minmax(c)
    c[1, 76] = 1                                                             # one of the submodel's tables is enough
    assert srm.features_minmax(c).shape == (2, 13000)
    with pytest.raises(ValueError, match="image 0"):                         # four rows: no vertical run of a third-order set
        srm.features_minmax(mm_np.counts(np.zeros((1, 4, 30), dtype=np.uint8)))
    with pytest.raises(ValueError, match="without a run"):
        mm_np.features(mm_np.counts(np.zeros((1, 4, 30), dtype=np.uint8)))


def test_default_submodels_leave_the_linear_path_as_it_was():
    c = np.random.default_rng(9).integers(0, 50, (2, 44, 625)).astype(np.int64)
    assert srm._COUNTS["linear"] == ("srm_counts",) and srm._FEATURES["srm_counts"] is srm.features
    assert srm._COUNTS["all"] == ("srm_counts", "srm_minmax_counts") and srm._COUNTS["minmax"] == ("srm_minmax_counts",)
    assert srm.features(c).tobytes() == srm_np.features(c).tobytes()
    assert srm.FLD().submodels == "linear" and srm.FLD().dual is False and srm.FEATURE_SETS["linear"] == srm.FEATURE_SET == "srm-linear"
    rng = np.random.default_rng(4)
    X0, X1 = rng.random((6, 3718)), rng.random((5, 3718)) + 0.01
    w, b = srm_np.fld_fit(X0, X1, 0.25)                                      # fewer rows than features, and still the primal solve's bits
    m = srm.FLD(0.25).fit(X0, X1)
    assert m.w.tobytes() == w.tobytes() and m.b == b
    with pytest.raises(ValueError, match="unknown submodels"):
        srm.FLD(submodels="nonlinear")
    with pytest.raises(ValueError, match="unknown submodels"):
        srm.extract("nowhere", submodels="some")


# ---- the dual fit -----------------------------------------------------------------------------------------------------------------------------

def test_dual_fit_equals_the_primal_fit():
    """650 features (two submodels' worth) of restated counts on 192 rows, ridge 0.1: w and b of the n x n dual against the d x d primal
    within 1e-9 relative (measured 5.8e-14; the margin is for another LAPACK); with more rows than features, or ridge 0, `fit` stays primal"""
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, (192, 16, 16), dtype=np.uint8)
    x[:96] //= 16
    y = x ^ rng.integers(0, 2, x.shape, dtype=np.uint8)
    F0, F1 = (srm.features_minmax(mm_np.counts(v))[:, 325:975] for v in (x, y))
    primal = spam.FLD(0.1).fit(F0, F1)
    dual = spam.FLD(0.1)
    dual.dual = True
    dual.fit(F0, F1)
    assert not np.array_equal(dual.w, primal.w)                               # another arithmetic, ...
    rel = np.linalg.norm(dual.w - primal.w) / np.linalg.norm(primal.w)
    print(f"dual against primal: relative difference of w {rel:.3e}, of b {abs(dual.b - primal.b) / abs(primal.b):.3e}")
    assert rel <= 1e-9 and abs(dual.b - primal.b) <= 1e-9 * abs(primal.b)     # ... the same discriminant
    wide = spam.FLD(0.1)
    wide.dual = True
    assert wide.fit(F0[:, :300], F1[:, :300]).w.tobytes() == spam.FLD(0.1).fit(F0[:, :300], F1[:, :300]).w.tobytes()   # 384 rows >= 300 features
    with pytest.raises(ValueError, match="no within-class variance"):
        dual.fit(np.ones((3, 650)), np.zeros((2, 650)))
    # srm.FLD takes the dual for its two larger sets: 16 718 features on a handful of rows without a 16 718 x 16 718 matrix
    rows0, rows1 = rng.random((7, 16718)), rng.random((6, 16718)) + 0.02
    m = srm.FLD(0.1, "all").fit(rows0, rows1)
    assert m.dual and m.w.shape == (16718,) and np.isfinite(m.w).all()
    assert (m.output(rows1) > 0.5).all() and (m.output(rows0) < 0.5).all()
    with pytest.raises(ValueError, match="13000"):
        srm.FLD(0.1, "minmax").fit(rows0, rows1)


# ---- the model file ---------------------------------------------------------------------------------------------------------------------------

def test_model_tag_round_trip_and_refusal(tmp_path):
    rng = np.random.default_rng(5)
    paths = {}
    for sub, tag in (("linear", "srm-linear"), ("minmax", "srm-minmax"), ("all", "srm-all")):
        d = srm.DIMS[sub]
        m = srm.FLD(0.2, sub).fit(rng.random((5, d)), rng.random((4, d)) + 0.01)
        m.stego_methods, m.alphas = ["SUNIWARD"], [0.4]
        paths[sub] = tmp_path / f"{sub}.npz"
        m.save(paths[sub])
        with np.load(paths[sub], allow_pickle=False) as z:
            assert str(z["features"]) == tag and z["w"].shape == (d,)
            assert sorted(z.files) == sorted(["w", "b", "ridge", "features", "order", "T", "q2_S1", "q2_S2", "q2_S3", "q2_S3x3", "q2_S5x5",
                                              "stego_methods", "alphas"])
        for r in (srm.load(paths[sub]), srm.load(paths[sub], sub), srm.FLD.load(paths[sub], submodels=sub)):
            assert r.submodels == sub and r.dual == (sub != "linear") and (r.ridge, r.stego_methods, r.alphas) == (0.2, ["SUNIWARD"], [0.4])
            np.testing.assert_array_equal(r.w, m.w)
            assert r.b == m.b
    for have, asked in itertools.permutations(paths, 2):
        with pytest.raises(ValueError, match=f"not a model on the 'srm-{asked}' features but on 'srm-{have}'"):
            srm.load(paths[have], asked)
    with pytest.raises(ValueError, match="unknown submodels"):
        srm.load(paths["all"], "everything")
    with pytest.raises(Exception):                                          # SPAM's loader takes none of them
        spam.FLD.load(paths["minmax"])
    model = srm.load(paths["minmax"])
    with pytest.raises(ValueError, match="'srm-minmax' features, not on 'srm-all'"):       # before any file of the data set is read
        srm.score(tmp_path / "no_data", model, ["LSBR"], [0.1], submodels="all")
    with pytest.raises(ValueError, match="'srm-minmax' features, not on 'srm-linear'"):
        srm.score(tmp_path / "no_data", model, ["LSBR"], [0.1])
    model.w = model.w[:3718]
    model.save(tmp_path / "short.npz")
    with pytest.raises(ValueError, match="3718 weights, expected 13000"):
        srm.load(tmp_path / "short.npz")


# ---- the C entry's argument errors: errno-style code + message before any HIP call ------------------------------------------------------

def test_c_entry_rejects_bad_arguments_without_a_gpu():
    assert _lib.SIGNATURES["wsu_srm_minmax_counts"] == _lib.SIGNATURES["wsu_srm_counts"]
    lib = _lib.load()
    err = lib.wsu_last_error

    def call(x=8, counts=8, n=1, h=8, w=8):
        return lib.wsu_srm_minmax_counts(x, counts, n, h, w, None)
    assert call(x=None) == -1 and b"null" in err() and b"srm_minmax_counts" in err()
    assert call(counts=None) == -1 and b"null" in err()
    assert call(n=0) == -1 and b"bad shape" in err()
    assert call(n=65536) == -1 and b"bad shape" in err()
    assert call(h=0) == -1 and b"bad shape" in err()
    assert call(w=0) == -1 and b"bad shape" in err()
    assert call(h=2 ** 31 - 1, w=2 ** 31 - 1) == -1 and b"too many tiles" in err()
    with pytest.raises(_lib.WsuError, match="CPU tensor"):                   # a valid call gets as far as the device check
        ops.srm_minmax_counts(torch.zeros((1, 8, 8), dtype=torch.uint8))


def test_cli_parser_takes_submodels():
    a = srm.parse_args(["fit", "--data", "d", "--alphas", ".4", "--out", "m.npz"])
    assert a.submodels == "linear"
    a = srm.parse_args(["fit", "--data", "d", "--alphas", ".4", "--submodels", "all", "--simulate", "--stego-methods", "SUNIWARD", "--out", "m.npz"])
    assert (a.submodels, a.simulate, a.stego_methods) == ("all", True, ["SUNIWARD"])
    for cmd in (["score", "--model", "m.npz"], ["features"]):
        assert srm.parse_args(cmd + ["--data", "d", "--alphas", ".1", "--submodels", "minmax", "--out", "o"]).submodels == "minmax"
    with pytest.raises(SystemExit):
        srm.parse_args(["fit", "--data", "d", "--alphas", ".4", "--submodels", "nonlinear", "--out", "m.npz"])
