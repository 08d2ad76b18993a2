"""CPU: the host side of the SRM detector (K49, ws_unet_amd/srm.py): the orbit table against enumeration, `features` against the numpy
restatement (srm_np) and under both symmetries, the 3 718 layout, the digit formula at its ties, the restatement's totals, the model
file, the C entry's argument errors (no GPU call is made) and the CLI parser."""
import itertools

import numpy as np
import pytest
import torch

import srm_np
from ws_unet_amd import _lib, ops, spam, srm


def _image(h=13, w=17, seed=5):
    x = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    x[2:9, 3:12] = 90
    x[10] = np.arange(w, dtype=np.uint8) * 2
    x[0, :4] = (0, 255, 0, 255)
    return x


def _counts(seed=1, n=3):
    c = np.random.default_rng(seed).integers(0, 1000, (n, 44, 625)).astype(np.int64)
    c[1, :, :300] = 0
    c[2] = 0
    c[2, :, 312] = 12345                                                     # a constant plane: everything in the centre bin
    return c


def _digits(b):
    return tuple(b // 5 ** (3 - k) % 5 - 2 for k in range(4))


def _bin(t):
    return sum((d + 2) * 5 ** (3 - k) for k, d in enumerate(t))


# ---- the table layout as data ---------------------------------------------------------------------------------------------------------

def test_table_layout_equals_the_restated_one():
    assert len(ops.SRM_TABLES) == 44 == len(srm_np.TABLES) and (ops.SRM_T, ops.SRM_ORDER, ops.SRM_BINS) == (2, 4, 625)
    assert [t[:4] for t in ops.SRM_TABLES] == srm_np.TABLES
    assert [t[4:] for t in ops.SRM_TABLES] == [srm_np.REACH[cls][res + scan] for cls, _, res, scan in srm_np.TABLES]
    first = {cls: min(i for i, t in enumerate(ops.SRM_TABLES) if t[0] == cls) for cls in ops.SRM_Q2}
    assert first == {"S1": 0, "S2": 8, "S3": 20, "S3x3": 32, "S5x5": 38}
    assert ops.SRM_TABLES[0] == ("S1", 2, "h", "h", 0, 4) and ops.SRM_TABLES[43] == ("S5x5", 48, "n", "v", 7, 4)
    assert ops.SRM_TABLES[9] == ("S2", 4, "h", "v", 3, 2) and ops.SRM_TABLES[34] == ("S3x3", 12, "n", "h", 2, 5)
    assert srm.DIM == 3718 == srm_np.DIM == 8 * 338 + 6 * 169 and len(srm.BLOCKS) == 22
    assert [b[:3] for b in srm.BLOCKS[:3]] == [("S1", 2, "par"), ("S1", 2, "perp"), ("S1", 4, "par")]
    assert srm.BLOCKS[0][3] == (0, 3) and srm.BLOCKS[1][3] == (1, 2) and srm.BLOCKS[16] == ("S3x3", 8, "n", (32, 33)) and srm.BLOCKS[21][3] == (42, 43)


def test_restatement_totals_and_small_images():
    for h, w in ((13, 17), (1, 1), (4, 4), (5, 8), (8, 5), (8, 8), (7, 30)):
        x = np.random.default_rng(h * w).integers(0, 256, (2, h, w), dtype=np.uint8)
        c = srm_np.counts(x)
        assert c.shape == (2, 44, 625) and c.dtype == np.int64
        assert c.sum(axis=2).tolist() == [srm_np.totals(h, w)] * 2
    assert srm_np.totals(512, 512)[:2] == [512 * 508, 509 * 511] and 512 * 508 == 260096 and 509 * 511 == 260099
    t44 = srm_np.totals(4, 4)                                               # 4 x 4: only a difference scanned across its own direction has a run
    assert t44[:4] == [0, 3, 3, 0] and not any(t44[32:]) and sum(1 for t in t44 if t) == 16
    assert [srm_np.totals(5, 8)[i] for i in (38, 39)] == [1, 0] and [srm_np.totals(8, 5)[i] for i in (38, 39)] == [0, 1]
    # a constant plane: every run in the centre bin
    c = srm_np.counts(np.full((1, 9, 11), 200, dtype=np.uint8))[0]
    assert c[:, 312].tolist() == srm_np.totals(9, 11) and c.sum() == sum(srm_np.totals(9, 11))
    # one hand-made run: the 3x3 kernel on a single bright pixel, scanned h, at q2 = 8 (q = 4): residuals 2,-4,2 and digits 1,-1,1 around it
    x = np.zeros((1, 3, 7), dtype=np.uint8)
    x[0, 1, 3] = 1
    c = srm_np.counts(x)[0, 32]
    assert c.sum() == 2 and c[_bin((0, 1, -1, 1))] == 1 and c[_bin((1, -1, 1, 0))] == 1


def test_digit_formula_and_its_ties():
    R = np.arange(-3100, 3101)
    for steps in ops.SRM_Q2.values():
        for q2 in steps:
            want = np.sign(R) * np.minimum(np.floor(np.abs(R) / (q2 / 2) + 0.5), 2)
            np.testing.assert_array_equal(srm_np.digit(R, q2), want.astype(np.int64))
    assert srm_np.digit(np.array([-1, 1, -2, 2, -3, 3, 0]), 2).tolist() == [-1, 1, -2, 2, -2, 2, 0]              # q = 1
    assert srm_np.digit(np.array([-1, 1, -2, 2, -3, 3, -4, 4, -5, 5]), 4).tolist() == [-1, 1, -1, 1, -2, 2, -2, 2, -2, 2]   # q = 2: ties at 1, 3
    assert srm_np.digit(np.array([2, 3, 6, 7, -2, -3, -6, -7]), 9).tolist() == [0, 1, 1, 2, 0, -1, -1, -2]      # q = 4.5: 2.25 and 6.75 are the edges


# ---- orbits and features ------------------------------------------------------------------------------------------------------------------

def test_orbit_table():
    orbits = srm_np.orbits()
    assert len(orbits) == 169 == srm.ORBITS == (625 + 1 + 25 + 25) // 4
    assert sorted(b for o in orbits for b in o) == list(range(625))         # every tuple in exactly one orbit
    assert [min(o) for o in orbits] == sorted(min(o) for o in orbits)       # ordered by their smallest member
    for k, o in enumerate(orbits):
        for b in o:
            assert srm._ORBIT[b] == k
            t = _digits(b)
            assert _bin(tuple(-d for d in t)) in o and _bin(t[::-1]) in o
    assert sorted(len(o) for o in orbits).count(1) == 1 and orbits[srm._ORBIT[312]] == [312]
    assert srm._FOLD.shape == (625, 169) and (srm._FOLD.sum(axis=1) == 1).all() and srm._FOLD.sum(axis=0).tolist() == [len(o) for o in orbits]


def test_features_against_the_restatement_and_block_sums():
    c = _counts()
    want = srm_np.features(c)
    for got in (srm.features(c), srm.features(torch.from_numpy(c))):
        assert got.dtype == np.float64 and got.shape == (3, 3718)
        np.testing.assert_array_equal(got, want)
    blocks = want.reshape(3, 22, 169)
    np.testing.assert_allclose(blocks.sum(axis=2), 1., rtol=0, atol=1e-12)
    assert (blocks[2, :, srm._ORBIT[312]] == 1.).all() and np.count_nonzero(blocks[2]) == 22
    # from real counts: the first block is T[hh] + T[vv] of S1 at q2 = 2, folded
    x = np.stack([_image(), _image(seed=6)])
    cx = srm_np.counts(x)
    F = srm.features(cx)
    np.testing.assert_array_equal(F, srm_np.features(cx))
    par = (cx[:, 0] + cx[:, 3]).astype(np.float64)
    k = srm._ORBIT[_bin((0, 0, 1, -1))]
    members = [_bin(t) for t in {(0, 0, 1, -1), (0, 0, -1, 1), (-1, 1, 0, 0), (1, -1, 0, 0)}]
    np.testing.assert_array_equal(F[:, k], par[:, members].sum(axis=1) / par.sum(axis=1))


def test_features_are_invariant_under_both_symmetries_of_the_raw_tables():
    c = _counts(seed=3)[:2]
    tuples = list(itertools.product(range(-2, 3), repeat=4))
    neg = np.array([_bin(tuple(-d for d in t)) for t in tuples])
    rev = np.array([_bin(t[::-1]) for t in tuples])
    F = srm.features(c)
    assert not np.array_equal(c[:, :, neg], c) and not np.array_equal(c[:, :, rev], c)
    for perm in (neg, rev, neg[rev]):
        np.testing.assert_array_equal(srm.features(c[:, :, perm]), F)
        np.testing.assert_array_equal(srm_np.features(c[:, :, perm]), F)


def test_features_refuse_an_empty_block_and_bad_shapes():
    c = np.ones((2, 44, 625), dtype=np.int64)
    c[1, 42:44] = 0                                                          # no 5x5 run: an image too small for one
    with pytest.raises(ValueError, match="image 1.*S5x5"):
        srm.features(c)
    c[1, 42] = 1                                                             # one of the block's two tables is enough
    assert srm.features(c).shape == (2, 3718)
    for bad in (c[0], c[:, :43], c[:, :, :624]):
        with pytest.raises(ValueError, match="expected"):
            srm.features(bad)
    with pytest.raises(ValueError, match="block without a run"):
        srm_np.features(srm_np.counts(np.zeros((1, 4, 30), dtype=np.uint8)))


# ---- the model file -----------------------------------------------------------------------------------------------------------------------

def test_model_save_and_load_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    X0, X1 = rng.random((6, 3718)), rng.random((5, 3718)) + 0.01
    m = srm.FLD(0.25).fit(X0, X1)
    assert isinstance(m, spam.FLD) and (m.order, m.T, m.ridge) == (4, 2, 0.25) and m.w.shape == (3718,)
    w, b = srm_np.fld_fit(X0, X1, 0.25)                                      # the discriminant's arithmetic is spam's
    np.testing.assert_array_equal(m.w, w)
    assert m.b == b
    m.stego_methods, m.alphas = ["SUNIWARD", "WOW"], [0.4, 0.2]
    m.save(tmp_path / "m.npz")
    with np.load(tmp_path / "m.npz", allow_pickle=False) as z:              # data only
        assert sorted(z.files) == sorted(["w", "b", "ridge", "features", "order", "T", "q2_S1", "q2_S2", "q2_S3", "q2_S3x3", "q2_S5x5",
                                          "stego_methods", "alphas"])
        assert str(z["features"]) == "srm-linear" and int(z["T"]) == 2 and int(z["order"]) == 4
        assert z["q2_S1"].tolist() == [2, 4] and z["q2_S5x5"].tolist() == [24, 36, 48]
    for r in (srm.FLD.load(tmp_path / "m.npz"), srm.load(tmp_path / "m.npz")):
        np.testing.assert_array_equal(r.w, m.w)
        assert (r.b, r.ridge, r.stego_methods, r.alphas) == (m.b, 0.25, ["SUNIWARD", "WOW"], [0.4, 0.2])
        np.testing.assert_array_equal(r.output(X1), m.output(X1))
    with pytest.raises(Exception):                                          # SPAM's loader does not take an SRM model ...
        spam.FLD.load(tmp_path / "m.npz")
    s = spam.FLD().fit(rng.random((6, 686)), rng.random((6, 686)))
    s.save(tmp_path / "spam.npz")
    with pytest.raises(ValueError, match="srm-linear"):                     # ... nor this one a SPAM model
        srm.load(tmp_path / "spam.npz")
    m.w = m.w[:686]
    m.save(tmp_path / "short.npz")
    with pytest.raises(ValueError, match="686 weights, expected 3718"):
        srm.load(tmp_path / "short.npz")
    with pytest.raises(ValueError, match="not fitted"):
        srm.FLD().save(tmp_path / "n.npz")
    with pytest.raises(ValueError, match="3718"):
        srm.FLD().fit(X0[:, :686], X1[:, :686])
    with pytest.raises(ValueError):
        srm.FLD(-1.)


# ---- the C entry's argument errors: errno-style code + message before any HIP call ------------------------------------------------------

def test_c_entry_rejects_bad_arguments_without_a_gpu():
    assert _lib.SIGNATURES["wsu_srm_counts"] == _lib.SIGNATURES["wsu_rs_counts"]
    lib = _lib.load()
    err = lib.wsu_last_error

    def call(x=8, counts=8, n=1, h=8, w=8):
        return lib.wsu_srm_counts(x, counts, n, h, w, None)
    assert call(x=None) == -1 and b"null" in err() and b"srm_counts" in err()
    assert call(counts=None) == -1 and b"null" in err()
    assert call(n=0) == -1 and b"bad shape" in err()
    assert call(n=65536) == -1 and b"bad shape" in err()
    assert call(h=0) == -1 and b"bad shape" in err()
    assert call(w=0) == -1 and b"bad shape" in err()
    assert call(h=2 ** 31 - 1, w=2 ** 31 - 1) == -1 and b"too many tiles" in err()
    with pytest.raises(_lib.WsuError, match="CPU tensor"):                   # a valid call gets as far as the device check
        ops.srm_counts(torch.zeros((1, 8, 8), dtype=torch.uint8))


# ---- drivers: argument errors before any file or device work, and the CLI parser ----------------------------------------------------------

def test_extract_and_cli_argument_errors(tmp_path):
    with pytest.raises(ValueError, match="both stego_method and alpha"):
        srm.extract(tmp_path, "SUNIWARD")
    with pytest.raises(ValueError, match="SUNIWARD / WOW"):
        srm.extract(tmp_path, "LSBRS", 0.4, simulate=True)
    assert srm.SIMULATED == ("LSBR", "HILLR", "LSBM", "HILL", "SUNIWARD", "WOW")
    a = srm.parse_args(["fit", "--data", "d", "--alphas", ".4", ".2", "--out", "m.npz"])
    assert (a.command, a.data, a.split, a.stego_methods, a.alphas, a.simulate, a.stream, a.batch_size, a.ridge, a.out) == (
        "fit", "d", None, ["LSBR"], [0.4, 0.2], False, 0, 32, 0.1, "m.npz")
    a = srm.parse_args(["score", "--data", "d", "--split", "split_te.csv", "--model", "m.npz", "--stego-methods", "SUNIWARD", "WOW", "--alphas", ".1",
                        "--simulate", "--out", "s.csv"])
    assert (a.command, a.split, a.model, a.stego_methods, a.alphas, a.simulate, a.out) == ("score", "split_te.csv", "m.npz", ["SUNIWARD", "WOW"], [0.1], True, "s.csv")
    a = srm.parse_args(["features", "--data", "d", "--alphas", ".1", "--out", "F.npz"])
    assert a.command == "features" and not hasattr(a, "order")
    for bad in (["fit", "--data", "d", "--out", "m.npz"], ["score", "--data", "d", "--alphas", ".1", "--out", "s.csv"], ["--data", "d"]):
        with pytest.raises(SystemExit):
            srm.parse_args(bad)
    assert srm.CSV_COLUMNS == ["name", "height", "width", "output", "prediction", "stego_method", "alpha"]
