"""CPU: the host side of the SPAM detector (K36, ws_unet_amd/spam.py): the opposite-direction permutation against brute-force counting,
`features` against the numpy restatement (spam_np) on hand-made counts, the Fisher discriminant against a closed-form solve, the model
file, the C entry's argument errors (no GPU call is made) and the CLI parser."""
import numpy as np
import pytest
import torch

import spam_np
from ws_unet_amd import _lib, ops, spam

CONFIGS = [(2, 3), (1, 4), (2, 1), (2, 4), (1, 8)]                          # (order, T)


def _image(h=13, w=17, seed=5):
    """a noisy plane with a flat patch, a ramp and the two extremes side by side (differences of every size, many of them clipped)"""
    x = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    x[2:8, 3:11] = 90
    x[9] = np.arange(w, dtype=np.uint8) * 2
    x[0, :4] = (0, 255, 0, 255)
    return x


# ---- the opposite directions are a permutation of the counted ones --------------------------------------------------------------------

@pytest.mark.parametrize("order,T", CONFIGS)
def test_opposite_equals_counting_the_opposite_step(order, T):
    x = np.stack([_image(), _image(seed=6)])
    fwd = spam_np.counts(x, order, T)
    bwd = spam_np.counts(x, order, T, steps=spam_np.STEPS8[4:])
    assert fwd.shape == (2, 4, spam_np.bins(order, T)) == bwd.shape and fwd.sum() > 0
    for d in range(4):
        assert not np.array_equal(fwd[:, d], bwd[:, d])                   # (the check below is not vacuous)
    np.testing.assert_array_equal(spam_np.opposite(fwd, order, T), bwd)
    np.testing.assert_array_equal(spam.opposite(fwd, order, T), bwd)
    got = spam.opposite(torch.from_numpy(fwd), order, T)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64
    np.testing.assert_array_equal(got.numpy(), bwd)
    np.testing.assert_array_equal(spam.opposite(spam.opposite(fwd, order, T), order, T), fwd)
    np.testing.assert_array_equal(spam.opposite(fwd[0, 1], order, T), bwd[0, 1])          # any leading shape
    assert spam.bins(order, T) == spam_np.bins(order, T) == ops.spam_bins(order, T)


def test_restatement_totals_and_clipping():
    x = _image()[None]
    h, w = x.shape[1:]
    for order, T in CONFIGS:
        k = order + 1
        c = spam_np.counts(x, order, T)[0]
        assert c.sum(axis=1).tolist() == [h * (w - k), (h - k) * w, (h - k) * (w - k), (h - k) * (w - k)]
    # 0 / 255 columns: every horizontal difference is clipped to +-T, alternating; every vertical one is 0
    cols = np.broadcast_to((np.arange(8) % 2 * 255).astype(np.uint8), (1, 6, 8)).copy()
    c = spam_np.counts(cols, 2, 3)[0]
    B = 7
    assert c[0, (0 * B + 6) * B + 0] == 6 * 3 and c[0, (6 * B + 0) * B + 6] == 6 * 2 and c[0].sum() == 6 * 5       # (-T, T, -T) from even columns
    assert c[1, (3 * B + 3) * B + 3] == 3 * 8 == c[1].sum()
    assert not spam_np.counts(np.zeros((1, 3, 9), dtype=np.uint8), 2, 3)[0, 1:].any()                                # too few rows for a vertical run


def test_bins_and_argument_checks():
    assert spam.bins(2, 3) == 343 and spam.bins(1, 4) == 81 and spam.bins(2, 4) == 729 and spam.bins(1, 8) == 289
    for order, T in ((3, 1), (0, 1), (2, 5), (1, 9), (2, 0), (1, -1), (2, 2.5)):
        with pytest.raises(ValueError, match="order"):
            spam.bins(order, T)
    with pytest.raises(ValueError, match="343 bins"):
        spam.opposite(np.zeros((4, 81), dtype=np.int64), 2, 3)
    with pytest.raises(_lib.WsuError, match="CPU tensor"):                                 # a valid call gets as far as the device check
        ops.spam_counts(torch.zeros((1, 8, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="order"):
        ops.spam_counts(torch.zeros((1, 8, 8), dtype=torch.uint8), order=3)


# ---- features ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order,T", [(2, 3), (1, 4), (2, 1)])
@pytest.mark.parametrize("normalise", spam.NORMALISE)
def test_features_against_the_restatement_on_hand_made_counts(order, T, normalise):
    nb, B = spam_np.bins(order, T), 2 * T + 1
    rng = np.random.default_rng(order * 10 + T)
    c = rng.integers(0, 1000, (3, 4, nb)).astype(np.int64)
    c[1, :, : nb // 2] = 0                                                   # whole transition rows without a count
    c[2] = 0
    c[2, :, nb // 2] = 12345                                                 # a constant plane: everything in the centre bin
    want = spam_np.features(c, order, T, normalise)
    for got in (spam.features(c, order, T, normalise), spam.features(torch.from_numpy(c), order, T, normalise)):
        assert got.dtype == np.float64 and got.shape == (3, 2 * nb)
        np.testing.assert_array_equal(got, want)
    halves = want.reshape(3, 2, nb)
    if normalise == "joint":
        np.testing.assert_allclose(halves.sum(axis=2), 1., rtol=0, atol=1e-12)
        assert want[2, nb // 2] == 1. and want[2, nb + nb // 2] == 1.
    else:
        rows = halves.reshape(3, 2, nb // B, B).sum(axis=3)
        # a half is the mean of four tables whose transition rows each sum to 1 or 0: a row of the mean sums to a multiple of 1/4 ...
        np.testing.assert_allclose(rows * 4, np.round(rows * 4), rtol=0, atol=1e-12)
        # ... and every single table's rows to 1 or 0
        digits = np.stack([np.arange(nb) // B ** j % B for j in range(order + 1)])
        small = (np.abs(digits - T) <= 1).all(axis=0)                        # counts only where every difference is in -1..1
        one = np.broadcast_to(np.where(small, c[0, 0], 0), (1, 4, nb))
        sym = one + spam_np.opposite(one, order, T)                         # its own opposite: all eight tables are this one
        r = spam.features(sym, order, T, normalise).reshape(2, nb // B, B).sum(axis=2)
        assert np.all((np.abs(r - 1.) <= 1e-12) | (r == 0.)) and (r != 0.).any() and (T == 1 or (r == 0.).any())
        assert want[2, nb // 2] == 1.


def test_features_refuse_an_empty_direction_and_bad_arguments():
    c = np.ones((2, 4, 343), dtype=np.int64)
    c[1, 3] = 0                                                              # no down-left run: an image narrower than order + 2
    with pytest.raises(ValueError, match="image 1"):
        spam.features(c)
    with pytest.raises(ValueError, match="normalise"):
        spam.features(c[:1], normalise="rows")
    with pytest.raises(ValueError, match="expected"):
        spam.features(c[:1], order=1, T=4)
    with pytest.raises(ValueError, match="expected"):
        spam.features(c[0])


# ---- the discriminant -------------------------------------------------------------------------------------------------------------------

def _clouds(d=5, n0=40, n1=30, seed=2):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d))
    return rng.standard_normal((n0, d)) @ A, rng.standard_normal((n1, d)) @ A + np.linspace(0.5, 1.5, d)


@pytest.mark.parametrize("ridge", [0.1, 1e-3, 0.0])
def test_fld_against_the_closed_form(ridge):
    X0, X1 = _clouds()
    d = X0.shape[1]
    mu0, mu1 = X0.mean(0), X1.mean(0)
    S = ((len(X0) - 1) * np.cov(X0, rowvar=False) + (len(X1) - 1) * np.cov(X1, rowvar=False)) / (len(X0) + len(X1) - 2)
    w = np.linalg.inv(S + ridge * np.trace(S) / d * np.eye(d)) @ (mu1 - mu0)
    b = w @ (mu0 + mu1) / 2
    m = spam.FLD(ridge).fit(X0, X1)
    np.testing.assert_allclose(m.w, w, rtol=1e-10, atol=0)
    assert abs(m.b - b) <= 1e-10 * max(1., abs(b))
    wn, bn = spam_np.fld_fit(X0, X1, ridge)
    np.testing.assert_array_equal(m.w, wn)
    assert m.b == bn
    X = np.concatenate([X0, X1])
    np.testing.assert_allclose(m.log_odds(X), X @ w - b, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(m.output(X), spam_np.fld_output(X, wn, bn))
    assert abs(m.output((mu0 + mu1)[None] / 2)[0] - 0.5) <= 1e-12 and abs(m.log_odds((mu0 + mu1)[None] / 2)[0]) <= 1e-12
    assert m.output(mu1[None])[0] > 0.5 > m.output(mu0[None])[0]
    assert spam_np.auc(m.output(X0), m.output(X1)) > 0.9
    assert spam.FLD().fit(X0, X1, ridge=ridge).ridge == ridge and spam.FLD().ridge == 0.1


def test_fld_save_and_load_round_trip(tmp_path):
    X0, X1 = _clouds(d=162)
    m = spam.FLD(0.25, order=1, T=4, normalise="transition").fit(X0, X1)
    m.stego_methods, m.alphas = ["LSBR", "HILLR"], [0.4, 0.1]
    m.save(tmp_path / "m.npz")
    with np.load(tmp_path / "m.npz", allow_pickle=False) as z:              # data only: nothing in the file needs unpickling
        assert sorted(z.files) == ["T", "alphas", "b", "normalise", "order", "ridge", "stego_methods", "w"]
    r = spam.FLD.load(tmp_path / "m.npz")
    np.testing.assert_array_equal(r.w, m.w)
    assert (r.b, r.ridge, r.order, r.T, r.normalise, r.stego_methods, r.alphas) == (m.b, 0.25, 1, 4, "transition", ["LSBR", "HILLR"], [0.4, 0.1])
    np.testing.assert_array_equal(r.output(X1), m.output(X1))
    with pytest.raises(ValueError, match="not fitted"):
        spam.FLD().save(tmp_path / "n.npz")
    with pytest.raises(ValueError, match="not fitted"):
        spam.FLD().output(X0)
    m.order, m.T = 2, 3                                                      # 162 weights are not a SPAM-686 model
    m.save(tmp_path / "bad.npz")
    with pytest.raises(ValueError, match="162 weights"):
        spam.FLD.load(tmp_path / "bad.npz")
    for bad in (dict(ridge=-1.), dict(normalise="rows"), dict(order=3)):
        with pytest.raises(ValueError):
            spam.FLD(**bad)
    with pytest.raises(ValueError, match="classes of shape"):
        spam.FLD().fit(X0, X1[:, :5])


# ---- the C entry's argument errors: errno-style code + message before any HIP call ------------------------------------------------------

def test_c_entry_rejects_bad_arguments_without_a_gpu():
    assert "wsu_spam_counts" in _lib.SIGNATURES
    lib = _lib.load()
    err = lib.wsu_last_error

    def call(x=8, counts=8, n=1, h=8, w=8, order=2, T=3):
        return lib.wsu_spam_counts(x, counts, n, h, w, order, T, None)
    assert call(x=None) == -1 and b"null" in err()
    assert call(counts=None) == -1 and b"null" in err()
    assert call(order=3) == -1 and b"order=3" in err()
    assert call(order=0) == -1 and b"order=0" in err()
    assert call(T=5) == -1 and b"T=5" in err() and b"1..4" in err()
    assert call(order=1, T=9) == -1 and b"T=9" in err() and b"1..8" in err()
    assert call(T=0) == -1 and b"T=0" in err()
    assert call(n=0) == -1 and b"bad shape" in err()
    assert call(n=65536) == -1 and b"bad shape" in err()
    assert call(h=0) == -1 and b"bad shape" in err()
    assert call(w=0) == -1 and b"bad shape" in err()
    assert call(h=2 ** 31 - 1, w=2 ** 31 - 1) == -1 and b"too many tiles" in err()


# ---- drivers: argument errors before any file or device work, and the CLI parser ----------------------------------------------------------

def test_extract_and_cli_argument_errors(tmp_path):
    with pytest.raises(ValueError, match="both stego_method and alpha"):
        spam.extract(tmp_path, "LSBR")
    with pytest.raises(ValueError, match="order"):
        spam.extract(tmp_path, order=2, T=5)
    with pytest.raises(ValueError, match="normalise"):
        spam.extract(tmp_path, normalise="rows")
    a = spam.parse_args(["fit", "--data", "d", "--alphas", ".4", ".2", "--out", "m.npz"])
    assert (a.command, a.data, a.split, a.stego_methods, a.alphas, a.simulate, a.order, a.T, a.normalise, a.ridge, a.out) == (
        "fit", "d", None, ["LSBR"], [0.4, 0.2], False, 2, 3, "joint", 0.1, "m.npz")
    a = spam.parse_args(["score", "--data", "d", "--split", "split_te.csv", "--model", "m.npz", "--stego-methods", "LSBR", "HILLR", "--alphas", ".1",
                         "--simulate", "--out", "s.csv"])
    assert (a.command, a.split, a.model, a.stego_methods, a.alphas, a.simulate, a.out) == ("score", "split_te.csv", "m.npz", ["LSBR", "HILLR"], [0.1], True, "s.csv")
    a = spam.parse_args(["features", "--data", "d", "--alphas", ".1", "--order", "1", "--T", "4", "--normalise", "transition", "--out", "F.npz"])
    assert (a.command, a.order, a.T, a.normalise) == ("features", 1, 4, "transition")
    for bad in (["fit", "--data", "d", "--out", "m.npz"], ["score", "--data", "d", "--alphas", ".1", "--out", "s.csv"], ["--data", "d"]):
        with pytest.raises(SystemExit):
            spam.parse_args(bad)
    assert spam.CSV_COLUMNS == ["name", "height", "width", "output", "prediction", "stego_method", "alpha"]
