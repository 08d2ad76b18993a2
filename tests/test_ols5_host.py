"""CPU: the host side of the 5x5 least-squares predictors (ws_unet_amd/ols5.py, K56 / K57): the symmetric classes, unpack / fit on
synthetic moments, the invalid-fit fallback, the kernels file, the model names, the drivers' --kernels5 and the argument errors of the
two C entries (no GPU call is made)."""
import json

import numpy as np
import pytest

import ols5_np
from ws_unet_amd import _lib, filters, ols5
from ws_unet_amd.ws import estimate, keysearch, locate, roc


@pytest.fixture
def registry():
    keep = dict(ols5.KERNELS)
    yield
    ols5.KERNELS.clear()
    ols5.KERNELS.update(keep)


def _image(seed, shape=(24, 31)):
    """a smooth random image plus noise: neighbours that correlate, so the normal equations are well conditioned"""
    rng = np.random.default_rng(seed)
    base = np.cumsum(np.cumsum(rng.normal(size=shape), axis=0), axis=1)
    base = 128 + 100 * base / np.abs(base).max()
    return np.clip(np.rint(base + rng.normal(scale=3., size=shape)), 0, 255).astype(np.uint8)


def test_symmetric_matrix_has_the_class_sizes_4_4_4_8_4():
    S = ols5.SYMMETRIC
    assert S.shape == (24, 5) and S.sum(axis=0).tolist() == [4, 4, 4, 8, 4] and (S.sum(axis=1) == 1).all()
    np.testing.assert_array_equal(S, ols5_np.symmetric_matrix())
    assert ols5.OFFSETS == [(a - 2, b - 2) for a, b in ols5_np.OFFSETS]
    # the inner ring: edges are class 0, corners class 1
    np.testing.assert_array_equal(np.argmax(S[[6, 7, 8, 11, 12, 15, 16, 17]], axis=1), [1, 0, 1, 0, 0, 1, 0, 1])


def test_kb_embedding():
    kb = ols5_np.kb_taps()
    np.testing.assert_array_equal(ols5._kb(), kb)
    np.testing.assert_array_equal(ols5.embed3x3(ols5_np.KB3), kb)
    assert np.count_nonzero(kb) == 8 and kb.sum() == 1.0
    np.testing.assert_array_equal(np.insert(kb, 12, 0.).reshape(5, 5)[1:4, 1:4], ols5_np.KB3)
    np.testing.assert_array_equal(kb, ols5.SYMMETRIC @ np.array([.5, -.25, 0, 0, 0]))


def test_a_transposed_or_mirrored_image_gives_the_same_symmetric_fit():
    x = _image(1)
    want, ok = ols5.fit(ols5_np.moments(x), symmetric=True)
    assert ok
    for y in (x.T, x[::-1], x[:, ::-1], x[::-1, ::-1].T):
        got, ok = ols5.fit(ols5_np.moments(np.ascontiguousarray(y)), symmetric=True)
        assert ok
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)          # the folded 5x5 system has the same entries, summed in another order
    assert len(np.unique(np.round(want, 12))) <= 5 and np.allclose(want, ols5.SYMMETRIC @ (ols5.SYMMETRIC.T @ want / ols5.SYMMETRIC.sum(axis=0)))


def test_unpack_and_fit_recover_planted_taps():
    """integer y = X k for integer taps: the moments are exact, and the solve returns k to rounding"""
    rng = np.random.default_rng(3)
    X = rng.integers(0, 256, (4000, 24)).astype(np.int64)
    for symmetric in (False, True):
        k = ols5.SYMMETRIC @ rng.integers(-3, 4, 5) if symmetric else rng.integers(-3, 4, 24)
        v = np.concatenate([X, (X @ k.astype(np.int64))[:, None]], axis=1)
        m = (v.T @ v)[ols5_np.IU]
        A, b, yty = ols5.unpack(m)
        np.testing.assert_array_equal(A, (X.T @ X).astype(np.float64))
        np.testing.assert_array_equal(b, (X.T @ v[:, 24]).astype(np.float64))
        assert yty == float(v[:, 24] @ v[:, 24])
        taps, ok = ols5.fit(m, symmetric)
        assert ok and taps.shape == (24,)
        np.testing.assert_allclose(taps, k, rtol=0, atol=1e-8)
        assert abs(ols5.residual_mse(m, k, len(X))) < 1e-3
    both, oks = ols5.fit(np.stack([m, m]))
    assert both.shape == (2, 24) and oks.tolist() == [True, True]
    A2, b2, y2 = ols5.unpack(np.stack([m, m]))
    assert A2.shape == (2, 24, 24) and b2.shape == (2, 24) and y2.shape == (2,)
    with pytest.raises(ValueError, match="integer moments"):
        ols5.unpack(np.zeros(325))
    with pytest.raises(ValueError, match="integer moments"):
        ols5.unpack(np.zeros(45, dtype=np.int64))
    with pytest.raises(OverflowError):
        ols5.unpack(np.full(325, 2 ** 53 + 2, dtype=np.int64))
    with pytest.raises(OverflowError):
        ols5.unpack(np.full(325, -1, dtype=np.int64))


def test_a_flat_image_gives_the_invalid_fit_fallback_embedded_kb():
    flat = ols5_np.moments(np.full((9, 11), 9, dtype=np.uint8))
    for symmetric in (False, True):
        taps, ok = ols5.fit(flat, symmetric)
        assert not ok
        np.testing.assert_array_equal(taps, ols5_np.kb_taps())
    taps, ok = ols5.fit(np.stack([flat, ols5_np.moments(_image(5))]))
    assert ok.tolist() == [False, True] and not np.array_equal(taps[1], ols5_np.kb_taps())
    np.testing.assert_array_equal(taps[0], ols5_np.kb_taps())
    # fewer pixels than parameters: singular as well
    assert not ols5.fit(ols5_np.moments(_image(6, (6, 7))))[1]


def test_kernels_file_round_trip(tmp_path, registry):
    taps = np.random.default_rng(7).normal(size=24) / 7.
    path = tmp_path / "sub" / "kernels5.json"
    ols5.save_kernels(path, {"OLS5x5": taps, "other": taps[::-1]})
    got = ols5.load_kernels(path)
    assert list(got) == ["OLS5x5", "other"]
    np.testing.assert_array_equal(got["OLS5x5"], taps)
    np.testing.assert_array_equal(got["other"], taps[::-1])
    assert list(json.loads(path.read_text())) == ["OLS5x5", "other"] and "OLS5x5" not in ols5.KERNELS
    ols5.load_kernels(path, register=True)
    np.testing.assert_array_equal(ols5.KERNELS["OLS5x5"], taps)
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"OLS": [0.125] * 8}))
    with pytest.raises(ValueError, match="expected 24 taps"):
        ols5.load_kernels(bad)
    bad.write_text("[1, 2]")
    with pytest.raises(ValueError, match="JSON object"):
        ols5.load_kernels(bad)
    for name in ("KB", "OLSa", "OLSa5x5", ""):
        with pytest.raises(ValueError, match="name"):
            ols5.register_kernel(name, taps)
    with pytest.raises(ValueError, match="finite"):
        ols5.register_kernel("x", np.full(24, np.nan))


def test_estimator_names(registry):
    a, s = ols5.estimator("OLSa5x5"), ols5.estimator("OLSa5x5s")
    assert isinstance(a, ols5.Predictor5x5) and a.adaptive and not a.symmetric and a.fallbacks == 0
    assert isinstance(s, ols5.Predictor5x5) and s.adaptive and s.symmetric
    assert ols5.estimator("OLSa5x5") is not a                                   # a fresh one per call
    for name in ("KB", "OLSa", "OLS5x5", "JPEG", "nothing"):
        assert ols5.estimator(name) is None
    ols5.register_kernel("OLS5x5", ols5_np.kb_taps())
    fixed = ols5.estimator("OLS5x5")
    assert isinstance(fixed, ols5.Predictor5x5) and not fixed.adaptive
    np.testing.assert_array_equal(fixed.taps, ols5_np.kb_taps())
    assert ols5.names() == ["OLSa5x5", "OLSa5x5s", "OLS5x5"]
    assert isinstance(locate.pixel_predictor("OLSa5x5s", None, (3,))[0], ols5.Predictor5x5)
    assert locate.pixel_predictor("OLS5x5", None, (3,))[1] == "OLS5x5"
    assert estimate._native_planes_ok((3,), a, estimate.imread4_u8, None)
    estimate._check_options(a, 1, True)                                        # bias correction is defined for it
    with pytest.raises(ValueError):
        ols5.Predictor5x5()
    with pytest.raises(ValueError):
        ols5.Predictor5x5(np.zeros(8))
    with pytest.raises(ValueError):
        ols5.Predictor5x5(ols5_np.kb_taps(), symmetric=True)
    with pytest.raises(ValueError, match="unknown filter"):
        roc.collect_ws_scores("nowhere", ["LSBR"], [1.0], ["OLS5x5x"])


def test_a_predictor_refuses_planes_below_5x5():
    import torch
    for shape in ((1, 4, 9), (1, 9, 4), (4, 9)):
        with pytest.raises(ValueError, match="5 x 5"):
            ols5.Predictor5x5(ols5_np.kb_taps()).planes(torch.zeros(shape, dtype=torch.uint8))


def test_the_four_drivers_accept_kernels5():
    assert estimate.parse_args(["--kernels5", "k5.json"]).kernels5 == "k5.json" and estimate.parse_args([]).kernels5 is None
    assert roc.parse_args(["--data", "d", "--out-dir", "o", "--kernels5", "k5.json"]).kernels5 == "k5.json"
    assert locate.parse_args(["--data", "d", "--out-dir", "o", "--alpha", "0.5", "--kernels5", "k5.json"]).kernels5 == "k5.json"
    a = keysearch.parse_args(["--data", "d", "--out", "o", "--alpha", "0.5", "--first", "0", "--count", "4", "--kernels5", "k5.json", "--kernels", "k.json"])
    assert a.kernels5 == "k5.json" and a.kernels == "k.json"


def test_c_entries_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    m = lib.wsu_ols_moments5
    assert m(None, 8, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert m(8, None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    for n, h, w in ((1, 4, 8), (1, 8, 4), (0, 8, 8), (65536, 8, 8)):
        assert m(8, 8, n, h, w, None) == -1 and b"ols_moments5: bad shape" in lib.wsu_last_error()
    p = lib.wsu_predict5x5
    assert p(None, 8, 0, 8, None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert p(8, None, 0, 8, None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert p(8, 8, 0, None, 8, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    for n, h, w in ((1, 2, 8), (1, 8, 2), (0, 8, 8), (65536, 8, 8)):
        assert p(8, 8, 1, 8, None, n, h, w, None) == -1 and b"predict5x5: bad shape" in lib.wsu_last_error()
