"""CPU: the host layer of the least-squares predictors (ws_unet_amd/ols.py) -- the float64 solve against numpy.linalg.lstsq on the
golden covers, the residual algebra, the KB fallback, the filter registry and kernels.json, and the drivers' --kernels flag."""
import numpy as np
import pytest

from conftest import GOLDEN
import ols_np
from ws_unet_amd import filters, ols
from ws_unet_amd.imread import imread4_u8

COVERS = (6, 7, 8, 9, 10)
KB8 = filters.NAMED_FILTERS["KB"][:, 0]


@pytest.fixture(scope="module")
def covers():
    """[(design matrix int64 (P,9), moments (45,) int64)] of the five golden covers' Y planes"""
    out = []
    for k in COVERS:
        v = ols_np.design(imread4_u8(GOLDEN / f"cover_{k}.png")[..., 3])
        out.append((v, (v.T @ v)[ols_np.IU]))
    return out


@pytest.fixture
def registry():
    """the two name tables as they were, whatever a test registers"""
    keep = dict(filters.NAMED_FILTERS), dict(filters.NAMED_FILTERS_2D)
    yield
    for table, saved in zip((filters.NAMED_FILTERS, filters.NAMED_FILTERS_2D), keep):
        table.clear()
        table.update(saved)


def test_fit_matches_lstsq_on_the_golden_covers(covers):
    for v, m in covers:
        taps, ok = ols.fit(m)
        ref = np.linalg.lstsq(v[:, :8].astype(np.float64), v[:, 8].astype(np.float64), rcond=None)[0]
        assert ok and taps.shape == (8,) and taps.dtype == np.float64
        np.testing.assert_allclose(taps, ref, rtol=0, atol=1e-10)
        np.testing.assert_allclose(taps, ols_np.solve(m), rtol=0, atol=1e-12)
    taps_n, ok_n = ols.fit(np.stack([m for _, m in covers]))
    assert taps_n.shape == (5, 8) and ok_n.dtype == bool and ok_n.all()
    for i, (_, m) in enumerate(covers):
        np.testing.assert_array_equal(taps_n[i], ols.fit(m)[0])


def test_symmetric_fit_matches_lstsq_on_the_two_column_design(covers):
    for v, m in covers:
        taps, ok = ols.fit(m, symmetric=True)
        x = v[:, :8].astype(np.float64)
        two = np.stack([x[:, 1::2].sum(axis=1), x[:, 0::2].sum(axis=1)], axis=1)            # edge sum, corner sum
        edge, corner = np.linalg.lstsq(two, v[:, 8].astype(np.float64), rcond=None)[0]
        assert ok
        np.testing.assert_allclose(taps, [corner, edge] * 4, rtol=0, atol=1e-10)


def test_residual_mse_is_the_mean_squared_residual(covers):
    rng = np.random.default_rng(3)
    for v, m in covers:
        x, y = v[:, :8].astype(np.float64), v[:, 8].astype(np.float64)
        for taps in (ols.fit(m)[0], KB8, rng.normal(size=8)):
            direct = np.mean((y - x @ taps) ** 2)
            np.testing.assert_allclose(ols.residual_mse(m, taps, len(y)), direct, rtol=1e-9, atol=0)
        assert ols.residual_mse(m, ols.fit(m)[0], len(y)) <= ols.residual_mse(m, KB8, len(y))


def test_unpack_layout_and_range():
    x = np.random.default_rng(1).integers(0, 256, (6, 9), dtype=np.uint8)
    v = ols_np.design(x)
    A, b, yty = ols.unpack(ols_np.moments(x))
    np.testing.assert_array_equal(A, (v[:, :8].T @ v[:, :8]).astype(np.float64))
    np.testing.assert_array_equal(b, (v[:, :8].T @ v[:, 8]).astype(np.float64))
    assert yty == float(v[:, 8] @ v[:, 8])
    big = np.zeros(45, dtype=np.int64)
    big[0] = 2 ** 53 + 2
    with pytest.raises(OverflowError):
        ols.unpack(big)
    with pytest.raises(ValueError):
        ols.unpack(np.zeros(44, dtype=np.int64))
    with pytest.raises(ValueError):
        ols.unpack(np.zeros(45))


def test_degenerate_images_fall_back_to_kb():
    rng = np.random.default_rng(7)
    for x in (np.full((16, 16), 93, dtype=np.uint8), rng.integers(1, 256, (3, 3), dtype=np.uint8), np.zeros((8, 8), dtype=np.uint8)):
        for symmetric in (False, True):
            taps, ok = ols.fit(ols_np.moments(x), symmetric)
            assert ok is False
            np.testing.assert_array_equal(taps, KB8)
    x = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    taps, ok = ols.fit(ols_np.moments(x))
    assert ok is True
    np.testing.assert_allclose(taps, ols_np.solve(ols_np.moments(x)), rtol=0, atol=1e-12)
    # rows of a batch fall back on their own
    taps_n, ok_n = ols.fit(np.stack([ols_np.moments(x), ols_np.moments(np.full((5, 7), 4, dtype=np.uint8))]))
    assert ok_n.tolist() == [True, False]
    np.testing.assert_array_equal(taps_n[1], KB8)
    np.testing.assert_array_equal(taps_n[0], taps)


def test_registering_kb_taps_gives_the_builtin_arrays(registry):
    filters.register_filter("KB_again", KB8)
    for table in (filters.NAMED_FILTERS, filters.NAMED_FILTERS_2D):
        assert table["KB_again"].shape == table["KB"].shape and table["KB_again"].dtype == table["KB"].dtype
        np.testing.assert_array_equal(table["KB_again"], table["KB"])
    from ws_unet_amd.ws import estimate
    assert estimate.NAMED_FILTERS is filters.NAMED_FILTERS_2D and "KB_again" in estimate.NAMED_FILTERS


def test_registered_kernel_is_the_same_predictor_as_its_taps(registry):
    """an asymmetric filter: the (3,3,1) kernel and the 8 taps reach the C entry points as the same nine weights"""
    from ws_unet_amd import ops
    taps = np.arange(1., 9.) / 7.
    filters.register_filter("ramp", taps)
    for layout in ("weights", "kernel"):
        np.testing.assert_array_equal(ops.filter_taps(filters.get_coefficients("ramp", flatten=False), np.float32, layout),
                                      ops.filter_taps(filters.get_coefficients("ramp"), np.float32, layout, allow="8"))
    wgt = ops.filter_taps(filters.get_coefficients("ramp"), np.float64, "weights", allow="8").reshape(3, 3)
    assert [wgt[a, b] for a, b in ols_np.RING] == taps.tolist() and wgt[1, 1] == 0


def test_registry_misuse_and_kernel_files(tmp_path, registry):
    for name in ("AVG", "AVG9", "KB", "1"):
        with pytest.raises(ValueError, match="built-in"):
            filters.register_filter(name, KB8)
    with pytest.raises(ValueError):
        filters.register_filter("short", np.ones(7))
    with pytest.raises(ValueError):
        filters.register_filter("nan", np.full(8, np.nan))
    assert sorted(filters.NAMED_FILTERS) == ["AVG", "KB"] and sorted(filters.NAMED_FILTERS_2D) == ["1", "AVG", "AVG9", "KB"]
    taps = {"OLS": np.random.default_rng(5).normal(size=8) / 3., "OLS2": np.array([-.1, .35] * 4) + 1e-17}
    path = tmp_path / "sub" / "kernels.json"
    ols.save_kernels(path, taps)
    back = ols.load_kernels(path)
    assert list(back) == ["OLS", "OLS2"]
    for name in taps:
        assert back[name].dtype == np.float64 and back[name].tobytes() == taps[name].tobytes()           # bit-exact round trip
    assert "OLS" not in filters.NAMED_FILTERS
    ols.load_kernels(path, register=True)
    for name in taps:
        np.testing.assert_array_equal(filters.get_coefficients(name), taps[name].reshape(8, 1))
        np.testing.assert_array_equal(filters.get_coefficients(name, flatten=False), filters.kernel_2d(taps[name]))
        assert filters.get_coefficients(name, flatten=False).shape == (3, 3, 1)
    path.write_text('{"bad": [1, 2, 3]}')
    with pytest.raises(ValueError, match="8 taps"):
        ols.load_kernels(path)


def test_kernels_flag_parses_in_the_five_drivers():
    from ws_unet_amd import correlation, error_boxes, prediction_error
    from ws_unet_amd.ws import estimate, roc
    base = ["--data", "d", "--out", "o.csv"]
    for mod, argv in ((prediction_error, base), (correlation, base), (error_boxes, base),
                      (roc, ["--data", "d", "--out-dir", "o"]), (estimate, [])):
        a = mod.parse_args(argv + ["--kernels", "k.json", "--filters", "AVG", "KB", "OLS"])
        assert a.kernels == "k.json" and a.filters == ["AVG", "KB", "OLS"], mod.__name__
        assert mod.parse_args(argv).kernels is None
    assert error_boxes.parse_args(base).filters == ["KB", "AVG"]                     # the table's two filter rows, as before
    assert ols.adaptive_estimator("OLSa").symmetric is False and ols.adaptive_estimator("OLSa2").symmetric is True
    assert ols.adaptive_estimator("KB") is None
