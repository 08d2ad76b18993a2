"""CPU: the host side of the HILL-cost weighted prediction error -- the numpy quantile index, the new C-ABI argument checks,
the filter tap layout and the row layout / zip semantics of filters.run (device call stubbed)."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from ws_unet_amd import filters, hill

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    so = ROOT / "ws_unet_amd" / "libwsu.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(ROOT / "ws_unet_amd" / "csrc"), "-j4"], check=True)
    from ws_unet_amd import _lib
    return _lib.load()


def _np_lerp(c, k, g):
    a, b = c[k], c[min(k + 1, len(c) - 1)]
    d = b - a
    return b - d * (1 - g) if g >= 0.5 else a + d * g


@pytest.mark.parametrize("n", [1, 2, 3, 7, 10, 11, 101, 1000, 4097, 260100, 3136524])
def test_quantile_index_matches_numpy(n):
    rng = np.random.default_rng(n)
    c = np.sort(rng.random(min(n, 5000)) * 10)
    for q in (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0, 1 / 3, 0.999999, 1e-9, *rng.random(20)):
        k, g = hill.quantile_index(n, q)
        v = (n - 1) * q
        assert 0 <= k <= n - 1 and 0.0 <= g < 1.0
        if v < n - 1:
            assert k == np.floor(v) and g == v - np.floor(v)
        if n <= 5000:
            assert _np_lerp(c, k, g) == np.quantile(c, q)


def test_quantile_index_rejects_bad_arguments():
    for n, q in ((0, 0.1), (5, -0.1), (5, 1.5)):
        with pytest.raises(ValueError):
            hill.quantile_index(n, q)


def test_argument_errors_without_gpu(lib):
    assert lib.wsu_hill_threshold_workspace_bytes(2) == 2 * (3 * 2048 + 4) * 4
    assert lib.wsu_prediction_error_workspace_bytes(3) == 3 * 64 * 3 * 8
    assert lib.wsu_hill_cost(None, None, 1e10, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_hill_cost(1, 1, 1e10, 1, 2, 8, None) == -1 and b"h=2" in lib.wsu_last_error()
    assert lib.wsu_hill_cost(1, 1, 1e10, 0, 8, 8, None) == -1 and b"n=0" in lib.wsu_last_error()
    assert lib.wsu_hill_cost(1, 1, float("inf"), 1, 8, 8, None) == -1 and b"clamp" in lib.wsu_last_error()
    ws = lib.wsu_hill_threshold_workspace_bytes(1)
    assert lib.wsu_hill_threshold(None, 0, 0.0, 1, 1, ws, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_hill_threshold(1, 0, 0.0, 1, 1, ws, 1, 8, 2, None) == -1 and b"w=2" in lib.wsu_last_error()
    assert lib.wsu_hill_threshold(1, 36, 0.0, 1, 1, ws, 1, 8, 8, None) == -1 and b"k=36" in lib.wsu_last_error()
    assert lib.wsu_hill_threshold(1, 3, 1.0, 1, 1, ws, 1, 8, 8, None) == -1 and b"g=1" in lib.wsu_last_error()
    assert lib.wsu_hill_threshold(1, 3, 0.5, 1, 1, ws - 1, 1, 8, 8, None) == -1 and b"workspace" in lib.wsu_last_error()
    taps = (ctypes.c_double * 9)()
    wsp = lib.wsu_prediction_error_workspace_bytes(1)
    assert lib.wsu_prediction_error(1, None, None, 1, 255., 1, 1, 1, 1, None, 1, wsp, 1, 8, 8, None) == -1 \
        and b"exactly one" in lib.wsu_last_error()
    assert lib.wsu_prediction_error(1, 1, taps, 1, 255., 1, 1, 1, 1, None, 1, wsp, 1, 8, 8, None) == -1 \
        and b"exactly one" in lib.wsu_last_error()
    assert lib.wsu_prediction_error(1, None, taps, 1, 255., None, 1, 1, 1, None, 1, wsp, 1, 8, 8, None) == -1 \
        and b"null" in lib.wsu_last_error()
    assert lib.wsu_prediction_error(1, None, taps, 1, 255., 1, 1, 1, 1, None, 1, wsp, 1, 1, 8, None) == -1 \
        and b"h=1" in lib.wsu_last_error()
    assert lib.wsu_prediction_error(1, None, taps, 1, 255., 1, 1, 1, 1, None, 1, wsp, -1, 8, 8, None) == -1 \
        and b"n=-1" in lib.wsu_last_error()


def test_filter_taps_layout():
    from ws_unet_amd.ops import filter_taps

    def weights(k):
        return filter_taps(k, np.float64, "weights", "2d 8")
    flat = np.arange(1, 9, dtype=np.float64)                 # x00 x01 x02 x12 x22 x21 x20 x10
    np.testing.assert_array_equal(weights(flat).reshape(3, 3), [[1, 2, 3], [8, 0, 4], [7, 6, 5]])
    np.testing.assert_array_equal(weights(flat[:, None]), weights(flat))
    # the (3,3,1) convolution layout of NAMED_FILTERS_2D gives the same weights as the flattened taps
    for name in ("AVG", "KB"):
        np.testing.assert_array_equal(weights(filters.NAMED_FILTERS_2D[name]), weights(filters.NAMED_FILTERS[name]))
    with pytest.raises(ValueError):
        weights(np.ones((2, 2)))
    # one layout, two directions: the kernel layout is the weights reversed, in the dtype asked for, and a (3,3[,1]) array passes through
    for name, k2d in filters.NAMED_FILTERS_2D.items():
        kern = filter_taps(k2d, np.float32, "kernel")
        assert kern.dtype == np.float32 and kern.flags.c_contiguous
        np.testing.assert_array_equal(kern, np.asarray(k2d, dtype=np.float32).reshape(9))
        np.testing.assert_array_equal(filter_taps(k2d, np.float64, "kernel")[::-1], weights(k2d))
    np.testing.assert_array_equal(filter_taps(flat, np.float64, "kernel", "2d 8")[::-1], weights(flat))
    nine = np.arange(9, dtype=np.float64)
    np.testing.assert_array_equal(filter_taps(nine, np.float64, "weights", "2d 8 9"), nine)       # already in the layout
    for bad, allow in ((flat, "2d"), (nine, "2d 8")):        # 8 or 9 flat values only where the wrapper takes them
        with pytest.raises(ValueError):
            filter_taps(bad, np.float64, "weights", allow)
    assert filter_taps(None, np.float32, "kernel") is None


def _fake_dataset(root, names):
    (root / "images").mkdir()
    for n in names:
        (root / "images" / n).write_bytes(b"")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{n},4,5\n" for n in names))


@pytest.mark.parametrize("iterator", ["python", "batched"])
def test_run_row_layout_and_zip_semantics(tmp_path, monkeypatch, iterator):
    _fake_dataset(tmp_path, ["6.png", "10.png", "7.png"])
    calls = []

    def fake_device_error(x_u8, filter):
        calls.append((x_u8.shape, float(np.asarray(filter).ravel()[0])))
        n = x_u8.shape[0]
        return np.arange(n, dtype=np.float64) + 1, np.arange(n, dtype=np.float64) + 10

    monkeypatch.setattr(filters, "_device_error", fake_device_error)
    img = lambda f: np.zeros((4, 5, 4), dtype=np.float32)      # noqa: E731  (imread4_f32-like)
    df = filters.run(tmp_path, imread=img, iterator=iterator)
    # the default channels has ONE entry: zip() stops after the first filter, as in the reference
    assert list(df.columns) == ["fname", "mae_3_AVG", "wmae_3_AVG", "name", "height", "width"]
    assert df["name"].tolist() == ["images/10.png", "images/6.png", "images/7.png"]
    assert [str(f) for f in df["fname"]] == [str(tmp_path / n) for n in df["name"]]
    assert all(f == 1 / 8 for _, f in calls)
    df2 = filters.run(tmp_path, filter_names=["AVG", "KB"], channels=[[3], [3]], imread=img, iterator=iterator)
    assert list(df2.columns) == ["fname", "mae_3_AVG", "wmae_3_AVG", "name", "height", "width", "mae_3_KB", "wmae_3_KB"]
    assert len(df2) == 6 and df2["mae_3_KB"].isna().sum() == 3 and df2["mae_3_AVG"].isna().sum() == 3
    assert isinstance(df2, pd.DataFrame)
    with pytest.raises(ValueError):
        filters.run(tmp_path, imread=lambda f: np.full((4, 5, 4), 0.5, dtype=np.float32), iterator=iterator)
