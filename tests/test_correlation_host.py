"""CPU: the host side of the predictor / stego-change correlation -- Student's t survival function, the p-value formula, the
median table layout, the K15 C-ABI argument checks, the numpy restatement on the fixtures and the input errors of run()."""
import ctypes
import json
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import corr_np
from conftest import GOLDEN
from ws_unet_amd import correlation, filters

ROOT = Path(__file__).resolve().parent.parent
PAIRS = (6, 7, 8, 9, 10)


@pytest.fixture(scope="module")
def lib():
    so = ROOT / "ws_unet_amd" / "libwsu.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(ROOT / "ws_unet_amd" / "csrc"), "-j4"], check=True)
    from ws_unet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("df", [1, 2, 5, 30, 10 ** 3, 260098, 4 * 10 ** 6])
def test_student_t_sf_matches_scipy(df):
    stats = pytest.importorskip("scipy.stats")
    for t in (0, 1e-8, 0.5, 1, 3, 7, 10, 40):
        ref = float(stats.t.sf(t, df))
        got = correlation.student_t_sf(t, df)
        if ref > 1e-300:
            assert abs(got - ref) <= 1e-10 * ref, (df, t, got, ref)
        got_neg = correlation.student_t_sf(-t, df)
        assert abs(got_neg - float(stats.t.sf(-t, df))) <= 1e-12


def test_student_t_sf_special_values():
    assert math.isnan(correlation.student_t_sf(math.nan, 5))
    assert math.isnan(correlation.student_t_sf(1.0, math.nan))
    assert math.isnan(correlation.student_t_sf(1.0, -1))
    assert correlation.student_t_sf(0.0, 260098) == 0.5
    assert correlation.student_t_sf(math.inf, 260098) == 0.0
    assert correlation.student_t_sf(-math.inf, 3) == 1.0
    # the far tail of the fixtures: pair 9, identity filter (cor given to 13 digits: ~1e-11 relative in p)
    assert abs(correlation.student_t_sf(0.01881180388869 / math.sqrt(1 - 0.01881180388869 ** 2) * math.sqrt(260098), 260098)
               - 4.203069912237e-22) <= 1e-9 * 4.2e-22


def test_p_value_formula():
    n = 260100
    assert correlation.p_value(0.0, n) == 0.5
    assert correlation.p_value(1.0, n) == 0.0 and correlation.p_value(-1.0, n) == 0.0
    for c in (1.0000001, -1.5, 3.0, math.inf, math.nan):
        assert math.isnan(correlation.p_value(c, n))
    arr = correlation.p_value(np.array([[0.01, -0.01], [2.0, np.nan]]), n)
    assert arr.shape == (2, 2) and arr[0, 0] == arr[0, 1] and np.isnan(arr[1]).all()
    stats = pytest.importorskip("scipy.stats")
    for c in (1e-4, 0.0134, -0.3, 0.999):
        assert abs(correlation.p_value(c, n) - corr_np.p_value(c, n)) <= 1e-10 * corr_np.p_value(c, n) + 1e-300
    assert stats is not None


def _frame(model, rows):
    return pd.DataFrame([{"name_c": f"images/{i}.png", "name_s": f"stego/{i}.png", "correlation": c, "p-value": p}
                         for i, (c, p) in enumerate(rows)]).assign(model_name=model)


def test_table_layout(tmp_path):
    frames = [_frame("KB", [(0.3, 0.1), (np.nan, np.nan), (0.1, 0.3)]),
              _frame("1", [(0.5, 0.2), (0.7, 0.4), (0.6, np.nan)]),
              _frame("AVG9", [(np.nan, np.nan), (np.nan, np.nan)]),
              _frame("AVG", [(-1.0, 0.9), (1.0, 0.7), (0.0, 0.8), (2.0, 0.6)])]
    t = correlation.table(frames)
    assert list(t.columns) == ["KB", "1", "AVG9", "AVG"] and list(t.index) == ["correlation", "p-value"]
    assert t.loc["correlation", "KB"] == pytest.approx(0.2) and t.loc["p-value", "KB"] == pytest.approx(0.2)       # NaN skipped
    assert t.loc["correlation", "1"] == pytest.approx(0.6) and t.loc["p-value", "1"] == pytest.approx(0.3)
    assert np.isnan(t.loc["correlation", "AVG9"])
    assert t.loc["correlation", "AVG"] == pytest.approx(0.5) and t.loc["p-value", "AVG"] == pytest.approx(0.75)
    out = tmp_path / "c.csv"
    correlation.table([_frame("1", [(0.25, 0.5)]), _frame("AVG9", [(0.125, 0.75)])]).to_csv(out)
    assert out.read_text().splitlines() == [",1,AVG9", "correlation,0.25,0.125", "p-value,0.5,0.75"]


def test_argument_errors_without_gpu(lib):
    assert lib.wsu_pair_correlation_workspace_bytes(3) == 3 * 64 * 6 * 8
    ws = lib.wsu_pair_correlation_workspace_bytes(1)
    taps = (ctypes.c_double * 9)()
    call = lib.wsu_pair_correlation
    assert call(None, 1, None, taps, 1, 255., 1, None, 1, ws, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert call(1, None, None, taps, 1, 255., 1, None, 1, ws, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert call(1, 1, None, taps, 1, 255., None, None, 1, ws, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert call(1, 1, None, taps, 1, 255., 1, None, None, ws, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert call(1, 1, None, None, 1, 255., 1, None, 1, ws, 1, 8, 8, None) == -1 and b"exactly one" in lib.wsu_last_error()
    assert call(1, 1, 1, taps, 1, 255., 1, None, 1, ws, 1, 8, 8, None) == -1 and b"exactly one" in lib.wsu_last_error()
    assert call(1, 1, 1, None, 2, 255., 1, None, 1, ws, 1, 8, 8, None) == -1 and b"hat_full=2" in lib.wsu_last_error()
    assert call(1, 1, 1, None, -1, 255., 1, None, 1, ws, 1, 8, 8, None) == -1 and b"hat_full=-1" in lib.wsu_last_error()
    assert call(1, 1, None, taps, 1, 255., 1, None, 1, ws, 1, 2, 8, None) == -1 and b"h=2" in lib.wsu_last_error()
    assert call(1, 1, None, taps, 1, 255., 1, None, 1, ws, 1, 8, 2, None) == -1 and b"w=2" in lib.wsu_last_error()
    assert call(1, 1, None, taps, 1, 255., 1, None, 1, ws, 0, 8, 8, None) == -1 and b"n=0" in lib.wsu_last_error()
    assert call(1, 1, None, taps, 1, 255., 1, None, 1, ws - 1, 1, 8, 8, None) == -1 and b"workspace" in lib.wsu_last_error()
    assert call(1, 1, None, taps, 1, 255., 1, None, 1, ws, 2, 8, 8, None) == -1 and b"workspace" in lib.wsu_last_error()


def _read(path):
    from PIL import Image
    return np.array(Image.open(path))


def test_numpy_restatement_reproduces_kat():
    pytest.importorskip("scipy.stats")
    kat = json.loads((GOLDEN / "correlation_kat.json").read_text())
    n = kat["n"]
    exact = {"1": filters.NAMED_FILTERS_2D["1"], "AVG9": np.ones((3, 3)) / 9, "AVG": filters.NAMED_FILTERS_2D["AVG"],
             "KB": filters.NAMED_FILTERS_2D["KB"]}
    meds = {m: [] for m in exact}
    for k in PAIRS:
        xc, xs = _read(GOLDEN / f"cover_{k}.png"), _read(GOLDEN / f"stego_LSBR_1.0_{k}.png")
        assert xc.shape == xs.shape == (512, 512) and (xc != xs).any()
        for m, kern in exact.items():
            want = kat["per_pair"][f"images/{k}.png"][m]
            cor = corr_np.correlation(xc, xs, corr_np.filter_hat(xs, kern))
            assert abs(cor - want["correlation"]) <= 1e-14 + 1e-11 * abs(want["correlation"]), (k, m, cor)
            assert abs(corr_np.p_value(cor, n) - want["p-value"]) <= 1e-11 * want["p-value"], (k, m)
            meds[m].append(cor)
    pub = kat["published"]
    for m in exact:
        assert abs(np.median(meds[m]) - pub["correlation"][pub["columns"].index(m)]) <= 6e-10


def _dataset(root, pairs=PAIRS, stego_pairs=PAIRS):
    (root / "images").mkdir(parents=True)
    sdir = root / "stego_LSBR_alpha_1.0_independent_images"
    sdir.mkdir()
    for k in pairs:
        shutil.copyfile(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")           # (the fixtures are read-only)
    for k in stego_pairs:
        shutil.copyfile(GOLDEN / f"stego_LSBR_1.0_{k}.png", sdir / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in pairs))
    (sdir / "files.csv").write_text("name,height,width,stego_method,alpha\n" + "".join(
        f"{sdir.name}/{k}.png,512,512,LSBR,1.0\n" for k in stego_pairs))
    return sdir


@pytest.mark.parametrize("iterator", ["python", "batched"])
def test_run_input_errors_before_any_device_work(tmp_path, iterator):
    """a cover without a stego twin and a colour image raise ValueError naming the file (the reference crashes on a path built from
    NaN / broadcasts the colour channels); both are found before anything is decoded or uploaded"""
    _dataset(tmp_path / "a", stego_pairs=(6, 7, 8, 9))                   # 10 is the first pair in fabrika's order
    pred = filters.get_filter_estimator(filter_name="KB", flatten=False)
    with pytest.raises(ValueError, match=r"images/10\.png has no stego twin"):
        correlation.run(tmp_path / "a", stego_method="LSBR", alpha=1.0, predictor=pred, iterator=iterator)
    sdir = _dataset(tmp_path / "b")
    from PIL import Image
    Image.open(GOLDEN / "stego_LSBR_1.0_10.png").convert("RGB").save(sdir / "10.png")
    with pytest.raises(ValueError, match=r"10\.png: a RGB image"):
        correlation.run(tmp_path / "b", stego_method="LSBR", alpha=1.0, predictor=pred, iterator=iterator)
    with pytest.raises(ValueError, match="predictor"):
        correlation.run(tmp_path / "b", stego_method="LSBR", alpha=1.0, iterator=iterator)
