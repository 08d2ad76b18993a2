"""CPU: the host side of the detection ROC tables (ws_unet_amd.ws.roc) -- the fp64 step from confusion counts to the reference's frame
against the reference's own loop (tests/roc_np.py), the published B0 row from its scores, the CSV layouts, the K19 C-ABI argument
checks and the CLI's input errors."""
import ctypes
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import roc_np
from conftest import GOLDEN
from ws_unet_amd.ws import roc

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    so = ROOT / "ws_unet_amd" / "libwsu.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(ROOT / "ws_unet_amd" / "csrc"), "-j4"], check=True)
    from ws_unet_amd import _lib
    return _lib.load()


def _host_roc(df_ws):
    """produce_roc with the K19 counts replaced by roc_np's: everything the host does, nothing the device does."""
    groups = roc._groups(df_ws)
    ktaus, _, _ = roc._kernel_taus(roc.TAUS)
    counts = roc_np.group_counts([g[2] for g in groups], [g[3] for g in groups], ktaus)
    return roc._roc_frame(groups, counts, roc.TAUS)


def _ws_rows(model, stego_method, alpha, betas):
    return pd.DataFrame({"name": [f"{stego_method}/{i}.png" for i in range(len(betas))], "stego_method": stego_method,
                         "alpha": alpha, "model_name": model, "beta_hat": np.asarray(betas, dtype=np.float32)})


def _b0_rows(model, stego_method, alpha, scores):
    return pd.DataFrame({"name": [f"{stego_method}/{i}.png" for i in range(len(scores))], "stego_method": stego_method,
                         "alpha": alpha, "model_name": model, "score": np.asarray(scores, dtype=np.float64)})


def _cases():
    rng = np.random.default_rng(7)
    t = roc.TAUS
    cases = {}
    # mixed: two methods, pooled alphas, float32 estimates (some negative: clipped), B0 scores, scores ON grid values and at 0.5
    cases["mixed"] = pd.concat([
        _ws_rows("AVG", "Cover", 0., rng.normal(0.01, 0.03, 40)),
        _ws_rows("AVG", "LSBR", .1, rng.normal(0.05, 0.03, 20)), _ws_rows("AVG", "LSBR", .01, rng.normal(0.01, 0.03, 20)),
        _ws_rows("AVG", "HILLR", .1, list(t[[0, 3, 250, 251, 499, 500]]) + [0.5, -1.0, 2.0]),
        _b0_rows("B0_0.01", "Cover", 0., rng.uniform(0.3, 0.6, 30)), _b0_rows("B0_0.01", "LSBR", .05, list(rng.uniform(0.4, 0.9, 25)) + [0.5, 1.0, 0.0]),
    ]).reset_index(drop=True)
    # a class empty everywhere: a model with no covers (fpr 0/0) and a method with alpha 0 (no positives: tpr 0/0, NaN inside the argmin)
    cases["empty_class"] = pd.concat([
        _ws_rows("KB", "LSBR", .1, rng.uniform(0, 0.2, 12)),
        _ws_rows("AVG", "Cover", 0., rng.uniform(0, 0.2, 12)), _ws_rows("AVG", "LSBR", 0., rng.uniform(0, 0.2, 12)),
    ]).reset_index(drop=True)
    # bins.sum() == 0: every cover clipped to 0, so fpr is 0 at every tau
    cases["flat_fpr"] = pd.concat([_ws_rows("KB", "Cover", 0., -rng.uniform(0, 1, 10)), _ws_rows("KB", "LSBR", .4, rng.uniform(0, 1, 10))]).reset_index(drop=True)
    # argmin ties: well separated classes give a plateau of the minimum
    cases["ties"] = pd.concat([_ws_rows("KB", "Cover", 0., [0.001, 0.002, 0.003]), _ws_rows("KB", "LSBR", .4, [0.3, 0.31, 0.32])]).reset_index(drop=True)
    # stale FN: every positive in (0, 0.5] -> tpr_50 = 0 / (0 + 0) = NaN in the reference (an honest FN would give 0) ...
    cases["stale_nan"] = pd.concat([_ws_rows("KB", "Cover", 0., [-0.1, 0.01, 0.6]), _ws_rows("KB", "LSBR", .4, [0.1, 0.2, 0.5, 1e-6])]).reset_index(drop=True)
    # ... and positives at 0, in (0, 0.5] and above 0.5: the stale and the honest value differ
    cases["stale_mixed"] = pd.concat([_ws_rows("KB", "Cover", 0., [0.0, 0.7]), _ws_rows("KB", "LSBR", .4, [-0.2, -0.1, 0.3, 0.4, 0.8])]).reset_index(drop=True)
    # NaN scores and NaN labels: in none of the counts
    cases["nan"] = pd.concat([_b0_rows("B0_x", "Cover", 0., [0.2, np.nan, 0.7]), _b0_rows("B0_x", "LSBR", .1, [0.6, np.nan, 0.9, 0.3]),
                              _b0_rows("B0_x", "LSBR", np.nan, [0.95, 0.1])]).reset_index(drop=True)
    return cases


CASES = _cases()


@pytest.mark.parametrize("case", sorted(CASES))
def test_counts_to_frame_matches_the_reference_loop(case):
    df = CASES[case]
    got, want = _host_roc(df), roc_np.produce_roc(df)
    pd.testing.assert_frame_equal(got.reset_index(drop=True), want.reset_index(drop=True), check_exact=True)
    if case == "stale_nan":
        assert math.isnan(got["tpr_50"].iloc[0]) and got["fpr_50"].iloc[0] == 1 / 3
    if case == "stale_mixed":
        assert got["tpr_50"].iloc[0] == 1 / 3                     # TP_0.5 = 1, stale FN (tau = 0) = 2; the honest FN_0.5 would give 1/5
    if case == "flat_fpr":
        assert np.isnan(got["auc"]).all()
    if case == "empty_class":
        kb = got[got.model_name == "KB"]
        assert np.isnan(kb["fpr"]).all() and np.isnan(kb["auc"]).all()
        avg = got[got.model_name == "AVG"]
        assert np.isnan(avg["tpr"]).all() and (avg["tau0"] == 1.0).all()          # argmin of all-NaN: the first index (tau = 1)


def _published():
    auc = pd.read_csv(GOLDEN / "auc_0.01.csv", float_precision="round_trip")
    curves = pd.read_csv(GOLDEN / "roc_0.01.csv", float_precision="round_trip")
    return auc, curves


def test_published_b0_row_from_its_scores():
    """the B0_0.01 row and curve of the published tables, bit for bit, from results/detection/b0.csv (covers + LSBR 0.1 / 0.05 / 0.01)"""
    b0 = roc.load_scores(GOLDEN / "b0.csv", "B0_0.01", ["LSBR"], [.1, .05, .01])
    assert len(b0) == 20 and list(b0["stego_method"].iloc[:5].isna()) == [True] * 5
    df = b0.assign(stego_method=b0["stego_method"].fillna("Cover"), alpha=b0["alpha"].fillna(0.)).reset_index(drop=True)
    got = _host_roc(df)
    auc, curves = _published()
    want = auc[auc.model_name == "B0_0.01"].reset_index(drop=True)
    pd.testing.assert_frame_equal(roc.auc_table(got).reset_index(drop=True), want, check_exact=True)
    table = roc.roc_table(got)
    for c in ("tpr_LSBR_B0_0.01", "fpr_LSBR_B0_0.01"):
        np.testing.assert_array_equal(table[c].to_numpy(), curves[c].to_numpy())


def test_table_layouts():
    names = ["AVG", "B0_0.01", "KB", "UNet", "ns-r-B0_0.01"]
    rng = np.random.default_rng(3)
    parts = []
    for m in names:
        rows = _b0_rows if "B0" in m else _ws_rows
        parts += [rows(m, "Cover", 0., rng.uniform(0, 1, 4)), rows(m, "LSBR", .1, rng.uniform(0, 1, 4))]
    df_roc = _host_roc(pd.concat(parts).reset_index(drop=True))
    auc = roc.auc_table(df_roc)
    assert list(auc.columns) == roc.AUC_COLUMNS and auc["model_name"].tolist() == names
    table = roc.roc_table(df_roc)
    _, curves = _published()
    assert list(table.columns) == list(curves.columns)             # tpr_* for every model, then fpr_*, in the published order
    assert (np.diff(table.index.to_numpy()) > 0).all() and len(table) == 501
    assert list(df_roc["label"].drop_duplicates()) == ["WS-AVG", "B0_0.01", "WS-KB", "WS-UNet", "ns-r-B0_0.01"]


def test_kernel_taus_hold_the_grid_and_one_half():
    k, at_grid, at_50 = roc._kernel_taus(roc.TAUS)
    np.testing.assert_array_equal(k[at_grid], roc.TAUS)
    assert k[at_50] == 0.5 and (np.diff(k) > 0).all()
    k2, at2, at50 = roc._kernel_taus(np.array([0.1, 0.7]))
    assert k2.tolist() == [0.1, 0.5, 0.7] and at2.tolist() == [0, 2] and at50 == 1


def test_argument_errors_without_gpu(lib):
    wsb = lib.wsu_roc_counts_workspace_bytes
    assert wsb(3, 501) == 8 * (501 + 4 + 3 * 2 * 502)
    assert wsb(0, 501) == 0 and wsb(1, 0) == 0 and wsb(1, 4097) == 0 and wsb(65536, 1) == 0 and wsb(1, 4096) > 0
    call = lib.wsu_roc_counts

    def arr(ct, vals):
        return (ct * len(vals))(*vals)

    taus = arr(ctypes.c_double, [0.0, 0.5, 1.0])
    off = arr(ctypes.c_longlong, [0, 4, 10])
    ws = wsb(2, 3)

    def err(*args):
        assert call(*args) == -1
        return lib.wsu_last_error()

    assert b"null" in err(None, 1, off, 2, taus, 3, 1, 1, ws, None)
    assert b"null" in err(1, None, off, 2, taus, 3, 1, 1, ws, None)
    assert b"null" in err(1, 1, None, 2, taus, 3, 1, 1, ws, None)
    assert b"null" in err(1, 1, off, 2, None, 3, 1, 1, ws, None)
    assert b"null" in err(1, 1, off, 2, taus, 3, None, 1, ws, None)
    assert b"null" in err(1, 1, off, 2, taus, 3, 1, None, ws, None)
    assert b"groups=0" in err(1, 1, off, 0, taus, 3, 1, 1, ws, None)
    assert b"t=0" in err(1, 1, off, 2, taus, 0, 1, 1, ws, None)
    big = arr(ctypes.c_double, list(np.arange(4097) / 4097))
    assert b"t=4097" in err(1, 1, off, 2, big, 4097, 1, 1, ws, None)
    assert b"ascending" in err(1, 1, off, 2, arr(ctypes.c_double, [0.0, 1.0, 0.5]), 3, 1, 1, ws, None)
    assert b"ascending" in err(1, 1, off, 2, arr(ctypes.c_double, [0.0, 0.5, 0.5]), 3, 1, 1, ws, None)
    assert b"not finite" in err(1, 1, off, 2, arr(ctypes.c_double, [0.0, math.nan, 1.0]), 3, 1, 1, ws, None)
    assert b"not finite" in err(1, 1, off, 2, arr(ctypes.c_double, [-math.inf, 0.5, 1.0]), 3, 1, 1, ws, None)
    assert b"offsets[0]" in err(1, 1, arr(ctypes.c_longlong, [1, 4, 10]), 2, taus, 3, 1, 1, ws, None)
    assert b"decrease" in err(1, 1, arr(ctypes.c_longlong, [0, 4, 3]), 2, taus, 3, 1, 1, ws, None)
    assert b"workspace" in err(1, 1, off, 2, taus, 3, 1, 1, ws - 8, None)


def test_cli_input_errors_before_any_device_work(tmp_path):
    with pytest.raises(ValueError, match="must contain 'B0'"):
        roc.main(["--data", str(tmp_path), "--out-dir", str(tmp_path / "o"), "--scores", str(GOLDEN / "b0.csv"), "CNN_0.01"])
    bad = tmp_path / "scores.csv"
    pd.read_csv(GOLDEN / "b0.csv").drop(columns="output").to_csv(bad, index=False)
    with pytest.raises(ValueError, match="'output'"):
        roc.main(["--data", str(tmp_path), "--out-dir", str(tmp_path / "o"), "--scores", str(bad), "B0_0.01"])
    assert not (tmp_path / "o").exists()
    help_text = subprocess.run([sys.executable, "-m", "ws_unet_amd.ws.roc", "--help"], cwd=ROOT, capture_output=True, text=True).stdout
    assert "LAST" in help_text                                     # the files are named after the last alpha, all alphas pooled
