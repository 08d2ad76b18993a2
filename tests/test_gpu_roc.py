"""GPU: the detection ROC / AUC tables (ws_unet_amd.ws.roc, K19 wsu_roc_counts) -- the published AVG, KB and B0_0.01 rows and curves
of results/detection/auc_0.01.csv / roc_0.01.csv end to end and through the CLI, collect_ws_scores against ws.estimate.run, and K19
against the numpy sweep (tests/roc_np.py)."""
import json
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

import roc_np
from conftest import GOLDEN
from ws_unet_amd import formula, ops
from ws_unet_amd.ws import estimate, roc

pytestmark = pytest.mark.gpu

ALPHAS = (.1, .05, .01)
IMAGES = (6, 7, 8, 9, 10)


def _dataset(root):
    """The reference's data layout: images/ and one stego_LSBR_alpha_<a>_independent_images/ per alpha, each with its files.csv."""
    (root / "images").mkdir(parents=True)
    for k in IMAGES:
        shutil.copyfile(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")         # (the fixtures are read-only)
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in IMAGES))
    for a in ALPHAS:
        sdir = root / f"stego_LSBR_alpha_{a}_independent_images"
        sdir.mkdir()
        for k in IMAGES:
            shutil.copyfile(GOLDEN / f"stego_LSBR_{a}_{k}.png", sdir / f"{k}.png")
        (sdir / "files.csv").write_text("name,height,width,stego_method,alpha\n" + "".join(
            f"{sdir.name}/{k}.png,512,512,LSBR,{a}\n" for k in IMAGES))
    return root


def _published():
    return (pd.read_csv(GOLDEN / "auc_0.01.csv", float_precision="round_trip"),
            pd.read_csv(GOLDEN / "roc_0.01.csv", float_precision="round_trip"))


PINNED = ["AVG", "B0_0.01", "KB"]
CURVES = [f"{r}_LSBR_{m}" for r in ("tpr", "fpr") for m in PINNED]


def _check_pins(auc, curves):
    pa, pr = _published()
    want = pa[pa.model_name.isin(PINNED)].reset_index(drop=True)
    got = auc[auc.model_name.isin(PINNED)].reset_index(drop=True)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert len(curves) == 501
    for c in CURVES:
        np.testing.assert_array_equal(curves[c].to_numpy(), pr[c].to_numpy(), err_msg=c)


def test_published_tables_end_to_end(tmp_path):
    data = _dataset(tmp_path / "data")
    ws = roc.collect_ws_scores(data, ["LSBR"], list(ALPHAS), ("AVG", "KB"))
    assert len(ws) == 2 * 5 * 4 and set(ws.model_name) == {"AVG", "KB"}
    # every positive WS estimate is clear of every threshold, so K11's exact sums and the reference's FFT convolution (noise ~1e-7) agree
    # on all counts; a 0 is K11's clip of a negative estimate (the reference's clip in attack), at least 1.25e-4 below 0 on these images
    b = ws["beta_hat"].to_numpy(np.float64)
    assert (b >= 0).all() and (b == 0).sum() < len(b)
    assert np.abs(b[b > 0][:, None] - roc.TAUS[None, :]).min() >= 1e-5
    res = pd.concat([ws, roc.load_scores(GOLDEN / "b0.csv", "B0_0.01", ["LSBR"], list(ALPHAS))]).reset_index(drop=True)
    res["stego_method"] = res["stego_method"].fillna("Cover")
    res["alpha"] = res["alpha"].fillna(0.)
    df_roc = roc.produce_roc(res)
    _check_pins(roc.auc_table(df_roc), roc.roc_table(df_roc))
    # and the whole frame is the reference's loop on the same estimates
    pd.testing.assert_frame_equal(df_roc.reset_index(drop=True), roc_np.produce_roc(res).reset_index(drop=True), check_exact=True)


def test_cli_writes_the_published_rows(tmp_path):
    data = _dataset(tmp_path / "data")
    out = tmp_path / "detection"
    roc.main(["--data", str(data), "--out-dir", str(out), "--scores", str(GOLDEN / "b0.csv"), "B0_0.01"])
    assert sorted(p.name for p in out.iterdir()) == ["auc_0.01.csv", "roc_0.01.csv"]
    auc = pd.read_csv(out / "auc_0.01.csv", float_precision="round_trip")
    curves = pd.read_csv(out / "roc_0.01.csv", float_precision="round_trip")
    assert list(auc.columns) == roc.AUC_COLUMNS and auc.model_name.tolist() == PINNED
    _, pr = _published()
    assert list(curves.columns) == [c for c in pr.columns if c in curves.columns] == [
        "tpr_LSBR_AVG", "tpr_LSBR_B0_0.01", "tpr_LSBR_KB", "fpr_LSBR_AVG", "fpr_LSBR_B0_0.01", "fpr_LSBR_KB"]
    _check_pins(auc, curves)


def _unet_dir(root):
    run = root / "LSBR" / "run-a"
    (run / "model").mkdir(parents=True)
    (run / "config.json").write_text(json.dumps({"stego_method": "LSBR", "alpha": "0.400", "loss": "l1ws", "network": "unet_2",
                                                 "drop_rate": 0.0, "debug": False}))
    sd = formula.formula_state_dict(2, "he")
    torch.save({"epoch": 1, "state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, run / "model" / "best_model.pt.tar")
    return root / "LSBR", "run-a"


def test_collect_ws_scores_equals_the_per_predictor_runs(tmp_path):
    data = _dataset(tmp_path / "data")
    model_path, model_name = _unet_dir(tmp_path / "models")
    got = roc.collect_ws_scores(data, ["LSBR"], list(ALPHAS), ("AVG", "KB"), unet=(model_path, model_name))
    runs = []
    for stego_method, alpha in [(None, None)] + [("LSBR", a) for a in ALPHAS]:
        for name in ("AVG", "KB", model_name):
            runs.append(estimate.run(data, stego_method, alpha, name, model_path, (3,), weighted=0, correct_bias=False, batched=True))
    want = pd.concat(runs).reset_index(drop=True)
    want["stego_method"] = want["stego_method"].fillna("Cover")
    want["alpha"] = want["alpha"].fillna(0.)
    assert list(got.columns) == list(want.columns) and len(got) == 3 * 20
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert got.model_name.tolist()[:15] == ["AVG"] * 5 + ["KB"] * 5 + ["UNet"] * 5


# ---- K19 against the numpy sweep -------------------------------------------------------------------------------------------------

def _k19(y_hats, labels, taus):
    off = np.concatenate([[0], np.cumsum([len(s) for s in y_hats])]).astype(np.int64)
    s = torch.from_numpy(np.concatenate(y_hats).astype(np.float64)).cuda()
    lab = torch.from_numpy(np.concatenate(labels).astype(np.int8)).cuda()
    return ops.roc_counts(s, lab, off, taus).cpu().numpy()


def _check(y_hats, labels, taus):
    got = _k19(y_hats, labels, taus)
    np.testing.assert_array_equal(got, roc_np.group_counts(y_hats, labels, taus))
    return got


def test_k19_random_groups_of_unequal_size_one_empty():
    rng = np.random.default_rng(1)
    sizes = [1000, 0, 37, 70001, 1]
    ys = [rng.uniform(-0.2, 1.2, n) for n in sizes]
    ls = [rng.integers(0, 2, n) for n in sizes]
    got = _check(ys, ls, roc_np.TAUS)
    assert (got[1] == 0).all() and got.shape == (5, 501, 4)


def test_k19_scores_on_the_thresholds_special_values_and_grids():
    rng = np.random.default_rng(2)
    t501 = roc_np.TAUS
    on = np.concatenate([t501, t501[::7], [0.5, 0.0, 1.0]])
    lab_on = rng.integers(-1, 2, on.size)
    special = np.array([np.nan, np.inf, -np.inf, 0.5, np.nan, 2.0, -1.0, 0.25])
    lab_sp = np.array([1, 1, 0, -1, 0, 0, 1, -1])
    for taus in (np.array([0.5]), t501, np.sort(np.concatenate([rng.uniform(-1, 2, 4000), t501[::5]]))[:4096]):
        assert np.all(np.diff(taus) > 0)
        got = _check([on, special, rng.normal(0.5, 0.5, 5000)], [lab_on, lab_sp, rng.integers(-1, 2, 5000)], taus)
        assert got.shape[1] == len(taus)
    t4096 = np.unique(np.concatenate([np.linspace(-1, 2, 3000) ** 3, rng.uniform(0, 1, 1096)]))[:4096]
    assert t4096.size == 4096                                        # LDS beyond 64 KiB: 32 768 B of taus + 32 776 B of bins
    _check([rng.uniform(-1, 8, 20000), t4096[::3]], [rng.integers(0, 2, 20000), rng.integers(0, 2, t4096[::3].size)], t4096)


def test_k19_one_bin_contention():
    n = 1 << 25
    s = torch.zeros(n, dtype=torch.float64, device="cuda")
    lab = torch.zeros(n, dtype=torch.int8, device="cuda")
    lab[::3] = 1
    got = ops.roc_counts(s, lab, [0, n], roc_np.TAUS).cpu().numpy()
    pos = (n + 2) // 3
    want = np.zeros((1, 501, 4), dtype=np.int64)
    want[0, :, 2], want[0, :, 3] = n - pos, pos                        # every score at or below every tau >= 0
    np.testing.assert_array_equal(got, want)


def test_k19_deterministic_and_split_independent():
    rng = np.random.default_rng(4)
    ys = [rng.uniform(0, 1, n) for n in (300000, 12345, 77777)]
    ls = [rng.integers(-1, 2, y.size) for y in ys]
    a, b = _k19(ys, ls, roc_np.TAUS), _k19(ys, ls, roc_np.TAUS)
    assert np.array_equal(a, b)
    split = np.concatenate([_k19(ys[:1], ls[:1], roc_np.TAUS), _k19(ys[1:], ls[1:], roc_np.TAUS)])
    assert np.array_equal(a, split)


def test_roc_counts_argument_errors():
    s = torch.zeros(4, dtype=torch.float64, device="cuda")
    lab = torch.zeros(4, dtype=torch.int8, device="cuda")
    with pytest.raises(ValueError, match="float64"):
        ops.roc_counts(s.float(), lab, [0, 4], roc_np.TAUS)
    with pytest.raises(ValueError, match="int8"):
        ops.roc_counts(s, lab.to(torch.int32), [0, 4], roc_np.TAUS)
    with pytest.raises(ValueError, match="GPU"):
        ops.roc_counts(s.cpu(), lab, [0, 4], roc_np.TAUS)
    with pytest.raises(ValueError, match="contiguous"):
        ops.roc_counts(torch.zeros(8, dtype=torch.float64, device="cuda")[::2], lab, [0, 4], roc_np.TAUS)
    with pytest.raises(ValueError, match="offsets"):
        ops.roc_counts(s, lab, [0, 3], roc_np.TAUS)
