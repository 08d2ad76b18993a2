"""GPU: the KB-stratified absolute-error box table (K16-K18, ws_unet_amd/error_boxes.py) against the published
results/prediction/ae_boxes_3.csv and the literal numpy / pandas restatement of the reference's plot_error (tests/boxes_np.py)."""
import os
import pathlib
import shutil
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import boxes_np
from conftest import GOLDEN, ROOT
from gpu_util import DEV, OUT_ATOL, gpu_model
from oracle import evaluate_ref, unet_ref
from ws_unet_amd import error_boxes, formula, ops

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
STATS = list(error_boxes.STATS)


def _covers_dataset(root):
    (root / "images").mkdir(parents=True)
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    (root / "split_te.csv").write_text("name,height,width\nimages/10.png,512,512\n")        # the reference's test split: one cover
    return root


def _planes(ks=COVERS):
    from PIL import Image
    return np.stack([np.array(Image.open(GOLDEN / f"cover_{k}.png")) for k in ks])


def _filter_ae(x, name):
    """|y - x @ f| of the reference on the interior, float64 (exact: dyadic taps)."""
    t = error_boxes.filter_taps(error_boxes.filters.NAMED_FILTERS[name]).reshape(3, 3)
    x = x.astype(np.float64)
    h, w = x.shape
    hat = sum(t[a, b] * x[a:h - 2 + a, b:w - 2 + b] for a in range(3) for b in range(3))
    return np.abs(x[1:-1, 1:-1] - hat)


def _assert_same(got, want):
    got, want = got.reset_index(drop=True), want.reset_index(drop=True)
    assert list(got.columns) == list(want.columns)
    assert got["Type"].tolist() == want["Type"].tolist()
    assert got["edge_interval"].tolist() == want["edge_interval"].tolist()
    for c in STATS:
        g, w = got[c].to_numpy(np.float64), want[c].to_numpy(np.float64)
        assert np.array_equal(g, w, equal_nan=True), (c, g, w)


def test_run_reproduces_published_filter_rows(tmp_path):
    data = _covers_dataset(tmp_path)
    pub = pd.read_csv(GOLDEN / "ae_boxes_3.csv", float_precision="round_trip")
    pub = pub[pub["Type"].isin(["AVG", "KB"])].reset_index(drop=True)
    got = error_boxes.run(data).reset_index(drop=True)
    _assert_same(got, pub)
    assert pub[STATS].size == 70
    # the CLI writes those rows unchanged
    out = tmp_path / "out" / "ae_boxes_3.csv"
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-m", "ws_unet_amd.error_boxes", "--data", str(data), "--out", str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = (GOLDEN / "ae_boxes_3.csv").read_text().splitlines()
    assert out.read_text().splitlines() == [ln for ln in lines if ln.split(",")[0] in ("Type", "AVG", "KB")]


def _synthetic(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "ties":
        a = rng.integers(0, 48, n) / 4.0                        # quarters: heavy ties, values exactly at every edge
        return {"KB": a, "AVG": rng.integers(0, 800, n) / 8.0, "U": rng.integers(0, 3, n).astype(np.float64)}
    if kind == "no_low":
        a = 0.75 + rng.integers(0, 60, n) / 4.0                 # no anchor <= 0.5: slice 0 = ranks [0, N-1), overlapping the others
    elif kind == "all_low":
        a = rng.integers(0, 31, n) / 4.0                        # all <= 7.5: the last slice is the single largest key
    elif kind == "empty":
        a = np.where(rng.random(n) < 0.5, 0.25, 10.0)           # nothing in (0.5, 7.5]: empty middle slices (NaN rows)
    else:
        a = rng.integers(0, 200, n) / 8.0
    u = (rng.random(n) * 40).astype(np.float32).astype(np.float64)
    return {"KB": a, "AVG": rng.integers(0, 800, n) / 8.0, "UNet": u}


@pytest.mark.parametrize("kind,n", [("ties", 50_000), ("ties", 7), ("no_low", 10_000), ("all_low", 10_000), ("empty", 5_000),
                                    ("mixed", 1), ("mixed", 2), ("no_low", 3), ("all_low", 2)])
def test_box_table_equals_restatement_synthetic(kind, n):
    res = _synthetic(kind, n, seed=n)
    _assert_same(error_boxes.box_table(res, "KB"), boxes_np.table(res, "KB"))


def test_box_table_equals_restatement_on_covers():
    x = _planes()
    res = {name: np.stack([_filter_ae(p, name) for p in x]) for name in ("KB", "AVG")}
    got = error_boxes.box_table(res, "KB")
    _assert_same(got, boxes_np.table(res, "KB"))
    # device tensors in, same table
    dev = {k: torch.from_numpy(v.astype(np.float32)).to(DEV) for k, v in res.items()}
    _assert_same(error_boxes.box_table(dev, "KB"), got)


def test_box_table_beyond_float_counters():
    n = 23_000_000
    rng = np.random.default_rng(24)
    a = np.where(rng.random(n) < 0.995, 12.0, rng.integers(0, 40, n) / 4.0)  # one slice of > 2^24 pixels, its anchor all one value
    u = (rng.integers(0, 1 << 20, n) / 1024.0).astype(np.float32)
    res = {"KB": a.astype(np.float32), "UNet": u}
    last = n - int((a <= 7.5).sum()) + 1                                       # the 7.5-inf slice: ranks [c_3 - 1, N)
    assert last > (1 << 24) and error_boxes.quantile_index(last, .75)[0] > (1 << 24)   # its size and its q75 rank exceed 2^24
    got = error_boxes.box_table(res, "KB")
    _assert_same(got, boxes_np.table_numpy(res, "KB"))


def test_determinism_and_batch_independence(tmp_path):
    data = _covers_dataset(tmp_path)
    frames = [error_boxes.run(data, split=None, batch_size=bs) for bs in (1, 2, 5) for _ in range(2)]
    frames.append(error_boxes.run(data, split=None, iterator="python"))
    for f in frames[1:]:
        _assert_same(f, frames[0])
    # and the restatement of the same pixels, in fabrika's order
    order = [int(p.stem) for p in error_boxes.fabrika.precovers(iterator=None, convert_to=None)(lambda df, **kw: df)(
        data, shuffle_seed=12345)["name"].map(pathlib.Path)]
    x = _planes(order)
    res = {name: np.stack([_filter_ae(p, name) for p in x]) for name in ("KB", "AVG")}
    _assert_same(frames[0], boxes_np.table(res, "KB"))


def test_num_pixels_equals_subset_residual(tmp_path):
    data = _covers_dataset(tmp_path)
    got = error_boxes.run(data, split=None, num_pixels=1000)
    order = error_boxes.fabrika.precovers(iterator=None, convert_to=None)(lambda df, **kw: df)(data, shuffle_seed=12345)["name"].tolist()
    from PIL import Image
    res = {}
    for name in ("KB", "AVG"):
        res[name] = np.stack([error_boxes.subset_residual(_filter_ae(np.array(Image.open(f)), name), f, 1000) for f in order])
    _assert_same(got, boxes_np.table(res, "KB"))
    # the reference's per-image API gives the same arrays
    mae = error_boxes.filter_mae("gray", (3,), "KB", data_path=data, num_pixels=1000)
    assert list(mae) == ["KB_3"] and mae["KB_3"].shape == (1, 1000)


@pytest.mark.parametrize("mode", ["f32", None])
def test_unet_column(tmp_path, mode):
    x = _planes()
    model = gpu_model(2, "he", mode, drop_rate=0.)
    xd = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        y = model(ops.u8_to_unit(xd)[:, None])[:, 0].contiguous()
    keys = torch.empty(5 * 510 * 510, dtype=torch.float32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.ae_values(xd, keys, 0, flag, x_hat=y, hat_scale=255.)
    assert int(flag.item()) == 0
    yh = y.cpu().numpy()
    want = np.abs(x[:, 1:-1, 1:-1].astype(np.float32) - (yh[:, 1:-1, 1:-1] * np.float32(255.))).reshape(-1)
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # the table through run(), against the CPU oracle's AE
    data = _covers_dataset(tmp_path)
    got = error_boxes.run(data, {"KB": "KB", "AVG": "AVG", "UNet": model}, split=None)
    order = error_boxes.fabrika.precovers(iterator=None, convert_to=None)(lambda df, **kw: df)(data, shuffle_seed=12345)["name"].tolist()
    from PIL import Image
    xo = np.stack([np.array(Image.open(f)) for f in order])
    ref_model = unet_ref.build_ref(2, formula.formula_state_dict(2, "he"))
    u = np.stack([np.abs(p[1:-1, 1:-1].astype(np.float32) - evaluate_ref.infere_single(p[..., None].astype(np.float32), ref_model)[..., 0])
                  for p in xo])
    res = {"KB": np.stack([_filter_ae(p, "KB") for p in xo]), "AVG": np.stack([_filter_ae(p, "AVG") for p in xo]), "UNet": u}
    want_t = boxes_np.table(res, "KB").reset_index(drop=True)
    got = got.reset_index(drop=True)
    filt = got["Type"] != "UNet"
    _assert_same(got[filt], want_t[filt])
    if mode == "f32":
        d = np.abs(got.loc[~filt, STATS].to_numpy(np.float64) - want_t.loc[~filt, STATS].to_numpy(np.float64))
        assert d.max() <= OUT_ATOL["f32"] * 255, d.max()


def test_errors(tmp_path):
    with pytest.raises(ValueError, match="not exact"):
        error_boxes.run(_covers_dataset(tmp_path / "a"), {"KB": "KB", "AVG9": np.ones((8, 1)) / 9.})
    with pytest.raises(ValueError, match="anchor"):
        error_boxes.run(tmp_path / "a", {"AVG": "AVG"})
    with pytest.raises(ValueError, match="anchor"):
        error_boxes.box_table({"AVG": np.ones(4)}, "KB")
    with pytest.raises(ValueError, match="count"):
        ops.ae_slices(torch.zeros(4, device=DEV), [0.5], count=5)
    with pytest.raises(ValueError, match="UNet: NaN or infinite"):
        error_boxes.box_table({"KB": np.ones(4), "UNet": np.array([1.0, np.nan, 2.0, 3.0])}, "KB")
    with pytest.raises(ValueError, match="UNet: negative, NaN or infinite"):
        error_boxes.box_table({"KB": np.ones(4), "UNet": torch.tensor([1.0, float("nan"), 2.0, 3.0], device=DEV)}, "KB")

    class NanNet(torch.nn.Module):
        def forward(self, x):
            return torch.full_like(x, float("nan"))
    with pytest.raises(ValueError, match="NanNet_p: NaN or infinite"):
        error_boxes.run(tmp_path / "a", {"KB": "KB", "NanNet_p": NanNet()}, split=None)
    # ragged sizes
    d = tmp_path / "b"
    _covers_dataset(d)
    from PIL import Image
    Image.fromarray(_planes((6,))[0][:300, :400]).save(d / "images" / "6.png")
    (d / "images" / "files.csv").write_text("name,height,width\n" + "".join(
        f"images/{k}.png,{300 if k == 6 else 512},{400 if k == 6 else 512}\n" for k in COVERS))
    with pytest.raises(ValueError, match="different sizes"):
        error_boxes.run(d, split=None)
