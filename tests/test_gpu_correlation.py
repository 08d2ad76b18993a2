"""GPU: the predictor / stego-change correlation (K15) against the published correlation.csv on the reference's five pairs and
against the numpy restatement (tests/corr_np.py) for every prediction source, degenerate inputs, a low-variance case, batch
independence, the UNet source against the CPU oracle, and the CLI."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import corr_np
from conftest import GOLDEN, ROOT
from gpu_util import DEV, gpu_model
from test_correlation_host import _dataset
from ws_unet_amd import correlation, filters, formula, ops
from ws_unet_amd.ws.estimate import UNetEstimator
from oracle import evaluate_ref, unet_ref

pytestmark = pytest.mark.gpu

FILTERS = ("1", "AVG9", "AVG", "KB")
KAT = json.loads((GOLDEN / "correlation_kat.json").read_text())
N_PIX = KAT["n"]


def _close_p(got, want):
    return abs(got - want) <= 1e-6 or abs(got - want) <= 1e-5 * abs(want)


def _pub(kind, model):
    return KAT["published"][kind][KAT["published"]["columns"].index(model)]


def _fixture_planes():
    from PIL import Image
    ks = (10, 6, 7, 8, 9)
    xc = np.stack([np.array(Image.open(GOLDEN / f"cover_{k}.png")) for k in ks])
    xs = np.stack([np.array(Image.open(GOLDEN / f"stego_LSBR_1.0_{k}.png")) for k in ks])
    return xc, xs


def test_fixtures_reproduce_published_table(tmp_path):
    _dataset(tmp_path)
    tables = {}
    for iterator in ("batched", "python"):
        frames = []
        for m in FILTERS:
            res = correlation.run(tmp_path, stego_method="LSBR", alpha=1.0, predictor=filters.get_filter_estimator(m, flatten=False),
                                  iterator=iterator)
            assert list(res.columns) == ["name_c", "name_s", "correlation", "p-value"]
            assert res["name_c"].tolist() == [f"images/{k}.png" for k in (10, 6, 7, 8, 9)]
            assert res["name_s"].tolist() == [f"stego_LSBR_alpha_1.0_independent_images/{k}.png" for k in (10, 6, 7, 8, 9)]
            for _, row in res.iterrows():
                want = KAT["per_pair"][row["name_c"]][m]
                assert abs(row["correlation"] - want["correlation"]) <= 2e-9, (iterator, m, row["name_c"], row["correlation"])
                assert _close_p(row["p-value"], want["p-value"]), (iterator, m, row["name_c"], row["p-value"])
            frames.append(res.assign(model_name=m))
        t = correlation.table(frames)
        assert list(t.columns) == list(FILTERS)
        for m in FILTERS:
            assert abs(t.loc["correlation", m] - _pub("correlation", m)) <= 2e-9
            assert _close_p(t.loc["p-value", m], _pub("p-value", m))
        tables[iterator] = pd.concat(frames).reset_index(drop=True)
    pd.testing.assert_frame_equal(tables["batched"], tables["python"], check_exact=True)


def _pair(h, w, change, seed):
    rng = np.random.default_rng(seed)
    xc = formula.synthetic_images(1, h, w, seed=seed)[0] if h >= 8 and w >= 8 else rng.integers(0, 256, (h, w), dtype=np.uint8)
    if change == "pm1":
        d = rng.choice([-1, 0, 0, 1], size=(h, w))
    elif change == "pm3":
        d = rng.choice([-3, -1, 0, 1, 3], size=(h, w))
    else:
        return xc, rng.integers(0, 256, (h, w), dtype=np.uint8)
    return xc, np.clip(xc.astype(np.int64) + d, 0, 255).astype(np.uint8)


def _agree(got, want):
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return abs(got - want) <= 1e-12 * abs(want) or abs(got - want) <= 1e-15


SIZES = [(512, 512), (130, 67), (3, 3), (2048, 1536)]


@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
@pytest.mark.parametrize("change", ["pm1", "pm3", "random"])
def test_kernel_matches_numpy_for_every_source(h, w, change):
    pairs = [_pair(h, w, change, seed) for seed in (1, 2)]
    xc = torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV)
    xs = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
    rng = np.random.default_rng(3)
    y01 = rng.random((2, h, w), dtype=np.float32)                                  # a network output in [0, 1]
    hat_in = (rng.random((2, h - 2, w - 2)) * 255).astype(np.float32)              # a host prediction in grey levels
    for name in ("KB", "AVG9"):
        k = filters.NAMED_FILTERS_2D[name]
        got = ops.pair_correlation(xc, xs, pixel_filter=k).cpu().numpy()
        for i, (c, s) in enumerate(pairs):
            want = corr_np.correlation(c, s, corr_np.filter_hat(s, k))
            assert _agree(got[i], want), (name, i, got[i], want)
    got = ops.pair_correlation(xc, xs, torch.from_numpy(y01).to(DEV), hat_full=True, hat_scale=255.).cpu().numpy()
    for i, (c, s) in enumerate(pairs):
        want = corr_np.correlation(c, s, (y01[i] * np.float32(255.))[1:-1, 1:-1])
        assert _agree(got[i], want), ("full", i, got[i], want)
    got = ops.pair_correlation(xc, xs, torch.from_numpy(hat_in).to(DEV), hat_full=False, hat_scale=1.).cpu().numpy()
    for i, (c, s) in enumerate(pairs):
        want = corr_np.correlation(c, s, hat_in[i])
        assert _agree(got[i], want), ("interior", i, got[i], want)
    if (h, w) == (3, 3):
        assert np.isnan(got).all()                                                # n = 1: cov = 0/0


def test_degenerate_cases_follow_numpy():
    rng = np.random.default_rng(7)
    h, w = 64, 80
    xc = rng.integers(0, 256, (h, w), dtype=np.uint8)
    d = np.where(xc > 127, -1, 1)
    xs = (xc.astype(np.int64) + d).astype(np.uint8)
    cases = {
        "no change": (xc, xc.copy(), rng.random((h - 2, w - 2)).astype(np.float32) * 255),
        "constant prediction": (xc, xs, np.full((h - 2, w - 2), 100.0, dtype=np.float32)),
        "constant prediction, negative": (xs, xc, np.full((h - 2, w - 2), 127.5, dtype=np.float32)),
        "|cor| > 1": (xc, xs, (128.0 + 0.5 * d[1:-1, 1:-1]).astype(np.float32)),
    }
    got_all = {}
    for name, (c, s, hat) in cases.items():
        t = lambda a: torch.from_numpy(a[None].copy()).to(DEV)        # noqa: E731
        got = float(ops.pair_correlation(t(c), t(s), t(hat), hat_full=False, hat_scale=1.).cpu()[0])
        want = corr_np.correlation(c, s, hat)
        assert _agree(got, want), (name, got, want)
        got_all[name] = got
    assert math.isnan(got_all["no change"])
    assert got_all["constant prediction"] == math.inf and got_all["constant prediction, negative"] == -math.inf
    assert got_all["|cor| > 1"] > 1 and math.isnan(correlation.p_value(got_all["|cor| > 1"], (h - 2) * (w - 2)))


def test_low_variance_prediction():
    """A flat cover with sparse changes and a prediction spread of ~1e-3 grey levels around 128: a raw-moment (one-pass) variance
    loses this to cancellation (sum xhat^2 ~ 4e9 against a centred sum of ~0.1)."""
    rng = np.random.default_rng(11)
    h = w = 512
    xc = np.full((h, w), 128, dtype=np.uint8)
    d = rng.choice([-1, 1], size=(h, w)) * (rng.random((h, w)) < 0.01)
    xs = (xc + d).astype(np.uint8)
    hat = (128.0 + 1e-3 * (rng.standard_normal((h - 2, w - 2)) + 0.3 * d[1:-1, 1:-1])).astype(np.float32)
    got, mom = ops.pair_correlation(torch.from_numpy(xc[None]).to(DEV), torch.from_numpy(xs[None]).to(DEV),
                                    torch.from_numpy(hat[None]).to(DEV), hat_full=False, hat_scale=1., moments=True)
    want = corr_np.correlation(xc, xs, hat)
    assert abs(float(got[0]) - want) <= 1e-9 * abs(want), (float(got[0]), want)
    m = mom[0].cpu().numpy()
    h64 = hat.astype(np.float64)
    assert abs(m[4] - np.sum((h64 - h64.mean()) ** 2)) <= 1e-9 * m[4]
    assert abs(m[0] - h64.mean()) <= 1e-13 * 128


def test_determinism_and_batch_independence():
    rng = np.random.default_rng(21)
    pairs = [_pair(96, 128, "pm1", 30 + i) for i in range(7)]
    xc = torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV)
    xs = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
    y = torch.from_numpy(rng.random((7, 96, 128), dtype=np.float32)).to(DEV)
    hi = torch.from_numpy((rng.random((7, 94, 126)) * 255).astype(np.float32)).to(DEV)
    sources = {"filter": lambda a, b, i: ops.pair_correlation(a, b, pixel_filter=filters.NAMED_FILTERS_2D["KB"], moments=True),
               "full": lambda a, b, i: ops.pair_correlation(a, b, y[i].contiguous(), moments=True),
               "interior": lambda a, b, i: ops.pair_correlation(a, b, hi[i].contiguous(), hat_full=False, hat_scale=1., moments=True)}
    for name, f in sources.items():
        full = [t.cpu() for t in f(xc, xs, slice(None))]
        again = [t.cpu() for t in f(xc, xs, slice(None))]
        assert all(torch.equal(a, b) for a, b in zip(full, again)), name
        alone = [t.cpu() for t in f(xc[3:4].contiguous(), xs[3:4].contiguous(), slice(3, 4))]
        for pos in range(7):                                           # pair 3 at every position of a batch of 7
            idx = list(range(7))
            idx[pos], idx[3] = 3, pos
            res = [t.cpu() for t in f(xc[idx].contiguous(), xs[idx].contiguous(), idx)]
            assert torch.equal(res[0][pos], alone[0][0]) and torch.equal(res[1][pos], alone[1][0]), (name, pos)
            assert torch.equal(res[0][pos], full[0][3]), (name, pos)


@pytest.mark.parametrize("mode,tol", [("f32", 1e-7), (None, 1e-5)])
def test_unet_source_against_cpu_oracle(tmp_path, mode, tol):
    xc_np, xs_np = _fixture_planes()
    model = gpu_model(2, "he", mode, drop_rate=0.)
    cor, p = correlation.correlation_u8_batch(torch.from_numpy(xc_np).to(DEV), torch.from_numpy(xs_np).to(DEV), model)
    ref_model = unet_ref.build_ref(2, formula.formula_state_dict(2, "he"))
    deltas = []
    for i in range(len(xc_np)):
        yref = evaluate_ref.infere_single(xs_np[i][..., None].astype(np.float32), ref_model)
        want = corr_np.correlation(xc_np[i], xs_np[i], yref[..., 0])
        deltas.append(abs(cor[i] - want))
        assert deltas[-1] <= tol, (mode, i, cor[i], want)
    print(f"\nUNet source, mode {mode or 'default'}: |delta cor| against the CPU oracle = {[f'{d:.3e}' for d in deltas]}")
    assert np.array_equal(p, correlation.p_value(cor, N_PIX))
    # through run(), both iterators, with the estimator object the CLI builds
    _dataset(tmp_path)
    for iterator in ("batched", "python"):
        res = correlation.run(tmp_path, stego_method="LSBR", alpha=1.0, predictor=UNetEstimator(model), iterator=iterator)
        np.testing.assert_allclose(res["correlation"].to_numpy(), cor, rtol=0, atol=tol)


def test_host_callable_predictor_equals_filter_source():
    xc_np, xs_np = _fixture_planes()
    kb = filters.NAMED_FILTERS_2D["KB"]
    xc, xs = torch.from_numpy(xc_np).to(DEV), torch.from_numpy(xs_np).to(DEV)
    calls = []

    def kb_numpy(x):
        assert x.shape == (512, 512, 1) and x.dtype == np.float32
        calls.append(1)
        return corr_np.filter_hat(x[..., 0], kb)[..., None]

    got, p_got = correlation.correlation_u8_batch(xc, xs, kb_numpy)
    want, p_want = correlation.correlation_u8_batch(xc, xs, filters.get_filter_estimator("KB", flatten=False))
    assert len(calls) == 5
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(p_got, p_want, rtol=1e-9, atol=0)
    with pytest.raises(ValueError, match="predictor returned"):
        correlation.correlation_u8_batch(xc, xs, lambda x: x)


def _cli(args, timeout=900):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-m", "ws_unet_amd.correlation", *args], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cli_writes_reference_layout(tmp_path):
    data = tmp_path / "data"
    _dataset(data)
    out, pp = tmp_path / "out" / "correlation.csv", tmp_path / "out" / "pairs.csv"
    _cli(["--data", str(data), "--out", str(out), "--per-pair-out", str(pp)])
    lines = out.read_text().splitlines()
    assert lines[0] == ",1,AVG9,AVG,KB" and lines[1].startswith("correlation,") and lines[2].startswith("p-value,") and len(lines) == 3
    t = pd.read_csv(out, index_col=0)
    for m in FILTERS:
        assert abs(t.loc["correlation", m] - _pub("correlation", m)) <= 2e-9
        assert _close_p(t.loc["p-value", m], _pub("p-value", m))
    rows = pd.read_csv(pp)
    assert list(rows.columns) == ["name_c", "name_s", "correlation", "p-value", "model_name"] and len(rows) == 20
    # a UNet column from a checkpoint in the reference's layout <model-dir>/<stego method>/<run>/
    run = tmp_path / "models" / "LSBR" / "run-x"
    (run / "model").mkdir(parents=True)
    (run / "config.json").write_text(json.dumps({"stego_method": "LSBR", "alpha": "1.0", "loss": "l1ws", "network": "unet_2",
                                                 "drop_rate": 0.0, "debug": False}))
    sd = formula.formula_state_dict(2, "he")
    torch.save({"epoch": 1, "state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, run / "model" / "best_model.pt.tar")
    out2 = tmp_path / "out" / "with_unet.csv"
    _cli(["--data", str(data), "--out", str(out2), "--filters", "KB", "--model-dir", str(tmp_path / "models"),
          "--unet-stego-methods", "LSBR", "--mode", "f32"])
    t2 = pd.read_csv(out2, index_col=0)
    assert out2.read_text().splitlines()[0] == ",KB,UNet_LSBR_l1ws"
    assert t2.loc["correlation", "KB"] == t.loc["correlation", "KB"]
    assert np.isfinite(t2.loc["correlation", "UNet_LSBR_l1ws"])


@pytest.mark.parametrize("iterator", ["python", "batched"])
def test_colour_image_and_missing_twin_raise(tmp_path, iterator):
    from PIL import Image
    _dataset(tmp_path / "a", stego_pairs=(6, 7, 9, 10))
    pred = filters.get_filter_estimator("AVG", flatten=False)
    with pytest.raises(ValueError, match=r"images/8\.png has no stego twin"):
        correlation.run(tmp_path / "a", stego_method="LSBR", alpha=1.0, predictor=pred, iterator=iterator)
    sdir = _dataset(tmp_path / "b")
    Image.open(GOLDEN / "stego_LSBR_1.0_9.png").convert("RGB").save(sdir / "9.png")
    with pytest.raises(ValueError, match=r"9\.png: a RGB image"):
        correlation.run(tmp_path / "b", stego_method="LSBR", alpha=1.0, predictor=pred, iterator=iterator)
