"""Time the kernels of the 5x5 least-squares predictors (ops.ols_moments5, K56; ops.predict5x5, K57) on one GPU; one JSON line per batch.

  * each kernel on --batches resident 512x512 planes (the five fixture covers tiled): median of --reps calls between HIP events after
    warm-up -> ms with the 10th and 90th percentile;
  * beside K56: K24 (ops.ols_moments, 45 sums) on the same planes, and a torch restatement in the same process -- per image `unfold`
    to the float64 (25, P) design matrix and one matmul (exact: an image's sums stay below 2^53), checked equal to the kernel's;
  * beside K57: a torch float32 `conv2d` of x / 255 with the 5x5 taps, times 255 (another sum order: compared to 1e-3 of a pixel unit on
    the pixels with a full window, not bit for bit), with and without the bias plane on the kernel's side;
  * --stat: ws.estimate._stat whole (moments -> host fit -> planes -> statistic) for 'OLSa5x5' beside 'OLSa' at --stat-batch planes,
    weighted 1, bias correction on, a host clock around a device synchronise;
  * --table: the mean absolute error of the change-rate estimate of KB, OLSa, OLSa2, OLSa5x5, OLSa5x5s on the five golden LSBR files at
    alpha 0.01 / 0.05 / 0.1 / 1.0, weighted 1, with and without bias correction (FIVE images: it shows that the predictors work, not how
    well).
Usage: python tools/bench_ols5.py [--batches 1 32 256] [--reps 30] [--stat] [--table]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from ws_unet_amd import filters, ols, ols5, ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import estimate

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="*", default=[1, 32, 256])
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--stat", action="store_true")
ap.add_argument("--stat-batch", type=int, default=32)
ap.add_argument("--table", action="store_true")
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
COVERS = (6, 7, 8, 9, 10)
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in COVERS])
AVG = filters.NAMED_FILTERS_2D["AVG"]


def events(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms": round(float(np.median(ms)), 4), "p10": round(float(np.percentile(ms, 10)), 4), "p90": round(float(np.percentile(ms, 90)), 4)}


_SKIP = [i for i in range(25) if i != 12] + [12]
_IU = torch.triu_indices(25, 25)


def torch_moments(x):
    out = []
    for p in x:
        v = torch.nn.functional.unfold(p[None, None].to(torch.float64), 5)[0][_SKIP]          # (25, P), neighbours then the centre
        out.append((v @ v.T)[_IU[0], _IU[1]].to(torch.int64))
    return torch.stack(out)


def torch_predict(x, taps):
    k = torch.zeros(25, dtype=torch.float32, device=x.device)
    k[[i for i in range(25) if i != 12]] = taps
    return torch.nn.functional.conv2d(x[:, None].to(torch.float32) / 255., k.reshape(1, 1, 5, 5))[:, 0] * 255.


taps = torch.from_numpy(ols5.fit(ops.ols_moments5(torch.from_numpy(covers).cuda()).sum(dim=0).cpu().numpy())[0].astype(np.float32)).cuda()
for batch in a.batches:
    x = torch.from_numpy(covers[np.arange(batch) % 5].copy()).cuda()
    row = {"batch": batch, "shape": [512, 512], "reps": a.reps}
    row["K56_ols_moments5"] = events(lambda: ops.ols_moments5(x), a.reps)
    row["K24_ols_moments"] = events(lambda: ops.ols_moments(x), a.reps)
    row["torch_unfold_matmul_f64"] = events(lambda: torch_moments(x), max(3, a.reps // 10))
    assert torch.equal(torch_moments(x), ops.ols_moments5(x)), "kernel and torch moments differ"
    row["K57_predict5x5"] = events(lambda: ops.predict5x5(x, taps), a.reps)
    row["K57_predict5x5_with_bias"] = events(lambda: ops.predict5x5(x, taps, want_bias=True), a.reps)
    row["torch_conv2d_f32"] = events(lambda: torch_predict(x, taps), a.reps)
    diff = (torch_predict(x, taps) - ops.predict5x5(x, taps)[:, 2:-2, 2:-2]).abs().max().item()
    assert diff < 1e-3, diff
    row["conv2d_max_abs_diff"] = diff
    row["K56_images_per_s"] = round(batch / row["K56_ols_moments5"]["ms"] * 1e3, 1)
    row["K56_int_madds_per_s"] = round(batch * 508 * 508 * 325 / row["K56_ols_moments5"]["ms"] * 1e3, 0)
    row["K57_output_GB_per_s"] = round(batch * 512 * 512 * 4 / row["K57_predict5x5"]["ms"] / 1e6, 2)
    print(json.dumps(row), flush=True)

if a.stat:
    x = torch.from_numpy(covers[np.arange(a.stat_batch) % 5].copy()).cuda()
    row = {"stat_batch": a.stat_batch, "weighted": 1, "correct_bias": True}
    for name, make in (("OLSa5x5", lambda: ols5.estimator("OLSa5x5")), ("OLSa", lambda: ols.adaptive_estimator("OLSa"))):
        for _ in range(3):
            estimate._stat(x, make(), AVG, 1, True)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            estimate._stat(x, make(), AVG, 1, True)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        row[name] = {"ms": round(float(np.median(ms)), 3), "p10": round(float(np.percentile(ms, 10)), 3), "p90": round(float(np.percentile(ms, 90)), 3)}
    print(json.dumps(row), flush=True)

if a.table:
    makers = {"KB": lambda: filters.get_filter_estimator(filter_name="KB", flatten=False), "OLSa": lambda: ols.adaptive_estimator("OLSa"),
              "OLSa2": lambda: ols.adaptive_estimator("OLSa2"), "OLSa5x5": lambda: ols5.estimator("OLSa5x5"),
              "OLSa5x5s": lambda: ols5.estimator("OLSa5x5s")}
    for alpha in ("0.01", "0.05", "0.1", "1.0"):
        x = torch.from_numpy(np.stack([imread4_u8(gold / f"stego_LSBR_{alpha}_{k}.png")[..., 3] for k in COVERS])).cuda()
        for correct_bias in (False, True):
            row = {"alpha": float(alpha), "true_change_rate": float(alpha) / 2, "images": len(COVERS), "weighted": 1, "correct_bias": correct_bias}
            for name, make in makers.items():
                beta = estimate._stat(x, make(), AVG, 1, correct_bias).cpu().numpy().astype(np.float64)
                row[name] = round(float(np.abs(beta - float(alpha) / 2).mean()), 5)
            print(json.dumps(row), flush=True)
