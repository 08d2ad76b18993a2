"""Time the JPEG-history kernels (ops.jpeg_energies, K31; ops.jpeg_predict, K32) on one GPU and print one JSON line.

  * K31 on --batch resident 512x512 planes (the five fixture covers precompressed at quality 75, tiled) against the 95 IJG tables of
    quality 1 .. 95 (three launches of 32 / 32 / 31 tables and the output's memset), and against one table (the transform's share);
  * K32 on the same planes, each with the table of quality 75: the prediction alone, and with the recompressed uint8 planes;
  * the whole predictor (ws.jpeg.JPEGEstimator.planes: K31, the rule, one read-back of the qualities, K32) by the wall clock;
  * for context, from the same process: the forward of an untrained unet_2 (formula weights, the default inference mode) on the same
    batch (unet_run.unet_plane), and the WS statistic on a resident prediction (K11).
  Each figure is the median of --reps timings between HIP events after warm-up, each over --inner back-to-back calls, with the 10th and
  90th percentile of those timings.  No gate: nothing
  earlier computes this.  The energies are checked against the numpy restatement (tests/jpeg_np.py) for one image.
Usage: python tools/bench_jpeg_history.py [--batch 32] [--reps 30] [--inner 5]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch

import jpeg_np
from ws_unet_amd import formula, ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.model import get_model
from ws_unet_amd.unet_run import unet_plane
from ws_unet_amd.ws import jpeg

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--inner", type=int, default=5)
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])
x = torch.from_numpy(covers[np.arange(a.batch) % 5].copy()).to("cuda")
x = ops.jpeg_recompress(x, 75)
tables95, table1 = ops.jpeg_tables(np.arange(1, 96)), ops.jpeg_tables([75])
tables75 = np.repeat(table1, a.batch, axis=0)


def sample_ms(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / a.inner)
    return np.asarray(ms)


def rates(samples):
    ms = float(np.median(samples))
    return {"ms": round(ms, 4), "p10": round(float(np.percentile(samples, 10)), 4), "p90": round(float(np.percentile(samples, 90)), 4),
            "ms_per_image": round(ms / a.batch, 5), "images_per_s": round(a.batch / ms * 1e3, 1)}


out = {"batch": a.batch, "shape": [512, 512]}
out["jpeg_energies_95_tables"] = rates(sample_ms(lambda: ops.jpeg_energies(x, tables95)))
out["jpeg_energies_1_table"] = rates(sample_ms(lambda: ops.jpeg_energies(x, table1)))
out["jpeg_predict"] = rates(sample_ms(lambda: ops.jpeg_predict(x, tables75)))
out["jpeg_predict_with_u8"] = rates(sample_ms(lambda: ops.jpeg_predict(x, tables75, want_u8=True)))
est = jpeg.JPEGEstimator()
est.planes(x)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(a.reps):
    est.planes(x)
torch.cuda.synchronize()
out["estimator_planes_wall"] = rates([(time.perf_counter() - t0) * 1e3 / a.reps])

model = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode=None)
model.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "he").items()})
model = model.to("cuda")
out["unet_2_forward"] = rates(sample_ms(lambda: unet_plane(model, x)))
hat = ops.jpeg_predict(x, tables75)
out["ws_attack_on_resident_plane"] = rates(sample_ms(lambda: ops.ws_attack(x, hat, hat_scale=1.0, weighted=0)))
out["energies_over_unet_forward"] = round(out["jpeg_energies_95_tables"]["ms"] / out["unet_2_forward"]["ms"], 3)

q = jpeg.estimate_quality(x[:5]).cpu().numpy()
assert np.array_equal(ops.jpeg_energies(x[:1], tables95).cpu().numpy(), jpeg_np.energies(x[:1].cpu().numpy(), tables95)), "kernel and numpy energies differ"
out["q_hat_of_the_five_covers_at_75"] = q.tolist()
print(json.dumps(out))
