"""Time the HILL-cost weighted prediction error on one GPU and print one JSON line.

  * the K12-K14 chain (hill_cost -> hill_threshold -> prediction_error with a full-frame x_hat) at 32 x 512^2 and 8 x 2048^2, per kernel
    and whole, by HIP events (ops.KernelTimer) over --reps repetitions;
  * the batched UNet evaluate on in-memory planes (unet_2, the default mode, batch 32 x 512^2): predict_u8_batch (WS statistics, no
    wMAE) against predict_u8_error_batch (mae + wmae), same process, alternating arms.
Usage: python tools/bench_prediction_error.py [--reps 50] [--rounds 6] [--steps 20]"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from ws_unet_amd import formula, ops, unet_run
from ws_unet_amd.model import get_model

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--steps", type=int, default=20)
a = ap.parse_args()
out = {"chain": {}}

for n, hw in ((32, 512), (8, 2048)):
    x = torch.from_numpy(formula.synthetic_images(n, hw, hw, seed=7)).cuda()
    hat = torch.rand((n, hw, hw), device="cuda")
    for _ in range(3):
        ops.prediction_error(x, hat)
    torch.cuda.synchronize()
    t = ops.KernelTimer()
    ops.set_timer(t)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.reps):
        ops.prediction_error(x, hat)
    e.record()
    torch.cuda.synchronize()
    ops.set_timer(None)
    per = {k: round(v["total_ms"] / a.reps, 4) for k, v in t.summary().items()}
    out["chain"][f"{n}x{hw}^2"] = {"ms_per_chain": round(s.elapsed_time(e) / a.reps, 4), "per_stage_ms": per}

m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None)
m.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "he").items()})
m = m.cuda()
x = torch.from_numpy(formula.synthetic_images(32, 512, 512, seed=8)).cuda()
arms = {"without_wmae": lambda: unet_run.predict_u8_batch(x, m), "with_wmae": lambda: unet_run.predict_u8_error_batch(x, m)}
for f in arms.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
rates = {k: [] for k in arms}
for r in range(a.rounds):
    for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            res = arms[k]()
        res[0].cpu()
        rates[k].append(32 * a.steps / (time.perf_counter() - t0))
out["evaluate_images_per_s"] = {k: round(float(np.median(v)), 1) for k, v in rates.items()}
out["evaluate_images_per_s_all"] = {k: [round(x, 1) for x in v] for k, v in rates.items()}
out["with_over_without"] = round(out["evaluate_images_per_s"]["with_wmae"] / out["evaluate_images_per_s"]["without_wmae"], 4)
out["mode"] = m.mode
print(json.dumps(out))
