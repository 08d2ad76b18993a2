"""Time the predictor / stego-change correlation on one GPU and print one JSON line.

  * K15 (ops.pair_correlation) at 32 x 512^2 and 8 x 2048^2, with the filter taps evaluated in the kernel (KB) and with a full-frame
    x_hat (a network output), per call by HIP events (ops.KernelTimer) over --reps repetitions;
  * the batched UNet correlation on in-memory planes (unet_2, the default mode, batch 32 x 512^2): correlation_u8_batch (forward of
    the stego planes + K15 + p-values on the host) against unet_run.predict_u8_batch (forward + WS statistics) on the same planes,
    same process, alternating arms.
Usage: python tools/bench_correlation.py [--reps 50] [--rounds 6] [--steps 20]"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from ws_unet_amd import correlation, filters, formula, ops, unet_run
from ws_unet_amd.model import get_model

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--steps", type=int, default=20)
a = ap.parse_args()
out = {"k15_ms": {}}


def lsbr(x, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    flip = torch.randint(0, 2, x.shape, generator=g, dtype=torch.uint8)
    return (x.cpu() ^ flip).cuda()


kb = filters.NAMED_FILTERS_2D["KB"]
for n, hw in ((32, 512), (8, 2048)):
    xc = torch.from_numpy(formula.synthetic_images(n, hw, hw, seed=7)).cuda()
    xs = lsbr(xc, 1)
    hat = torch.rand((n, hw, hw), device="cuda")
    arms = {"filter_taps": lambda: ops.pair_correlation(xc, xs, pixel_filter=kb),
            "full_frame_x_hat": lambda: ops.pair_correlation(xc, xs, hat)}
    for name, f in arms.items():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t = ops.KernelTimer()
        ops.set_timer(t)
        for _ in range(a.reps):
            f()
        torch.cuda.synchronize()
        ops.set_timer(None)
        out["k15_ms"][f"{n}x{hw}^2 {name}"] = round(t.summary()["pair_correlation"]["total_ms"] / a.reps, 4)

m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None)
m.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "he").items()})
m = m.cuda()
xc = torch.from_numpy(formula.synthetic_images(32, 512, 512, seed=8)).cuda()
xs = lsbr(xc, 2)
arms = {"predict_u8_batch": lambda: unet_run.predict_u8_batch(xs, m)[0].cpu(),
        "correlation_u8_batch": lambda: correlation.correlation_u8_batch(xc, xs, m)}
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
            arms[k]()
        torch.cuda.synchronize()
        rates[k].append(32 * a.steps / (time.perf_counter() - t0))
out["unet_images_per_s"] = {k: round(float(np.median(v)), 1) for k, v in rates.items()}
out["unet_images_per_s_all"] = {k: [round(x, 1) for x in v] for k, v in rates.items()}
out["correlation_over_predict"] = round(out["unet_images_per_s"]["correlation_u8_batch"] / out["unet_images_per_s"]["predict_u8_batch"], 4)
out["mode"] = m.mode
print(json.dumps(out))
