"""Time the stages of the cost-ordered WS estimator (placement='adaptive', K33) on one GPU and print one JSON line.

On --batch resident 512x512 planes (the five fixture covers tiled), in one process, each the median of --reps timings between HIP events
after warm-up, each timing --inner back-to-back calls -> ms per call:
  * cost: ops.hill_cost (K12), the float32 key of the image under attack;
  * sort: ops.interior_order on that key, torch.sort(stable=True) on the device plus the int32 copy;
  * terms: ops.ws_ordered_terms, kernel A of K33, with the in-kernel KB filter and with a full-frame x_hat, weighted;
  * fold: ops.ws_ordered_fold, kernels B and C of K33, along the cost order and along the identity path (no gather misses);
  * ws_ordered: A, B and C in one call;   adaptive_total: cost + sort + ws_ordered as ws.estimate runs them;
  * ws_sequential (K27) on the same batch: the yardstick, the same terms reduced in raster order without a term plane.
No threshold is asserted.  The device results are checked against tests/adaptive_np.py on the first planes.
Usage: python tools/bench_adaptive.py [--batch 32] [--reps 30] [--inner 10]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch

import adaptive_np
from ws_unet_amd import filters, ops
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--inner", type=int, default=10)
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])
planes = covers[np.arange(a.batch) % 5].copy()
x = torch.from_numpy(planes).to("cuda")
y = (x.to(torch.float32) / 255.).contiguous()                     # a full-frame prediction in [0,1] (the image itself: any values do)
KB = np.asarray(filters.NAMED_FILTERS_2D["KB"])[..., 0]
AVG = np.asarray(filters.NAMED_FILTERS_2D["AVG"])[..., 0]
H, W = planes.shape[1:]
M = (H - 2) * (W - 2)


def median_ms(fn):
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
    return round(float(np.median(ms)), 4)


cost = ops.hill_cost(x)
path = ops.interior_order(cost)
ident = torch.arange(M, dtype=torch.int32, device="cuda").repeat(a.batch, 1).contiguous()
terms = ops.ws_ordered_terms(x, pixel_filter=KB, mean_filter=AVG, weighted=1)


def adaptive_total():
    return ops.ws_ordered(x, ops.interior_order(ops.hill_cost(x)), pixel_filter=KB, mean_filter=AVG, weighted=1)


out = {"batch": a.batch, "shape": [H, W]}
out["cost_ms"] = median_ms(lambda: ops.hill_cost(x))
out["sort_ms"] = median_ms(lambda: ops.interior_order(cost))
out["terms_kb_ms"] = median_ms(lambda: ops.ws_ordered_terms(x, pixel_filter=KB, mean_filter=AVG, weighted=1))
out["terms_x_hat_ms"] = median_ms(lambda: ops.ws_ordered_terms(x, y, mean_filter=AVG, weighted=1))
out["fold_cost_order_ms"] = median_ms(lambda: ops.ws_ordered_fold(terms, path, H, W))
out["fold_identity_ms"] = median_ms(lambda: ops.ws_ordered_fold(terms, ident, H, W))
out["ws_ordered_kb_ms"] = median_ms(lambda: ops.ws_ordered(x, path, pixel_filter=KB, mean_filter=AVG, weighted=1))
out["adaptive_total_kb_ms"] = median_ms(adaptive_total)
out["ws_sequential_kb_ms"] = median_ms(lambda: ops.ws_sequential(x, pixel_filter=KB, mean_filter=AVG, weighted=1))
out["ws_sequential_x_hat_ms"] = median_ms(lambda: ops.ws_sequential(x, y, mean_filter=AVG, weighted=1))
out["ws_ordered_over_sequential_kb"] = round(out["ws_ordered_kb_ms"] / out["ws_sequential_kb_ms"], 2)
out["adaptive_total_over_sequential_kb"] = round(out["adaptive_total_kb_ms"] / out["ws_sequential_kb_ms"], 2)
out["images_per_s_adaptive_total"] = round(a.batch / out["adaptive_total_kb_ms"] * 1e3, 1)

k, t_max, t_all = (v.cpu().numpy() for v in adaptive_total())
keys, order = cost.cpu().numpy(), path.cpu().numpy()
for i in range(min(a.batch, 2)):
    assert np.array_equal(order[i], adaptive_np.interior_order_np(keys[i])), "device and numpy orders differ"
    want = adaptive_np.ws_ordered_np(planes[i], order[i], 1.0, pixel_kernel=KB, mean_kernel=AVG, weighted=1)
    assert (k[i], t_max[i], t_all[i]) == want, "kernel and numpy changepoints differ"
print(json.dumps(out))
