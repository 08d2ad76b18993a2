"""Time the sequential-payload kernels (ops.ws_sequential, K27; ops.embed_lsbr_seq, K28) on one GPU and print one JSON line.

On --batch resident 512x512 planes (the five fixture covers tiled), in one process, each the median of --reps timings between HIP events
after warm-up, each timing --inner back-to-back calls -> ms per call, images/s and GB/s of the bytes the kernel has to move:
  * ops.ws_sequential with the in-kernel KB filter (1 B per pixel) and with a full-frame x_hat (5 B per pixel), weighted, with and
    without the curve;
  * ops.ws_attack on the same inputs: the yardstick, the same per-pixel terms under a plain sum;
  * ops.embed_lsbr_seq at alpha 0.4 and 1 next to ops.embed_lsbr at the same alphas (2 B per pixel).
The device results are checked against tests/sequential_np.py on the first planes.
Usage: python tools/bench_sequential.py [--batch 32] [--reps 50] [--inner 20]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch

import sequential_np
from ws_unet_amd import embed, filters, ops
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--inner", type=int, default=20)
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])
planes = covers[np.arange(a.batch) % 5].copy()
x = torch.from_numpy(planes).to("cuda")
y = (x.to(torch.float32) / 255.).contiguous()                     # a full-frame prediction in [0,1] (the image itself: any values do)
KB = np.asarray(filters.NAMED_FILTERS_2D["KB"])[..., 0]
AVG = np.asarray(filters.NAMED_FILTERS_2D["AVG"])[..., 0]
seeds = torch.arange(1, a.batch + 1, dtype=torch.int64, device="cuda")


def median_ms(fn):
    for _ in range(5):
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
    return float(np.median(ms))


def rates(ms, bytes_per_pixel):
    return {"ms": round(ms, 4), "images_per_s": round(a.batch / ms * 1e3, 1), "GB_per_s": round(planes.size * bytes_per_pixel / ms / 1e6, 2)}


def thresholds(alpha):
    return torch.from_numpy(np.array([ops.lsbr_threshold(alpha)] * a.batch, dtype=np.uint32).view(np.int32)).to("cuda")


def counts(alpha):
    return torch.full((a.batch,), embed.lsbrs_count(alpha, 512, 512), dtype=torch.int64, device="cuda")


out = {"batch": a.batch, "shape": [512, 512]}
out["ws_sequential_kb"] = rates(median_ms(lambda: ops.ws_sequential(x, pixel_filter=KB, mean_filter=AVG, weighted=1)), 1)
out["ws_sequential_kb_curve"] = rates(median_ms(lambda: ops.ws_sequential(x, pixel_filter=KB, mean_filter=AVG, weighted=1, return_curve=True)), 1)
out["ws_sequential_kb_rows_up"] = rates(median_ms(lambda: ops.ws_sequential(x, pixel_filter=KB, mean_filter=AVG, weighted=1, order="rows_up")), 1)
out["ws_attack_kb"] = rates(median_ms(lambda: ops.ws_attack(x, None, pixel_filter=KB, mean_filter=AVG, weighted=1)), 1)
out["ws_sequential_x_hat"] = rates(median_ms(lambda: ops.ws_sequential(x, y, mean_filter=AVG, weighted=1)), 5)
out["ws_attack_x_hat"] = rates(median_ms(lambda: ops.ws_attack(x, y, mean_filter=AVG, weighted=1)), 5)
out["ws_sequential_kb_again"] = rates(median_ms(lambda: ops.ws_sequential(x, pixel_filter=KB, mean_filter=AVG, weighted=1)), 1)
out["sequential_over_attack_kb"] = round(out["ws_sequential_kb"]["ms"] / out["ws_attack_kb"]["ms"], 3)
out["sequential_over_attack_x_hat"] = round(out["ws_sequential_x_hat"]["ms"] / out["ws_attack_x_hat"]["ms"], 3)
for alpha in (0.4, 1.0):
    t, c = thresholds(alpha), counts(alpha)
    out[f"embed_lsbr_seq_{alpha}"] = rates(median_ms(lambda: ops.embed_lsbr_seq(x, seeds, c, "rows")), 2)
    out[f"embed_lsbr_seq_rows_up_{alpha}"] = rates(median_ms(lambda: ops.embed_lsbr_seq(x, seeds, c, "rows_up")), 2)
    out[f"embed_lsbr_{alpha}"] = rates(median_ms(lambda: ops.embed_lsbr(x, seeds, t)), 2)

k, t_max, t_all, curve = (v.cpu().numpy() for v in ops.ws_sequential(x, pixel_filter=KB, mean_filter=AVG, weighted=1, return_curve=True))
for i in range(min(a.batch, 5)):
    want = sequential_np.ws_sequential_np(planes[i], "rows", pixel_kernel=KB, mean_kernel=AVG, weighted=1)
    assert (k[i], t_max[i], t_all[i]) == want[:3] and np.array_equal(curve[i], want[3]), "kernel and numpy changepoints differ"
twin = ops.embed_lsbr_seq(x[:2], seeds[:2], counts(0.4)[:2], "rows_up")[0].cpu().numpy()
for i in range(2):
    assert np.array_equal(twin[i], sequential_np.lsbrs_np(planes[i], 0.4, i + 1, "rows_up")), "kernel and numpy LSBRS twins differ"
print(json.dumps(out))
