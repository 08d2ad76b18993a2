"""Time the moment kernel of the least-squares predictors (ops.ols_moments, K24) on one GPU and print one JSON line.

  * the kernel on --batch resident 512x512 planes (the five fixture covers tiled): median of --reps calls between HIP events after
    warm-up -> ms with the 10th and 90th percentile of the samples, images/s and GB/s of pixels read (1 byte per pixel);
  * numpy on the host for the same moments from the same uint8 planes: the float64 design matrix of every image and one BLAS
    `V.T @ V` each (exact: an image's sums stay below 2^53), images spread over --threads threads; checked equal to the kernel's.
Usage: python tools/bench_ols.py [--batch 32] [--reps 50] [--threads 16]"""
import argparse
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from ws_unet_amd import ops
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--threads", type=int, default=16)
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])
planes = covers[np.arange(a.batch) % 5].copy()
x = torch.from_numpy(planes).to("cuda")

for _ in range(5):
    got = ops.ols_moments(x)
torch.cuda.synchronize()
ms = []
for _ in range(a.reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ops.ols_moments(x)
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
p10, p90 = float(np.percentile(ms, 10)), float(np.percentile(ms, 90))
ms = float(np.median(ms))

_RING = ops._RING + ((1, 1),)


def host_moments(p):
    h, w = p.shape
    v = np.stack([p[r:r + h - 2, c:c + w - 2].reshape(-1) for r, c in _RING], axis=1).astype(np.float64)
    return (v.T @ v)[np.triu_indices(9)].astype(np.int64)


with ThreadPoolExecutor(max_workers=a.threads) as pool:
    list(pool.map(host_moments, planes[:a.threads]))                    # warm-up
    t0 = time.perf_counter()
    ref = np.stack(list(pool.map(host_moments, planes)))
    host_ms = (time.perf_counter() - t0) * 1e3
assert np.array_equal(ref, got.cpu().numpy()), "kernel and numpy moments differ"
print(json.dumps({"batch": a.batch, "shape": [512, 512], "kernel_ms": round(ms, 4), "p10": round(p10, 4), "p90": round(p90, 4), "images_per_s": round(a.batch / ms * 1e3, 1),
                  "pixel_GB_per_s": round(planes.size / ms / 1e6, 2), "numpy_ms": round(host_ms, 2), "numpy_threads": a.threads,
                  "numpy_images_per_s": round(a.batch / host_ms * 1e3, 1)}))
