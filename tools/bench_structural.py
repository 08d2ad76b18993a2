"""Time the count kernels of the structural estimators (ops.spa_tables, K25; ops.rs_counts, K26) on one GPU and print one JSON line.

  * each kernel on --batch resident 512x512 planes (the five fixture covers tiled): median of --reps calls between HIP events after
    warm-up, each timing --inner back-to-back calls (the output's memset and the kernel; one call is tens of microseconds, the size
    of an event's own resolution) -> ms per call with the 10th and 90th percentile of the samples, images/s and GB/s of pixels read
    (1 byte per pixel);
  * the moment kernel of the least-squares predictors (ops.ols_moments, K24) in the same process: a yardstick with the same input bytes;
  * K25 on a constant plane of the same size, where every pair falls into one bin, and its time over the covers' (the contention factor);
  * the numpy restatement of both tables (tests/structural_np.py) for the same planes, images spread over --threads threads; checked
    equal to the kernels' tables.
Usage: python tools/bench_structural.py [--batch 32] [--reps 50] [--inner 20] [--threads 16]"""
import argparse
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch

import structural_np
from ws_unet_amd import ops
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--threads", type=int, default=16)
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])
planes = covers[np.arange(a.batch) % 5].copy()
x = torch.from_numpy(planes).to("cuda")
flat = torch.full_like(x, 77)


def sample_ms(fn, t):
    for _ in range(5):
        fn(t)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn(t)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / a.inner)
    return np.asarray(ms)


def rates(samples):
    ms = float(np.median(samples))
    return {"kernel_ms": round(ms, 4), "p10": round(float(np.percentile(samples, 10)), 4), "p90": round(float(np.percentile(samples, 90)), 4),
            "images_per_s": round(a.batch / ms * 1e3, 1), "pixel_GB_per_s": round(planes.size / ms / 1e6, 2)}


spa_s, rs_s, ols_s = sample_ms(ops.spa_tables, x), sample_ms(ops.rs_counts, x), sample_ms(ops.ols_moments, x)
flat_s = sample_ms(ops.spa_tables, flat)
spa_s2 = sample_ms(ops.spa_tables, x)                                    # the covers again, after the constant plane: the same clocks
spa_ms, rs_ms, ols_ms, flat_ms, spa_ms2 = (float(np.median(s)) for s in (spa_s, rs_s, ols_s, flat_s, spa_s2))
tables, counts = ops.spa_tables(x).cpu().numpy(), ops.rs_counts(x).cpu().numpy()
assert ops.spa_tables(flat)[:, 0, 0].eq(2 * 512 * 511).all(), "constant plane: not every pair in E[0]"


def host(p):
    return structural_np.spa_table(p), structural_np.rs_counts(p)


with ThreadPoolExecutor(max_workers=a.threads) as pool:
    list(pool.map(host, planes[:a.threads]))                            # warm-up
    t0 = time.perf_counter()
    ref = list(pool.map(host, planes))
    host_ms = (time.perf_counter() - t0) * 1e3
assert np.array_equal(np.stack([r[0] for r in ref]), tables), "kernel and numpy sample-pairs tables differ"
assert np.array_equal(np.stack([r[1] for r in ref]), counts), "kernel and numpy RS counts differ"
print(json.dumps({"batch": a.batch, "shape": [512, 512], "spa_tables": rates(spa_s), "rs_counts": rates(rs_s), "ols_moments": rates(ols_s),
                  "spa_over_ols": round(spa_ms / ols_ms, 3), "rs_over_ols": round(rs_ms / ols_ms, 3),
                  "spa_tables_constant_plane": rates(flat_s), "spa_tables_covers_again": rates(spa_s2), "spa_tables_covers_again_ms": round(spa_ms2, 4),
                  "constant_over_covers": round(flat_ms / spa_ms2, 3),
                  "numpy_ms": round(host_ms, 2), "numpy_threads": a.threads, "numpy_images_per_s": round(a.batch / host_ms * 1e3, 1)}))
