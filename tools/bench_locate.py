"""Time the payload-location kernels (ops.ws_residual_accumulate, K29; ops.embed_lsbr_keyed, K30) on one GPU and print one JSON line.

On --batch resident 512x512 planes (the five fixture covers tiled), in one process, each the median of --reps timings between HIP events
after warm-up, each timing --inner back-to-back calls -> ms per call, images/s and GB/s of the bytes the kernel has to move:
  * ops.ws_residual_accumulate against ops.ws_attack (K11: the same per-pixel terms, reduced per image instead of added per pixel) on the
    same inputs, ALTERNATING the two --rounds times (a clock ramp would hit both): in-kernel KB filter (1 B per pixel) and a full-frame
    x_hat (5 B per pixel), weighted; the ratio is that of the medians over the rounds;
  * K29 with one owner per pixel (parts 1) against its images dealt to 2, 4 and 8 workgroups per pixel tile with atomics, on these planes
    and on --small-batch planes of 64 x 64, where one thread per pixel cannot fill the chip;
  * ops.embed_lsbr_keyed at alpha 0.5 and 1 next to ops.embed_lsbr at alpha 1 (2 B per pixel);
  * with --unet: the whole pipeline per image with an untrained unet_2 (formula weights, the default inference mode): ResidualAccumulator.add
    on the batch, next to its two stages (unet_run.unet_plane, then K29 on the resident prediction).
The device results are checked against tests/locate_np.py on the first planes.
Usage: python tools/bench_locate.py [--batch 32] [--reps 30] [--inner 20] [--rounds 5] [--unet]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch

import locate_np
from ws_unet_amd import filters, ops
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--small-batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--unet", action="store_true")
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])
planes = covers[np.arange(a.batch) % 5].copy()
x = torch.from_numpy(planes).to("cuda")
y = (x.to(torch.float32) / 255.).contiguous()                     # a full-frame prediction in [0,1] (the image itself: any values do)
small = torch.from_numpy(np.ascontiguousarray(covers.reshape(5, 8, 64, 8, 64).transpose(0, 1, 3, 2, 4).reshape(320, 64, 64)[:a.small_batch])).to("cuda")
KB = np.asarray(filters.NAMED_FILTERS_2D["KB"])[..., 0]
AVG = np.asarray(filters.NAMED_FILTERS_2D["AVG"])[..., 0]
seeds = torch.arange(1, a.batch + 1, dtype=torch.int64, device="cuda")


def accumulators(t):
    return [torch.zeros((t.shape[1] - 2, t.shape[2] - 2), dtype=torch.int64, device="cuda") for _ in range(2)]


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


def rates(ms, bytes_per_pixel, t=None):
    t = x if t is None else t
    return {"ms": round(ms, 4), "images_per_s": round(t.shape[0] / ms * 1e3, 1), "GB_per_s": round(t.numel() * bytes_per_pixel / ms / 1e6, 2)}


def alternate(f, g):
    """medians over --rounds of f and g timed in turn -> (ms f, ms g, every round's pair)"""
    pairs = [(median_ms(f), median_ms(g)) for _ in range(a.rounds)]
    return float(np.median([p[0] for p in pairs])), float(np.median([p[1] for p in pairs])), [[round(v, 4) for v in p] for p in pairs]


num, den = accumulators(x)
out = {"batch": a.batch, "shape": [512, 512]}
for name, pred, bpp in (("kb", dict(pixel_filter=KB), 1), ("x_hat", dict(x_hat=y), 5)):
    acc_ms, att_ms, pairs = alternate(lambda: ops.ws_residual_accumulate(x, num, den, mean_filter=AVG, weighted=1, **pred),
                                      lambda: ops.ws_attack(x, pred.get("x_hat"), pixel_filter=pred.get("pixel_filter"), mean_filter=AVG, weighted=1))
    out[f"ws_residual_accumulate_{name}"] = rates(acc_ms, bpp)
    out[f"ws_attack_{name}"] = rates(att_ms, bpp)
    out[f"accumulate_over_attack_{name}"] = round(acc_ms / att_ms, 3)
    out[f"rounds_{name}"] = pairs
for parts in (1, 2, 4, 8):
    out[f"ws_residual_accumulate_kb_parts{parts}"] = rates(median_ms(
        lambda: ops.ws_residual_accumulate(x, num, den, pixel_filter=KB, mean_filter=AVG, weighted=1, parts=parts)), 1)
snum, sden = accumulators(small)
for parts in (1, 4, 16, 0):
    out[f"small_kb_parts{parts}"] = rates(median_ms(
        lambda: ops.ws_residual_accumulate(small, snum, sden, pixel_filter=KB, mean_filter=AVG, weighted=1, parts=parts)), 1, small)
t1 = torch.from_numpy(np.array([ops.lsbr_threshold(1.0)] * a.batch, dtype=np.uint32).view(np.int32)).to("cuda")
for alpha in (0.5, 1.0):
    thr = ops.lsbr_key_threshold(alpha)
    out[f"embed_lsbr_keyed_{alpha}"] = rates(median_ms(lambda: ops.embed_lsbr_keyed(x, seeds, 2008, thr)), 2)
out["embed_lsbr_1.0"] = rates(median_ms(lambda: ops.embed_lsbr(x, seeds, t1)), 2)

if a.unet:
    from ws_unet_amd import formula
    from ws_unet_amd.model import get_model
    from ws_unet_amd.unet_run import unet_plane
    from ws_unet_amd.ws import estimate, locate
    model = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode=None)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "he").items()})
    model = model.to("cuda")
    est = estimate.UNetEstimator(model)
    acc = locate.ResidualAccumulator(512, 512, "cuda")

    def whole():
        acc.images = 0                                                # (timing only: the sums wrap harmlessly)
        acc.add(x, est, weighted=1)
    plane = unet_plane(model, x)
    out["unet_pipeline"] = rates(median_ms(whole), 5)
    out["unet_plane_alone"] = rates(median_ms(lambda: unet_plane(model, x)), 5)
    out["accumulate_on_resident_plane"] = rates(median_ms(lambda: ops.ws_residual_accumulate(x, num, den, plane, mean_filter=AVG, weighted=1)), 5)
    out["unet_pipeline_ms_per_image"] = round(out["unet_pipeline"]["ms"] / a.batch, 5)

num, den = accumulators(x)
ops.ws_residual_accumulate(x[:5], num, den, pixel_filter=KB, mean_filter=AVG, weighted=1)
want = locate_np.accumulate(planes[:5], pixel_kernels=[KB] * 5, mean_kernel=AVG, weighted=1)
assert np.array_equal(num.cpu().numpy(), want[0]) and np.array_equal(den.cpu().numpy(), want[1]), "kernel and numpy accumulators differ"
twin = ops.embed_lsbr_keyed(x[:2], seeds[:2], 2008, ops.lsbr_key_threshold(0.5))[0].cpu().numpy()
for i in range(2):
    assert np.array_equal(twin[i], locate_np.lsbrk_np(planes[i], 0.5, i + 1, 2008)), "kernel and numpy LSBRK twins differ"
print(json.dumps(out))
