"""Time the two kernels behind the side-information planes (parity_oracle / demosaic_oracle) on one GPU and print one JSON line.

1. assembly  64 samples of 512x512 with 5 input planes (image, parity, R, G, B sites) and D4 ops, from 48 resident uint8 planes:
     kernel   ops.pair_batch_planes: one launch
     parent   what a user could do without it: ops.pair_batch, then torch ops -- the parity plane from the assembled image, the Bayer planes
              gathered from the eight transformed grids (built once, outside the timing) -- and a concatenation
   Both are asserted equal before anything is timed.  Median of --reps windows of --inner calls between two device events; bytes/s on the
   algorithmic traffic (every source plane read once, every output plane written once).
2. train     unet_2, batch 16 at 512x512, 5 planes, L1WS, one model and one batch: the fp32-storage fallback (train_planes_planar=False) and
   the planar path alternate --rounds times in one process; a window is --steps train steps between two device events, ended by a
   synchronise.  `planar_wins` is the rule of ws_unet_amd/train.py: the slowest planar window is faster than the fastest fallback window.
Usage: python tools/bench_side_planes.py [--size 512] [--batch 16] [--steps 20] [--rounds 3] [--skip-train]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from ws_unet_amd import ops
from ws_unet_amd.model import get_model
from ws_unet_amd.trainer import Trainer

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--skip-train", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda")
out = {"size": a.size}

# ---- 1. assembly ----------------------------------------------------------------------------------------------------------------------
ncov, pairs = 16, 32
n, hw = 2 * pairs, a.size * a.size
planes = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (3 * ncov, a.size, a.size), dtype=np.uint8)).to(dev)
idx_in = np.array([j for i in range(pairs) for j in (i % ncov, ncov + i)])
idx_cov = np.array([i % ncov for i in range(pairs) for _ in (0, 1)])
op = np.repeat(np.random.default_rng(1).integers(0, 8, pairs), 2).astype(np.uint8)
r, c = torch.meshgrid(torch.arange(a.size, device=dev), torch.arange(a.size, device=dev), indexing="ij")
grid = torch.stack([(r % 2 == 0) & (c % 2 == 0), (r + c) % 2 == 1, (r % 2 == 1) & (c % 2 == 1)]).float()


def d4(x, o):
    x = x.flip(-1) if o & 1 else x
    x = x.flip(-2) if o & 2 else x
    return x.transpose(-1, -2) if o & 4 else x


grids = torch.stack([d4(grid, o).contiguous() for o in range(8)])
op_dev = torch.from_numpy(op.astype(np.int64)).to(dev)


def parent():
    x, cov = ops.pair_batch(planes, idx_in, idx_cov, op)
    parity = (torch.round(x * 255).int() & 1).float()
    return torch.cat([x, parity, grids[op_dev]], dim=1), cov


def kernel():
    return ops.pair_batch_planes(planes, idx_in, idx_cov, op, parity=True, demosaic=True)


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
    return float(np.median(ms)), float(min(ms)), float(max(ms))


want, got = parent(), kernel()
assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "pair_batch_planes differs from pair_batch + torch side planes"
traffic = planes.shape[0] * hw + n * (5 + 1) * 4 * hw
out["assembly"] = {"samples": n, "planes": 5, "bytes": traffic}
for name, fn in (("kernel", kernel), ("parent", parent)):
    m, lo, hi = median_ms(fn)
    out["assembly"][name] = {"ms": round(m, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "GB_per_s": round(traffic / m / 1e6, 1)}
del want, got, grids

# ---- 2. train step --------------------------------------------------------------------------------------------------------------------
if not a.skip_train:
    torch.manual_seed(0)
    model = get_model("unet_2", in_channels=5, out_channels=1, channel=[0], drop_rate=0.0, mode=None).to(dev)
    tr = Trainer(model, loss="l1ws", lr=1e-5)
    u8 = planes[:a.batch]
    st = (u8 ^ (torch.rand(u8.shape, device=dev) < 0.2).to(torch.uint8))
    inputs = ops.side_planes(st, True, True)
    covers = ops.u8_to_unit(u8)[:, None].contiguous()
    alphas = torch.full((a.batch,), 0.4, device=dev)

    def window(planar, steps):
        model.train_planes_planar = planar
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            tr.train_step(inputs, covers, alphas)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    for planar in (False, True):
        window(planar, 3)                                                         # warm-up: packing, workspaces, the first range look
    ms = {"fallback": [], "planar": []}
    for _ in range(a.rounds):
        ms["fallback"].append(round(window(False, a.steps), 3))
        ms["planar"].append(round(window(True, a.steps), 3))
    out["train"] = {"network": "unet_2", "batch": a.batch, "planes": 5, "steps_per_window": a.steps, "train_mode": model.train_mode,
                    "step_ms": ms, "planar_wins": max(ms["planar"]) < min(ms["fallback"]), "skipped_steps": tr.skipped_steps()}
print(json.dumps(out))
