"""Time the stego simulators on one GPU and print one JSON line.

  * (a) embed.simulate 'LSBR' and 'HILLR' at alpha 0.4 on --batch resident 512x512 cover planes (the five fixture covers tiled):
    images/s, median of --reps calls between HIP events; for HILLR also the three stages on their own (float64 cost K20, the six
    select passes K21, the threshold embed K22);
  * (b) data.pairs.PairLoader steps/s over the five-cover set, batch 4 (two pairs, two steps per epoch), --epochs epochs after one warm-up
    epoch: simulate=False (the file route: two decodes per pair, the twins written first by embed.write_dataset) against
    simulate=True (one decode per pair, the twin made on the device), for both methods.
Usage: python tools/bench_embed.py [--batch 32] [--reps 20] [--epochs 50]"""
import argparse
import json
import shutil
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from ws_unet_amd import embed, ops
from ws_unet_amd.data.pairs import PairLoader
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--epochs", type=int, default=50)
a = ap.parse_args()
imgs = (6, 7, 8, 9, 10)
gold = ROOT / "tests" / "golden"
dev = torch.device("cuda")
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in imgs])
x = torch.from_numpy(covers[np.arange(a.batch) % 5].copy()).to(dev)
seeds = [embed.image_seed(f"{i}.png") for i in range(a.batch)]


def median_ms(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


key = ops.hill_cost_f64(x)
rank = torch.full((a.batch,), embed.hillr_rank(0.4, 512, 512), dtype=torch.int64, device=dev)
bits = ops.rank_select_f64(key, rank)
stages = {"lsbr": lambda: embed.simulate(x, "LSBR", 0.4, seeds), "hillr": lambda: embed.simulate(x, "HILLR", 0.4),
          "hillr_cost_f64": lambda: ops.hill_cost_f64(x), "hillr_rank_select": lambda: ops.rank_select_f64(key, rank),
          "hillr_embed_threshold": lambda: ops.embed_threshold(x, key, bits)}
ms = {k: median_ms(fn) for k, fn in stages.items()}
out = {"batch": a.batch, "ms": {k: round(v, 4) for k, v in ms.items()},
       "images_per_s": {k: round(a.batch / ms[k] * 1e3, 1) for k in ("lsbr", "hillr")}}

# (b) the pair loader over the five covers: files against simulation
tmp = Path(tempfile.mkdtemp())
(tmp / "images").mkdir()
for k in imgs:
    shutil.copy(gold / f"cover_{k}.png", tmp / "images" / f"{k}.png")
(tmp / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in imgs))
steps = {}
for method in ("LSBR", "HILLR"):                                # the two methods PairLoader simulates
    embed.write_dataset(tmp, method, 0.4)
    for sim in (False, True):
        loader = PairLoader(tmp, None, method, 0.4, batch_size=4, device=dev, seed=1, simulate=sim)
        for _ in loader:                                        # warm-up epoch (pinned buffers, decoder pool)
            pass
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        for _ in range(a.epochs):
            loader.reshuffle()
            for inputs, _ in loader:
                n += 1
        torch.cuda.synchronize()
        steps[f"{method}_{'simulate' if sim else 'files'}"] = round(n / (time.perf_counter() - t0), 1)
out["pair_loader_steps_per_s"] = steps
shutil.rmtree(tmp, ignore_errors=True)
print(json.dumps(out))
