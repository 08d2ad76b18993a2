"""Time the KB-stratified absolute-error box table on one GPU and print one JSON line.

  * error_boxes.run over a data set of the five fixture covers (512^2) listed over and over to --images rows (fabrika order, PNG
    decode on the native reader beside the GPU work), with the filters only (KB, AVG) and with one UNet added (unet_2, formula
    weights, the default inference mode): images/s, median of --rounds;
  * unet_run.predict_u8_batch on in-memory planes (batch 32 x 512^2), same process, same model: images/s;
  * K16-K18 per call by HIP events (ops.KernelTimer) inside one run of each leg.
Usage: python tools/bench_error_boxes.py [--images 2048] [--rounds 3] [--steps 20]"""
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

from ws_unet_amd import error_boxes, formula, ops, unet_run
from ws_unet_amd.model import get_model

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
a = ap.parse_args()
covers = (6, 7, 8, 9, 10)
out = {"images": a.images}

tmp = Path(tempfile.mkdtemp())
(tmp / "images").mkdir()
for k in covers:
    shutil.copy(ROOT / "tests" / "golden" / f"cover_{k}.png", tmp / "images" / f"{k}.png")
(tmp / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{covers[i % 5]}.png,512,512\n" for i in range(a.images)))

m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None)
m.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "he").items()})
m = m.cuda()
legs = {"filters": {"KB": "KB", "AVG": "AVG"}, "filters+unet": {"KB": "KB", "AVG": "AVG", "UNet": m}}
x = torch.from_numpy(formula.synthetic_images(32, 512, 512, seed=8)).cuda()

for name, preds in legs.items():                                # warm-up (decoder pools, allocator, first-forward checks)
    error_boxes.run(tmp, preds, split=None, take_num_images=64)
for _ in range(3):
    unet_run.predict_u8_batch(x, m)[0].cpu()
torch.cuda.synchronize()

rates = {k: [] for k in list(legs) + ["predict_u8_batch"]}
for r in range(a.rounds):
    for name, preds in legs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        error_boxes.run(tmp, preds, split=None)
        rates[name].append(a.images / (time.perf_counter() - t0))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        unet_run.predict_u8_batch(x, m)[0].cpu()
    torch.cuda.synchronize()
    rates["predict_u8_batch"].append(32 * a.steps / (time.perf_counter() - t0))
out["images_per_s"] = {k: round(float(np.median(v)), 1) for k, v in rates.items()}
out["images_per_s_all"] = {k: [round(v, 1) for v in vs] for k, vs in rates.items()}
out["unet_run_over_predict"] = round(out["images_per_s"]["filters+unet"] / out["images_per_s"]["predict_u8_batch"], 4)

out["kernel_ms"] = {}
for name, preds in legs.items():
    t = ops.KernelTimer()
    ops.set_timer(t)
    error_boxes.run(tmp, preds, split=None)
    torch.cuda.synchronize()
    ops.set_timer(None)
    s = t.summary()
    out["kernel_ms"][name] = {k: round(s[k]["total_ms"], 3) for k in ("ae_values", "ae_slices", "ae_select") if k in s}
out["mode"] = m.mode
shutil.rmtree(tmp, ignore_errors=True)
print(json.dumps(out))
