"""Time the WS detection ROC driver and K19 on one GPU and print one JSON line.

  * (a) roc.collect_ws_scores with AVG + KB + one UNet (unet_2, formula weights, the default inference mode) over the cover set and
    the LSBR stego sets of --alphas, each the five fixture images listed over and over to --images rows (fabrika order, PNG decode on
    the native reader): images/s, median of --rounds;
  * (b) the same rows through three ws.estimate.run(batched=True) calls per set, one per predictor, as the reference's main does;
  * (c) ws.estimate.run(batched=True) with the UNet alone;
  * (d) K19 (ops.roc_counts, HIP events around the call) for G = 3 groups, t = 501, at N = 10^6 and 2^27 scores per group, uniform
    scores and all scores in bin 0: ms and read rate at 8 B + 1 B per score.
Usage: python tools/bench_roc.py [--images 2048] [--rounds 3] [--alphas .1 .05 .01]"""
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

from ws_unet_amd import formula, ops
from ws_unet_amd.ws import estimate, roc

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--alphas", nargs="+", type=float, default=[.1, .05, .01])
ap.add_argument("--skip-driver", action="store_true", help="time K19 only")
a = ap.parse_args()
imgs = (6, 7, 8, 9, 10)
gold = ROOT / "tests" / "golden"
out = {"images_per_set": a.images, "sets": 1 + len(a.alphas)}

tmp = Path(tempfile.mkdtemp())
(tmp / "images").mkdir()
for k in imgs:
    shutil.copy(gold / f"cover_{k}.png", tmp / "images" / f"{k}.png")
(tmp / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{imgs[i % 5]}.png,512,512\n" for i in range(a.images)))
for al in a.alphas:
    sdir = tmp / f"stego_LSBR_alpha_{al}_independent_images"
    sdir.mkdir()
    for k in imgs:
        shutil.copy(gold / f"stego_LSBR_{al}_{k}.png", sdir / f"{k}.png")
    (sdir / "files.csv").write_text("name,height,width,stego_method,alpha\n" + "".join(
        f"{sdir.name}/{imgs[i % 5]}.png,512,512,LSBR,{al}\n" for i in range(a.images)))
run_dir = tmp / "models" / "LSBR" / "run-a"
(run_dir / "model").mkdir(parents=True)
(run_dir / "config.json").write_text(json.dumps({"stego_method": "LSBR", "alpha": "0.400", "loss": "l1ws", "network": "unet_2",
                                                 "drop_rate": 0.0, "debug": False}))
torch.save({"epoch": 1, "state_dict": {k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "he").items()}},
           run_dir / "model" / "best_model.pt.tar")
model_path, model_name = tmp / "models" / "LSBR", "run-a"
sets = [(None, None)] + [("LSBR", al) for al in a.alphas]
n_images = a.images * len(sets)


def leg_a(take=None):
    kw = {"take_num_images": take} if take else {}
    return roc.collect_ws_scores(tmp, ["LSBR"], a.alphas, ("AVG", "KB"), unet=(model_path, model_name), **kw)


def leg_runs(names, take=None):
    kw = {"take_num_images": take} if take else {}
    return [estimate.run(tmp, sm, al, name, model_path, (3,), weighted=0, correct_bias=False, batched=True, **kw)
            for sm, al in sets for name in names]


legs = {"a_collect_avg_kb_unet": leg_a, "b_three_runs": lambda take=None: leg_runs(("AVG", "KB", model_name), take),
        "c_unet_run": lambda take=None: leg_runs((model_name,), take)}
if not a.skip_driver:
    for fn in legs.values():                                    # warm-up (decoder pools, pinned buffers, allocator, first-forward checks)
        fn(take=64)
    torch.cuda.synchronize()
    rates = {k: [] for k in legs}
    for r in range(a.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rates[name].append(n_images / (time.perf_counter() - t0))
    out["images_per_s"] = {k: round(float(np.median(v)), 1) for k, v in rates.items()}
    out["images_per_s_all"] = {k: [round(v, 1) for v in vs] for k, vs in rates.items()}
    ips = out["images_per_s"]
    out["a_over_b"] = round(ips["a_collect_avg_kb_unet"] / ips["b_three_runs"], 3)
    out["a_over_c"] = round(ips["a_collect_avg_kb_unet"] / ips["c_unet_run"], 3)

# (d) K19 alone
k19 = {}
taus = roc.TAUS
for n in (10 ** 6, 1 << 27):
    labels = torch.zeros(3 * n, dtype=torch.int8, device="cuda")
    labels[::2] = 1
    off = np.arange(4, dtype=np.int64) * n
    for dist in ("uniform", "bin0"):
        torch.manual_seed(0)
        s = torch.rand(3 * n, dtype=torch.float64, device="cuda") if dist == "uniform" else torch.zeros(3 * n, dtype=torch.float64, device="cuda")
        for _ in range(3):
            ops.roc_counts(s, labels, off, taus)
        torch.cuda.synchronize()
        ms = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.roc_counts(s, labels, off, taus)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        k19[f"n{n}_{dist}"] = {"ms": round(med, 4), "GB_per_s": round(3 * n * 9 / med / 1e6, 1)}
        del s
    del labels
for n in (10 ** 6, 1 << 27):
    k19[f"n{n}_bin0_over_uniform"] = round(k19[f"n{n}_bin0"]["ms"] / k19[f"n{n}_uniform"]["ms"], 3)
out["k19"] = k19
shutil.rmtree(tmp, ignore_errors=True)
print(json.dumps(out))
