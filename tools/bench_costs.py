"""Time the wavelet cost kernel (K48, ops.wavelet_cost_f64) and the embedders over it (ws_unet_amd.costs) on one GPU, and measure the coding
loss of the two-layer code under the two costs; print one JSON line.  Not gated, not part of bench.py.

  * (a) K48 on resident 512x512 cover planes (the five fixture covers tiled), 1 / --batch / --big of them, both kinds, with K20
    (ops.hill_cost_f64) beside it: ms per call between HIP events, median (p10, p90) of --reps samples after warm-up; from the median
    the achieved bytes/s (9 bytes of HBM per pixel: one read, one float64 written) and float64 operations/s (645 per pixel as the kernel
    executes them, halo and the whole runs of four included: per 32x32 tile 2 x 63 x 48 + 3 x 48 x 48 + 3 x 48 x 32 + 3 x 32 x 32 filter
    outputs of 16 multiplications and 16 additions; the divisions are not counted).
  * (b) the whole of costs.simulate and of costs.embed (h = 10) at --alpha, the cost included.
  * (c) the coding loss on the five fixture covers at alpha 0.4 / 0.2 / 0.1, h = 10: D(STCT) = costs.embed's distortion against D* = the
    expectation sum rho (p+ + p-) of the ternary payload-limited sender at the same payload, D / D* - 1 (tools/bench_stc_ml.py's table,
    for the two new costs).
Usage: python tools/bench_costs.py [--batch 32] [--big 256] [--reps 7] [--alpha 0.4]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from ws_unet_amd import costs, embed, ops
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--big", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--alpha", type=float, default=0.4)
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
dev = torch.device("cuda")
covers = np.stack([np.ascontiguousarray(imread4_u8(gold / f"cover_{k}.png")[..., 3]) for k in (6, 7, 8, 9, 10)])
n = a.batch
x = torch.from_numpy(covers[np.arange(max(n, a.big)) % 5].copy()).to(dev)
nmax, hh, ww = x.shape
hw = hh * ww
seed_list = [embed.image_seed(f"{i}.png") for i in range(nmax)]
FLOP_PER_PIXEL = (2 * 63 * 48 + 3 * 48 * 48 + 3 * 48 * 32 + 3 * 32 * 32) * 32 / 1024.0


def sample_ms(fn):
    """median, p10, p90 of the time of one call, from --reps samples"""
    for _ in range(2):
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
    return [round(float(v), 4) for v in (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90))]


# ---- (a), (b) -------------------------------------------------------------------------------------------------------------------------------
timing = {}
for nb in sorted({1, n, nmax}):
    xs = x[:nb]
    row = {"hill_cost_f64_k20_ms": sample_ms(lambda: ops.hill_cost_f64(xs))}
    for kind in ("suniward", "wow"):
        t = sample_ms(lambda: ops.wavelet_cost_f64(xs, kind))
        row[f"{kind}_k48_ms"] = t
        row[f"{kind}_k48_GB_per_s"] = round(9.0 * nb * hw / (t[0] * 1e-3) / 1e9, 2)
        row[f"{kind}_k48_f64_Gop_per_s"] = round(FLOP_PER_PIXEL * nb * hw / (t[0] * 1e-3) / 1e9, 1)
        row[f"{kind}_simulate_whole_ms"] = sample_ms(lambda: costs.simulate(xs, kind, a.alpha, seed_list[:nb]))
        row[f"{kind}t_embed_whole_h10_ms"] = sample_ms(lambda: costs.embed(xs, kind + "t", a.alpha, h=10, seeds=seed_list[:nb]))
    timing[f"batch{nb}"] = row

# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------
x5 = torch.from_numpy(covers).to(dev)
seeds5 = [embed.image_seed(f"{c}.png") for c in (6, 7, 8, 9, 10)]
loss = {}
for name in ("SUNIWARD", "WOW"):
    rho5 = costs.cost_map(x5, name)
    rho5_np = rho5.cpu().numpy()
    table = {"cost_min_median_max": [float(f"{v:.4g}") for v in (rho5_np.min(), np.median(rho5_np), rho5_np.max())],
             "clamped_pixels": int((rho5_np == ops.WAVELET_COST_CLAMPS[name.lower()]).sum())}
    for alpha in (0.4, 0.2, 0.1):
        kb = int(round(alpha * hw))
        lam = ops.ternary_lambda(x5, rho5, torch.full((5,), float(kb), dtype=torch.float64, device=dev))[0].cpu().numpy()
        dstar = []
        for i in range(5):                                                   # the sender's expectation in float64 on the host
            e = np.exp(-lam[i] * rho5_np[i])
            ep, em = np.where(covers[i] == 255, 0.0, e), np.where(covers[i] == 0, 0.0, e)
            p = (ep + em) / ((1.0 + ep) + em)
            dstar.append(float((np.where(p > 0, rho5_np[i], 0.0) * p).sum()))
        _, ch, d, ok, layers = costs.embed(x5, name + "T", alpha, rho=rho5, h=10, seeds=seeds5)
        assert bool(ok.all())
        r = d.cpu().numpy() / np.array(dstar)
        table[f"alpha_{alpha}"] = {"bits": kb, "ternary_sender_cost": [round(v, 3) for v in dstar],
                                   "stct_distortion": [round(float(v), 3) for v in d.tolist()],
                                   "loss_per_image": [round(float(v - 1), 4) for v in r], "loss_mean": round(float(r.mean() - 1), 4),
                                   "changes_per_pixel": round(float(ch.double().mean()) / hw, 5), "bits_high": layers[:, 0].tolist()}
    loss[name] = table
print(json.dumps({"batch": n, "big": nmax, "alpha": a.alpha, "flop_per_pixel": FLOP_PER_PIXEL, "ms_median_p10_p90": timing,
                  "coding_loss_h10_5_covers": loss}))
