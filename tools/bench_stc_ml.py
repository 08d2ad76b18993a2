"""Time the two-layer syndrome-trellis embedder (K43-K47, ws_unet_amd.stc_ml) on one GPU, and measure its coding loss; print one JSON line.

  * (a) on resident 512x512 cover planes (the five fixture covers tiled), 1 / --batch / --big of them, at --alpha and constraint heights 7
    and 10 along the keyed path: ms per call between HIP events, median (p10, p90) of --reps samples after warm-up, of every stage of
    stc_ml.embed (the multiplier search, K45, K43 over the high layer, K46, K43 over the low layer, K47), of stc_ml.embed whole (given
    costs; with the keyed path and its read-backs), of stc_ml.extract, and of stc.embed whole (the uniform entry point, as
    tools/bench_stc.py times it) for the comparison with the commit before the ragged kernels.
  * (b) the coding loss on the five fixture covers at alpha 0.4 / 0.2 / 0.1 over the HILL cost: D(STCT) = stc_ml.embed's distortion against
    D* = the expectation sum rho (p+ + p-) of the ternary payload-limited sender at the same payload (ops.ternary_lambda), D / D* - 1; and
    beside it D(STCM) = stc.embed(change='pm1')'s cost with the same k and rho against the same D*.  Nothing is gated on these figures.
Usage: python tools/bench_stc_ml.py [--batch 32] [--big 256] [--reps 7] [--alpha 0.4] [--heights 7 10] [--only-uniform]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from ws_unet_amd import embed, ops, stc
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--big", type=int, default=256, help="a second batch size: one workgroup per compute unit (0: skip)")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--alpha", type=float, default=0.4)
ap.add_argument("--heights", type=int, nargs="+", default=[7, 10])
ap.add_argument("--only-uniform", action="store_true", help="time stc.embed whole alone (this also runs on a tree without stc_ml)")
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
dev = torch.device("cuda")
covers = np.stack([np.ascontiguousarray(imread4_u8(gold / f"cover_{k}.png")[..., 3]) for k in (6, 7, 8, 9, 10)])
n = a.batch
x = torch.from_numpy(covers[np.arange(max(n, a.big)) % 5].copy()).to(dev)
nmax, hh, ww = x.shape
hw = hh * ww
seed_list = [embed.image_seed(f"{i}.png") for i in range(nmax)]
seeds = torch.tensor(seed_list, dtype=torch.int64, device=dev)


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


rho = ops.hill_cost_f64(x)
k = int(round(a.alpha * hw))
msg = stc.random_message(seed_list, k, dev)
timing = {}
for h in a.heights:
    for nb in sorted({1, n, nmax}):
        cap = nb * ops.stc_workspace_bytes(hw, h)
        timing[f"h{h}_batch{nb}"] = {"stc_embed_uniform_whole_ms": sample_ms(
            lambda: stc.embed(x[:nb], msg[:nb], seeds=seed_list[:nb], h=h, change="pm1", workspace_cap=cap))}
if a.only_uniform:
    print(json.dumps({"batch": n, "alpha": a.alpha, "tree": str(ROOT.name), "ms_median_p10_p90": timing}))
    sys.exit(0)

from ws_unet_amd import stc_ml

# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------
path = stc.key_path(seeds, hh, ww, dev)
bits = torch.full((nmax,), float(k), dtype=torch.float64, device=dev)
for h in a.heights:
    for nb in sorted({1, n, nmax}):
        xs, rs, ms_, ss, ps = x[:nb], rho[:nb], msg[:nb], seeds[:nb], path[:nb]
        cap = nb * ops.stc_workspace_bytes(hw, h)
        lam = ops.ternary_lambda(xs, rs, bits[:nb])[0]
        u1, rho1, ent = ops.stc_layer_high(xs, rs, lam)
        k1 = torch.clamp(torch.floor(ent), 0, k - 1).to(torch.int32)
        k0 = k - k1
        cols = stc_ml._columns_for(h, hw, torch.cat([k1, k0]), 0, dev)
        y1, _, _, ok1 = ops.stc_embed_ragged(u1, rho1, ms_, cols, ss, ks=k1, h=h, path=ps, workspace_cap=cap)
        u0, rho0 = ops.stc_layer_low(xs, rs, lam, y1, k1)
        y0, _, _, ok0 = ops.stc_embed_ragged(u0, rho0, ms_, cols, ss, ks=k0, first=k1, h=h, path=ps, workspace_cap=cap)
        stego, changes, dist, ok = ops.stc_layer_compose(xs, rs, y1, y0, k1, ok1, ok0)
        assert bool(ok.all())
        whole = stc_ml.embed(xs, ms_, rho=rs, h=h, seeds=seed_list[:nb], workspace_cap=cap)
        assert torch.equal(whole[0], stego) and torch.equal(stc_ml.extract(stego, whole[4], seeds=seed_list[:nb], h=h)[0], ms_)
        row = timing[f"h{h}_batch{nb}"]
        row.update({
            "lambda_search_ms": sample_ms(lambda: ops.ternary_lambda(xs, rs, bits[:nb])),
            "layer_high_k45_ms": sample_ms(lambda: ops.stc_layer_high(xs, rs, lam)),
            "ragged_embed_high_k43_ms": sample_ms(lambda: ops.stc_embed_ragged(u1, rho1, ms_, cols, ss, ks=k1, h=h, path=ps, workspace_cap=cap)),
            "layer_low_k46_ms": sample_ms(lambda: ops.stc_layer_low(xs, rs, lam, y1, k1)),
            "ragged_embed_low_k43_ms": sample_ms(lambda: ops.stc_embed_ragged(u0, rho0, ms_, cols, ss, ks=k0, first=k1, h=h, path=ps, workspace_cap=cap)),
            "compose_k47_ms": sample_ms(lambda: ops.stc_layer_compose(xs, rs, y1, y0, k1, ok1, ok0)),
            "stc_ml_embed_whole_ms": sample_ms(lambda: stc_ml.embed(xs, ms_, rho=rs, h=h, seeds=seed_list[:nb], workspace_cap=cap)),
            "stc_ml_extract_ms": sample_ms(lambda: stc_ml.extract(stego, whole[4], seeds=seed_list[:nb], h=h)),
            "k1_min_max": [int(k1.min()), int(k1.max())], "changes_per_pixel": round(float(changes.double().mean()) / hw, 5)})
        row["stc_ml_embed_whole_ms_per_image"] = round(row["stc_ml_embed_whole_ms"][0] / nb, 4)

# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------
x5 = torch.from_numpy(covers).to(dev)
rho5 = ops.hill_cost_f64(x5)
rho5_np, x5_np = rho5.cpu().numpy(), covers
seeds5 = [embed.image_seed(f"{c}.png") for c in (6, 7, 8, 9, 10)]
loss = {}
for alpha in (0.4, 0.2, 0.1):
    kb = int(round(alpha * hw))
    lam = ops.ternary_lambda(x5, rho5, torch.full((5,), float(kb), dtype=torch.float64, device=dev))[0].cpu().numpy()
    dstar, pstar = [], []
    for i in range(5):                                                       # the sender's expectation in float64 on the host
        e = np.exp(-lam[i] * rho5_np[i])
        ep, em = np.where(x5_np[i] == 255, 0.0, e), np.where(x5_np[i] == 0, 0.0, e)
        p = (ep + em) / ((1.0 + ep) + em)
        dstar.append(float((np.where(p > 0, rho5_np[i], 0.0) * p).sum()))
        pstar.append(float(p.sum()))
    row = {"bits": kb, "ternary_sender_cost": [round(v, 3) for v in dstar], "ternary_sender_changes_per_pixel": round(float(np.mean(pstar)) / hw, 5)}
    for h in a.heights:
        _, ch_t, d_t, ok_t, layers = stc_ml.embed(x5, alpha, rho=rho5, h=h, seeds=seeds5)
        _, ch_m, d_m, ok_m = stc.embed(x5, alpha, rho=rho5, h=h, seeds=seeds5, change="pm1")
        assert bool(ok_t.all()) and bool(ok_m.all())
        rt, rm = d_t.cpu().numpy() / np.array(dstar), d_m.cpu().numpy() / np.array(dstar)
        row[f"h{h}"] = {"stct_distortion": [round(float(v), 3) for v in d_t.tolist()], "stcm_cost": [round(float(v), 3) for v in d_m.tolist()],
                        "stct_loss_per_image": [round(float(v - 1), 4) for v in rt], "stct_loss_mean": round(float(rt.mean() - 1), 4),
                        "stcm_loss_per_image": [round(float(v - 1), 4) for v in rm], "stcm_loss_mean": round(float(rm.mean() - 1), 4),
                        "stct_changes_per_pixel": round(float(ch_t.double().mean()) / hw, 5),
                        "stcm_changes_per_pixel": round(float(ch_m.double().mean()) / hw, 5), "bits_high": layers[:, 0].tolist()}
    loss[f"alpha_{alpha}"] = row
print(json.dumps({"batch": n, "alpha": a.alpha, "ms_median_p10_p90": timing, "coding_loss_hill_cost_5_covers": loss}))
