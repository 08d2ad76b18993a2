"""Time the +-1 simulators (K37-K39) on one GPU, measure the detectors on their twins, print one JSON line.

  * (a) on --batch resident 512x512 cover planes (the five fixture covers tiled), ms per call between HIP events around --inner calls
    back to back, median of --reps such samples after warm-up: the float64 cost (K20), one K37 launch at 16 and at 1 multipliers,
    ops.ternary_lambda (nine K37 launches and the torch ops between them), K38 at the multipliers it found, K39, and embed_pm1.simulate
    'HILL' whole (cost + search + one read-back of the flags + draw);
  * the same in torch alone, checked against the kernels first: the entropy as elementwise float64 exp / log2 over (N,H,W) for one
    multiplier per image, a 40-step bisection of log2(lambda) over it, and the draw from a torch.rand plane (another generator: only
    the count of changes is compared);
  * (b) --auc: 64x64 crops of the fixture covers 6-8 (training) and 9-10 (held out), their LSBM, HILL and LSBR twins at --alpha: the
    held-out AUC of SPAM-686 + FLD trained on that method's twins, next to the AUC of the WS estimate (KB predictor, unweighted, no bias
    correction, as `ws.roc` collects its rows) of the same held-out crops and twins.  Five images decide nothing; the figures are
    recorded, not gated.
Usage: python tools/bench_pm1.py [--batch 32] [--reps 20] [--inner 5] [--alpha 0.4] [--auc]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from ws_unet_amd import embed, embed_pm1, filters, ops, spam
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--alpha", type=float, default=0.4)
ap.add_argument("--auc", action="store_true")
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
dev = torch.device("cuda")
planes = {k: np.ascontiguousarray(imread4_u8(gold / f"cover_{k}.png")[..., 3]) for k in (6, 7, 8, 9, 10)}
covers = np.stack([planes[k] for k in (6, 7, 8, 9, 10)])
x = torch.from_numpy(covers[np.arange(a.batch) % 5].copy()).to(dev)
n, h, w = x.shape
seeds = torch.tensor([embed.image_seed(f"{i}.png") for i in range(n)], dtype=torch.int64, device=dev)
LN2 = float(np.log(2.0))


def sample_ms(fn):
    """median, p10, p90 of the time of one call, from --reps samples of --inner calls back to back"""
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
    return [round(float(v), 4) for v in (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90))]


# ---- the torch composition ---------------------------------------------------------------------------------------------------------------
def torch_entropy(x_u8, rho, lam):
    """(N) entropies at one multiplier per image: the formulas of K37 as elementwise float64 ops"""
    e = torch.exp(-(lam[:, None, None] * rho))
    ep, em = torch.where(x_u8 == 255, 0.0, e), torch.where(x_u8 == 0, 0.0, e)
    z = (1.0 + ep) + em
    t = torch.where(e > 0, lam[:, None, None] * rho * e, 0.0)
    return (torch.log2(z) + (torch.where(x_u8 == 255, 0.0, t) + torch.where(x_u8 == 0, 0.0, t)) / (z * LN2)).sum(dim=(1, 2))


def torch_lambda(x_u8, rho, m, steps=40):
    """a bisection of log2(lambda) over [-50, 25], one multiplier per image and step; no host synchronisation either"""
    lo = torch.full((x_u8.shape[0],), -50.0, dtype=torch.float64, device=x_u8.device)
    hi = torch.full_like(lo, 25.0)
    for _ in range(steps):
        mid = (lo + hi) / 2
        ge = torch_entropy(x_u8, rho, torch.exp2(mid)) >= m
        lo, hi = torch.where(ge, mid, lo), torch.where(ge, hi, mid)
    return torch.exp2(lo)


def torch_draw(x_u8, rho, lam, gen):
    e = torch.exp(-(lam[:, None, None] * rho))
    ep, em = torch.where(x_u8 == 255, 0.0, e), torch.where(x_u8 == 0, 0.0, e)
    z = (1.0 + ep) + em
    u = torch.rand(x_u8.shape, dtype=torch.float64, device=x_u8.device, generator=gen)
    d = torch.where(u < ep / z, 1, torch.where(u < (ep + em) / z, -1, 0))
    return (x_u8.to(torch.int16) + d).to(torch.uint8)


def torch_lsbm(x_u8, alpha, gen):
    u = torch.rand(x_u8.shape, dtype=torch.float64, device=x_u8.device, generator=gen)
    tp = torch.where(x_u8 == 255, 0.0, torch.where(x_u8 == 0, alpha / 2, alpha / 4))
    tm = torch.where(x_u8 == 0, 0.0, torch.where(x_u8 == 255, alpha / 2, alpha / 4))
    return (x_u8.to(torch.int16) + torch.where(u < tp, 1, torch.where(u < tp + tm, -1, 0))).to(torch.uint8)


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------
rho = ops.hill_cost_f64(x)
m = torch.full((n,), a.alpha * h * w, dtype=torch.float64, device=dev)
lam, lam_hi, ok = ops.ternary_lambda(x, rho, m)
assert bool(ok.all())
ladder = torch.tensor(ops.TERNARY_LADDER, dtype=torch.float64, device=dev).expand(n, -1).contiguous()
lam16 = (lam[:, None] * torch.exp2(torch.linspace(-2, 2, 16, dtype=torch.float64, device=dev))).contiguous()
thr = torch.full((n,), ops.lsbm_threshold(a.alpha), dtype=torch.int32, device=dev)
gen = torch.Generator(device=dev)
gen.manual_seed(1)

# the composition computes what the kernels compute
h_k, h_t = ops.ternary_entropy(x, rho, lam[:, None].contiguous())[:, 0], torch_entropy(x, rho, lam)
lam_t = torch_lambda(x, rho, m)
ch_k, ch_t = ops.embed_ternary(x, rho, lam, seeds)[1].double(), (torch_draw(x, rho, lam, gen) != x).sum(dim=(1, 2)).double()
checks = {"entropy_max_rel_diff": float(((h_k - h_t).abs() / h_k).max()), "entropy_over_payload_minus_1_max": float((h_k / m - 1).abs().max()),
          "lambda_max_rel_diff_to_bisection": float(((lam - lam_t).abs() / lam).max()), "bracket_width_max": float((lam_hi / lam - 1).max()),
          "changes_per_pixel_k38": float(ch_k.mean() / (h * w)), "changes_per_pixel_torch": float(ch_t.mean() / (h * w)),
          "changes_per_pixel_k39": float(ops.embed_lsbm(x, seeds, thr)[1].double().mean() / (h * w))}
assert checks["entropy_max_rel_diff"] < 1e-9 and checks["lambda_max_rel_diff_to_bisection"] < 1e-6

stages = {
    "cost_f64_k20": lambda: ops.hill_cost_f64(x),
    "entropy_k37_l16": lambda: ops.ternary_entropy(x, rho, lam16),
    "entropy_k37_l16_ladder": lambda: ops.ternary_entropy(x, rho, ladder),
    "entropy_k37_l1": lambda: ops.ternary_entropy(x, rho, lam16[:, :1].contiguous()),
    "lambda_search_9_launches": lambda: ops.ternary_lambda(x, rho, m),
    "embed_ternary_k38": lambda: ops.embed_ternary(x, rho, lam, seeds),
    "embed_lsbm_k39": lambda: ops.embed_lsbm(x, seeds, thr),
    "simulate_hill": lambda: embed_pm1.simulate(x, "HILL", a.alpha, seeds),
    "simulate_lsbm": lambda: embed_pm1.simulate(x, "LSBM", a.alpha, seeds),
    "torch_entropy_l1": lambda: torch_entropy(x, rho, lam),
    "torch_lambda_bisection_40": lambda: torch_lambda(x, rho, m),
    "torch_draw": lambda: torch_draw(x, rho, lam, gen),
    "torch_lsbm": lambda: torch_lsbm(x, a.alpha, gen),
}
ms = {k: sample_ms(fn) for k, fn in stages.items()}
px = n * h * w
out = {"batch": n, "alpha": a.alpha, "ms_median_p10_p90": ms, "checks": checks,
       "ratio_torch_over_kernel": {"entropy_l1": round(ms["torch_entropy_l1"][0] / ms["entropy_k37_l1"][0], 1),
                                   "search": round(ms["torch_lambda_bisection_40"][0] / ms["lambda_search_9_launches"][0], 1),
                                   "draw_hill": round(ms["torch_draw"][0] / ms["embed_ternary_k38"][0], 1),
                                   "draw_lsbm": round(ms["torch_lsbm"][0] / ms["embed_lsbm_k39"][0], 1)},
       "gb_per_s": {"entropy_k37_l16": round(px * 9 / ms["entropy_k37_l16"][0] / 1e6, 1), "entropy_k37_l1": round(px * 9 / ms["entropy_k37_l1"][0] / 1e6, 1),
                    "embed_ternary_k38": round(px * 10 / ms["embed_ternary_k38"][0] / 1e6, 1), "embed_lsbm_k39": round(px * 2 / ms["embed_lsbm_k39"][0] / 1e6, 1)},
       "pixel_multipliers_per_ns_k37_l16": round(px * 16 / ms["entropy_k37_l16"][0] / 1e6, 2)}

# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------
if a.auc:
    def crops(ks):
        return np.stack([planes[k][r:r + 64, c:c + 64] for k in ks for r in range(0, 512, 64) for c in range(0, 512, 64)])

    def auc(neg, pos):
        neg, pos = np.asarray(neg, dtype=np.float64), np.asarray(pos, dtype=np.float64)
        return float(((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / (len(pos) * len(neg)))

    def twins(c, method, seed0):
        s = [seed0 + i for i in range(len(c))]
        sim = embed.simulate if method == "LSBR" else embed_pm1.simulate
        return sim(c, method, a.alpha, s)[0]

    feats = lambda t: spam.features(ops.spam_counts(t))
    kb = filters.NAMED_FILTERS_2D["KB"]
    ws = lambda t: ops.ws_attack(t, pixel_filter=kb, weighted=0).double().cpu().numpy()
    c_tr, c_te = torch.from_numpy(crops((6, 7, 8))).to(dev), torch.from_numpy(crops((9, 10))).to(dev)
    rows = {}
    for method in ("LSBR", "LSBM", "HILL"):
        s_tr, s_te = twins(c_tr, method, 1000), twins(c_te, method, 5000)
        model = spam.FLD(ridge=0.1).fit(feats(c_tr), feats(s_tr))
        rows[method] = {"spam_fld_auc": round(auc(model.output(feats(c_te)), model.output(feats(s_te))), 4),
                        "ws_kb_auc": round(auc(ws(c_te), ws(s_te)), 4),
                        "changes_per_pixel": round(float((s_te != c_te).double().mean()), 4),
                        "train_crops": len(c_tr), "held_out_crops": len(c_te)}
    out["auc_64x64_crops"] = rows
print(json.dumps(out))
