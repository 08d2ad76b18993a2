"""Time the selection-channel-aware SRM kernels (ops.srm_weighted_counts, K52; ops.change_weights, K51) on one GPU and print one JSON line.

  * K52 beside K49 (ops.srm_counts) in the same process on 1, 32 and 256 (--batches) resident 512x512 planes: the five fixture covers
    tiled, with the change weights of srm.selection_channel(., 'HILL', 0.4) for them: median of --reps samples between HIP events after
    warm-up, each sample --inner back-to-back calls (the output's memset and the kernel) -> ms per call, images/s, k52_over_k49;
  * the same sums from a torch composition on the device (the residuals from shifted slices, the integer digit, torch.maximum over the
    four positions of the weight plane cut to the residual's centres, one weighted torch.bincount per table, 44 in all): checked equal
    first on the covers and the noise (the first 32 planes of a larger batch; float64 sums of integers below 2^53 are exact), timed on
    the covers the same way with fewer samples -> torch_over_k52.  At 256 planes it is ONE sample of one call without warm-up: a call
    takes 50 s there.  The constant plane is checked against its closed form instead, every table's total times the weight in
    bin 312: the composition's float64 atomics all meet in one bin per image there (K49's integer composition took 2.7 s a call at 256
    planes, profiles/r37);
  * K52 on a constant plane with constant weights (every run in a centre bin) against the covers -> constant_over_covers, which must not
    exceed 1 by more than the spread of the samples: THE GATE is 1.05; and on uniform noise with random weights (every run an LDS atomic);
  * K51 alone on the covers and their HILL costs at the multiplier of alpha 0.4;
  * srm.selection_channel whole (cost, the nine launches of the multiplier search and its read-back of one flag per image, K51) per cost;
  * --score-repeats R: `srm.score(..., selection_channel='HILL', sc_alpha=0.4)` end to end from PNG files over the five fixture covers and
    their LSBR 0.1 twins, R times after one warm-up pass, by the wall clock -> images/s, beside the same without a selection channel.
A line per stage goes to stderr as it ends.
Usage: python tools/bench_srm_weighted.py [--batches 1 32 256] [--reps 50] [--inner 10] [--score-repeats 10]"""
import argparse
import json
import shutil
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch

import srm_np
import srm_weighted_np
from ws_unet_amd import costs, ops, srm
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batches", nargs="+", type=int, default=[1, 32, 256])
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--score-repeats", type=int, default=0)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_srm_weighted.py measures on a GPU"
H = W = 512
TABLES = len(ops.SRM_TABLES)
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])


def torch_sums(x, wt):
    """(N,44,625) int64: shifted slices, the integer digit, torch.maximum over a run's four weights, one weighted bincount per table"""
    n, h, w = x.shape
    xi, wf = x.to(torch.int32), wt.to(torch.float64)
    base = (torch.arange(n, device=x.device, dtype=torch.int64) * ops.SRM_BINS)[:, None, None]
    out, residuals = [], {}
    for cls, q2, res, scan in srm_np.TABLES:
        if (cls, res) not in residuals:
            taps = srm_np.CLASSES[cls][1][res]
            up, left = -min(dr for dr, _ in taps), -min(dc for _, dc in taps)
            hh, ww = h - up - max(dr for dr, _ in taps), w - left - max(dc for _, dc in taps)
            R = torch.zeros((n, hh, ww), dtype=torch.int32, device=x.device)
            for (dr, dc), c in taps.items():
                R += c * xi[:, up + dr:up + dr + hh, left + dc:left + dc + ww]
            residuals[cls, res] = (R.abs() * 4, R.sign(), wf[:, up:up + hh, left:left + ww])
        mag4, sign, wc = residuals[cls, res]
        d = sign * torch.clamp((mag4 + q2) // (2 * q2), max=2) + 2
        hh, ww = d.shape[1:]
        cut = (lambda t, k: t[:, :, k:ww - 3 + k]) if scan == "h" else (lambda t, k: t[:, k:hh - 3 + k, :])
        idx = ((cut(d, 0) * 5 + cut(d, 1)) * 5 + cut(d, 2)) * 5 + cut(d, 3)
        wmax = torch.maximum(torch.maximum(cut(wc, 0), cut(wc, 1)), torch.maximum(cut(wc, 2), cut(wc, 3)))
        out.append(torch.bincount((idx.to(torch.int64) + base).flatten(), weights=wmax.flatten(), minlength=n * ops.SRM_BINS)
                   .view(n, ops.SRM_BINS).to(torch.int64))
    return torch.stack(out, dim=1)


def samples_ms(fn, inner, reps, warm=2):
    """the ms per call of `reps` samples of `inner` back-to-back calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return np.asarray(ms)


def stats(ms, batch):
    med = float(np.median(ms))
    return {"ms": round(med, 5), "p10": round(float(np.percentile(ms, 10)), 5), "p90": round(float(np.percentile(ms, 90)), 5),
            "images_per_s": round(batch / med * 1e3, 1)}


T0 = time.perf_counter()


def stage(text):
    print(f"[{time.perf_counter() - T0:7.1f} s] {text}", file=sys.stderr, flush=True)


def u16(arr):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint16)).cuda()


res = {"shape": [H, W], "reps": a.reps, "inner": a.inner, "batches": {}}
for batch in a.batches:
    x = torch.from_numpy(covers[np.arange(batch) % 5].copy()).cuda()
    rho = costs.cost_map(x, "HILL")
    lam = ops.ternary_lambda(x, rho, torch.full((batch,), 0.4 * H * W, dtype=torch.float64, device="cuda"))[0]
    wt = ops.change_weights(x, rho, lam)
    assert torch.equal(wt, srm.selection_channel(x, "HILL", 0.4))
    rng = np.random.default_rng(1)
    inputs = {"covers": (x, wt),
              "constant": (torch.full((batch, H, W), 77, dtype=torch.uint8, device="cuda"), u16(np.full((batch, H, W), 20000))),
              "noise": (torch.from_numpy(rng.integers(0, 256, (batch, H, W), dtype=np.uint8)).cuda(), u16(rng.integers(0, 65536, (batch, H, W))))}
    out = torch.empty((batch, TABLES, ops.SRM_BINS), dtype=torch.int64, device="cuda")
    inner = a.inner if batch < 256 else max(1, a.inner // 5)
    row = {}
    for name, (xx, ww) in inputs.items():
        got = ops.srm_weighted_counts(xx, ww)
        if name == "constant":
            want = torch.zeros_like(got)
            want[:, :, 312] = 20000 * torch.tensor([(H - t[4]) * (W - t[5]) for t in ops.SRM_TABLES], dtype=torch.int64, device="cuda")
            assert torch.equal(got, want), f"batch {batch} constant: K52 and the closed form differ"
        else:
            assert torch.equal(got[:32], torch_sums(xx[:32], ww[:32])), f"batch {batch} {name}: K52 and the torch composition differ"
        assert np.array_equal(got[:1].cpu().numpy(), srm_weighted_np.sums(xx[:1].cpu().numpy(), ww[:1].cpu().numpy())), f"batch {batch} {name}: K52 and numpy differ"
        r = {"k52": stats(samples_ms(lambda: ops.srm_weighted_counts(xx, ww, out=out), inner, a.reps), batch),
             "k49": stats(samples_ms(lambda: ops.srm_counts(xx, out=out), inner, a.reps), batch)}
        r["k52_over_k49"] = round(r["k52"]["ms"] / r["k49"]["ms"], 3)
        if name == "covers":
            r["torch"] = stats(samples_ms(lambda: torch_sums(xx, ww), 1, *((max(3, a.reps // 10), 2) if batch < 256 else (1, 0))), batch)
            r["torch_over_k52"] = round(r["torch"]["ms"] / r["k52"]["ms"], 1)
        row[name] = r
        stage(f"batch {batch} {name}: {r}")
        del got
    row["constant_over_covers"] = round(row["constant"]["k52"]["ms"] / row["covers"]["k52"]["ms"], 3)
    row["k51"] = stats(samples_ms(lambda: ops.change_weights(x, rho, lam), inner, a.reps), batch)
    row["selection_channel"] = {c: stats(samples_ms(lambda: srm.selection_channel(x, c, 0.4), 1, max(3, a.reps // 10)), batch) for c in costs.COSTS}
    stage(f"batch {batch}: K51 {row['k51']}, selection_channel {row['selection_channel']}")
    res["batches"][str(batch)] = row
    del inputs, x, rho, wt, out
    torch.cuda.empty_cache()

if a.score_repeats:
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        (root / "images").mkdir()
        sdir = root / "stego_LSBR_alpha_0.1"
        sdir.mkdir()
        ks = (6, 7, 8, 9, 10)
        for k in ks:
            shutil.copy(gold / f"cover_{k}.png", root / "images" / f"{k}.png")
            shutil.copy(gold / f"stego_LSBR_0.1_{k}.png", sdir / f"{k}.png")
        (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in ks))
        (sdir / "files.csv").write_text("name,height,width,stego_method,alpha\n" + "".join(f"stego_LSBR_alpha_0.1/{k}.png,512,512,LSBR,0.1\n" for k in ks))
        for key, sc in (("score_from_png_selection_channel_HILL", dict(selection_channel="HILL", sc_alpha=0.4)), ("score_from_png_plain", {})):
            model = srm.fit(root, ["LSBR"], [0.1], **sc)
            srm.score(root, model, ["LSBR"], [0.1], **sc)                     # warm-up
            times = []
            for _ in range(a.score_repeats):
                t0 = time.perf_counter()
                df = srm.score(root, model, ["LSBR"], [0.1], **sc)
                df.to_csv(root / "srm.csv", index=False)
                times.append(time.perf_counter() - t0)
            med = float(np.median(times))
            stage(f"{key}: {med:.5f} s per pass")
            res[key] = {"images": 10, "repeats": a.score_repeats, "s_per_pass": round(med, 5), "p10": round(float(np.percentile(times, 10)), 5),
                        "p90": round(float(np.percentile(times, 90)), 5), "images_per_s": round(10 / med, 1)}
worst = max(row["constant_over_covers"] for row in res["batches"].values())
res["gate_constant_not_slower_than_covers"] = worst <= 1.05
print(json.dumps(res))
assert worst <= 1.05, f"K52 on a constant plane takes {worst} of its time on the covers"
