"""Time the SRM count kernel (ops.srm_counts, K49) on one GPU and print one JSON line.

  * K49 on 1, 32 and 256 (--batches) resident 512x512 planes of three kinds -- the five fixture covers tiled, a constant plane, uniform
    noise: median of --reps samples between HIP events after warm-up, each sample --inner back-to-back calls (the output's memset and the
    kernel) -> ms per call, images/s, bin updates per second (44 per pixel);
  * the same counts from a torch composition on the device in the same process (the residuals from shifted slices, the digit in integers,
    the bin index, one torch.bincount per table over the whole batch): what a user could do without K49; checked equal first, timed the
    same way with fewer samples.  THE GATE: K49 must be faster than this composition on all three kinds of plane at every batch, or the
    script fails;
  * K36 (ops.spam_counts, order 2, T 3: 4 bin updates per pixel) on the same inputs, as the yardstick for bin updates per second; the
    ratio and constant_over_covers are reported, not gated;
  * --score-repeats R: `srm.score` end to end from PNG files (decode, upload, K49, features, the discriminant) over the five fixture covers
    and their LSBR 0.1 twins, R times after one warm-up pass, by the wall clock -> images/s.
Usage: python tools/bench_srm.py [--batches 1 32 256] [--reps 50] [--inner 10] [--score-repeats 10]"""
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
from ws_unet_amd import ops, srm
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batches", nargs="+", type=int, default=[1, 32, 256])
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--score-repeats", type=int, default=0)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_srm.py measures on a GPU"
H = W = 512
UPDATES = len(ops.SRM_TABLES)                                                # bin updates per pixel (less the borders)
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])


def torch_counts(x):
    """(N,44,625) int64: shifted slices, the integer digit, one bincount per table"""
    n, h, w = x.shape
    xi = x.to(torch.int32)
    base = (torch.arange(n, device=x.device, dtype=torch.int64) * ops.SRM_BINS)[:, None, None]
    out, residuals = [], {}
    for cls, q2, res, scan in srm_np.TABLES:
        if (cls, res) not in residuals:
            taps = srm_np.CLASSES[cls][1][res]
            up, left = -min(dr for dr, _ in taps), -min(dc for _, dc in taps)
            hh, ww = h - up - max(dr for dr, _ in taps), w - left - max(dc for _, dc in taps)
            R = torch.zeros((n, hh, ww), dtype=torch.int32, device=x.device)
            for (dr, dc), wt in taps.items():
                R += wt * xi[:, up + dr:up + dr + hh, left + dc:left + dc + ww]
            residuals[cls, res] = (R.abs() * 4, R.sign())
        mag4, sign = residuals[cls, res]
        d = sign * torch.clamp((mag4 + q2) // (2 * q2), max=2) + 2
        hh, ww = d.shape[1:]
        runs = [d[:, :, k:ww - 3 + k] for k in range(4)] if scan == "h" else [d[:, k:hh - 3 + k, :] for k in range(4)]
        idx = ((runs[0] * 5 + runs[1]) * 5 + runs[2]) * 5 + runs[3]
        out.append(torch.bincount((idx.to(torch.int64) + base).flatten(), minlength=n * ops.SRM_BINS).view(n, ops.SRM_BINS))
    return torch.stack(out, dim=1)


def samples_ms(fn, inner, reps):
    """the ms per call of `reps` samples of `inner` back-to-back calls"""
    for _ in range(2):
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


def stats(ms, batch, updates):
    med = float(np.median(ms))
    return {"ms": round(med, 5), "p10": round(float(np.percentile(ms, 10)), 5), "p90": round(float(np.percentile(ms, 90)), 5),
            "images_per_s": round(batch / med * 1e3, 1), "G_updates_per_s": round(batch * H * W * updates / med / 1e6, 2)}


res = {"shape": [H, W], "reps": a.reps, "inner": a.inner, "batches": {}}
gate = []
for batch in a.batches:
    inputs = {"covers": torch.from_numpy(covers[np.arange(batch) % 5].copy()).cuda(),
              "constant": torch.full((batch, H, W), 77, dtype=torch.uint8, device="cuda"),
              "noise": torch.from_numpy(np.random.default_rng(1).integers(0, 256, (batch, H, W), dtype=np.uint8)).cuda()}
    row = {}
    for name, x in inputs.items():
        out = torch.empty((batch, UPDATES, ops.SRM_BINS), dtype=torch.int64, device="cuda")
        out36 = torch.empty((batch, 4, 343), dtype=torch.int64, device="cuda")
        got = ops.srm_counts(x)
        assert torch.equal(got, torch_counts(x)), f"batch {batch} {name}: K49 and the torch composition differ"
        k = min(batch, 2)
        assert np.array_equal(got[:k].cpu().numpy(), srm_np.counts(x[:k].cpu().numpy())), f"batch {batch} {name}: K49 and numpy differ"
        inner = a.inner if batch < 256 else max(1, a.inner // 5)
        k49 = samples_ms(lambda: ops.srm_counts(x, out=out), inner, a.reps)
        k36 = samples_ms(lambda: ops.spam_counts(x, 2, 3, out=out36), inner, a.reps)
        tc = samples_ms(lambda: torch_counts(x), 1, max(3, a.reps // 10))
        r = {"k49": stats(k49, batch, UPDATES), "k36": stats(k36, batch, 4), "torch_bincount": stats(tc, batch, UPDATES)}
        r["torch_over_k49"] = round(r["torch_bincount"]["ms"] / r["k49"]["ms"], 1)
        r["k49_over_k36_ms"] = round(r["k49"]["ms"] / r["k36"]["ms"], 2)
        r["k49_over_k36_updates_per_s"] = round(r["k49"]["G_updates_per_s"] / r["k36"]["G_updates_per_s"], 3)
        gate.append((batch, name, r["k49"]["ms"], r["torch_bincount"]["ms"]))
        row[name] = r
        del out, out36, got
    row["constant_over_covers"] = round(row["constant"]["k49"]["ms"] / row["covers"]["k49"]["ms"], 3)
    res["batches"][str(batch)] = row
    del inputs
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
        model = srm.fit(root, ["LSBR"], [0.1])
        srm.score(root, model, ["LSBR"], [0.1])                               # warm-up
        times = []
        for _ in range(a.score_repeats):
            t0 = time.perf_counter()
            df = srm.score(root, model, ["LSBR"], [0.1])
            df.to_csv(root / "srm.csv", index=False)
            times.append(time.perf_counter() - t0)
        med = float(np.median(times))
        res["score_from_png"] = {"images": 10, "repeats": a.score_repeats, "s_per_pass": round(med, 5), "p10": round(float(np.percentile(times, 10)), 5),
                                 "p90": round(float(np.percentile(times, 90)), 5), "images_per_s": round(10 / med, 1)}
res["gate_k49_faster_than_torch"] = all(k < t for _, _, k, t in gate)
print(json.dumps(res))
slower = [(b, n, k, t) for b, n, k, t in gate if not k < t]
assert not slower, f"K49 is not faster than the torch composition: {slower}"
