"""Time the SPAM count kernel (ops.spam_counts, K36) on one GPU and print one JSON line.

  * K36 on --batch resident 512x512 planes of three kinds -- the five fixture covers tiled, a constant plane, uniform noise -- per
    (order, T) of --configs: median of --reps samples between HIP events after warm-up, each sample --inner back-to-back calls (the
    output's memset and the kernel; one call is tens of microseconds, the size of an event's own resolution) -> ms per call, images/s,
    GB/s of pixels read (1 byte per pixel) and the share of the HBM read floor (the N H W bytes at the 8 TB/s of the data sheet);
  * the same counts from a torch composition on the device in the same process (differences of shifted slices, clamp, the bin index,
    one torch.bincount per direction over the whole batch): what a user could do before K36; checked equal, timed the same way;
  * --ab-lib FILE --ab-name NAME: an A/B against another build of the entry point, for instance another commit's
        hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-slp-vectorize -shared \
              ws_unet_amd/csrc/wsu_common.hip ws_unet_amd/csrc/spam.hip -o FILE
    Both arms run in this process, alternating sample by sample, results checked equal first (profiles/r29 compared the register path
    for the centre bins with all LDS atomics this way);
  * --score-repeats R: `spam.score` end to end from PNG files (decode, upload, K36, features, the discriminant) over the five fixture
    covers and their LSBR 0.1 twins, R times after one warm-up pass, by the wall clock -> images/s.
Usage: python tools/bench_spam.py [--batch 32] [--reps 100] [--inner 50] [--configs 2,3 1,4] [--ab-lib FILE [--ab-name NAME]] [--score-repeats 20]"""
import argparse
import ctypes
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

import spam_np
from ws_unet_amd import _lib, ops, spam
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--configs", nargs="+", default=["2,3", "1,4"], help="order,T pairs")
ap.add_argument("--ab-lib", default=None)
ap.add_argument("--ab-name", default="all_lds_atomics", help="what the build of --ab-lib is, for the record")
ap.add_argument("--score-repeats", type=int, default=0)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_spam.py measures on a GPU"
HBM_PEAK = 8.0e12                                                            # bytes/s, the data sheet's
H = W = 512
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])
inputs = {"covers": torch.from_numpy(covers[np.arange(a.batch) % 5].copy()).cuda(),
          "constant": torch.full((a.batch, H, W), 77, dtype=torch.uint8, device="cuda"),
          "noise": torch.from_numpy(np.random.default_rng(1).integers(0, 256, (a.batch, H, W), dtype=np.uint8)).cuda()}
nbytes = a.batch * H * W


def torch_counts(x, order, T):
    """(N,4,bins) int64 by index arithmetic and one bincount per direction"""
    n, h, w = x.shape
    B, k, nb = 2 * T + 1, order + 1, spam.bins(order, T)
    xi = x.to(torch.int32)
    base = (torch.arange(n, device=x.device, dtype=torch.int64) * nb)[:, None, None]
    out = []
    for dr, dc in spam_np.STEPS:
        c_lo, c_hi = max(0, -k * dc), w - max(0, k * dc)
        at = lambda j: xi[:, j * dr:h - k * dr + j * dr, c_lo + j * dc:c_hi + j * dc]
        idx = None
        for j in range(order + 1):
            d = (at(j) - at(j + 1)).clamp_(-T, T) + T
            idx = d if idx is None else idx * B + d
        out.append(torch.bincount((idx.to(torch.int64) + base).flatten(), minlength=n * nb).view(n, nb))
    return torch.stack(out, dim=1)


def samples_ms(fns, inner, reps):
    """per fn the ms per call of `reps` samples of `inner` back-to-back calls, the fns alternating sample by sample"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for j, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[j].append(e0.elapsed_time(e1) / inner)
    return [np.asarray(m) for m in ms]


def stats(ms):
    med = float(np.median(ms))
    return {"ms": round(med, 5), "p10": round(float(np.percentile(ms, 10)), 5), "p90": round(float(np.percentile(ms, 90)), 5),
            "images_per_s": round(a.batch / med * 1e3, 1), "pixel_GB_per_s": round(nbytes / med / 1e6, 1),
            "share_of_hbm_floor": round(nbytes / HBM_PEAK * 1e3 / med, 4)}


ab = None
if a.ab_lib:
    ab = ctypes.CDLL(str(Path(a.ab_lib).resolve()))
    ab.wsu_spam_counts.restype, ab.wsu_spam_counts.argtypes = _lib.SIGNATURES["wsu_spam_counts"]

res = {"batch": a.batch, "shape": [H, W], "reps": a.reps, "inner": a.inner, "hbm_floor_ms": round(nbytes / HBM_PEAK * 1e3, 5), "configs": {}}
for cfg in a.configs:
    order, T = (int(v) for v in cfg.split(","))
    nb = spam.bins(order, T)
    row = {}
    for name, x in inputs.items():
        out = torch.empty((a.batch, 4, nb), dtype=torch.int64, device="cuda")
        got = ops.spam_counts(x, order, T)
        assert torch.equal(got, torch_counts(x, order, T)), f"{cfg} {name}: K36 and the torch composition differ"
        assert np.array_equal(got[:5].cpu().numpy(), spam_np.counts(x[:5].cpu().numpy(), order, T)), f"{cfg} {name}: K36 and numpy differ"
        fns = [lambda: ops.spam_counts(x, order, T, out=out)]
        if ab is not None:
            out_ab = torch.empty_like(out)
            call_ab = lambda: ab.wsu_spam_counts(x.data_ptr(), out_ab.data_ptr(), a.batch, H, W, order, T, ops._stream())
            assert call_ab() == 0 and torch.equal(out_ab, got), f"{cfg} {name}: the {a.ab_name} build differs"
            fns.append(call_ab)
        ms = samples_ms(fns, a.inner, a.reps)
        t_ms, = samples_ms([lambda: torch_counts(x, order, T)], max(1, a.inner // 10), max(5, a.reps // 5))
        row[name] = {"k36": stats(ms[0]), "torch_bincount": stats(t_ms), "torch_over_k36": round(float(np.median(t_ms) / np.median(ms[0])), 1)}
        if ab is not None:
            row[name][a.ab_name] = stats(ms[1])
            row[name][f"{a.ab_name}_over_k36"] = round(float(np.median(ms[1]) / np.median(ms[0])), 3)
    row["constant_over_covers"] = round(row["constant"]["k36"]["ms"] / row["covers"]["k36"]["ms"], 3)
    res["configs"][cfg] = row

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
        model = spam.fit(root, ["LSBR"], [0.1])
        spam.score(root, model, ["LSBR"], [0.1])                              # warm-up
        times = []
        for _ in range(a.score_repeats):
            t0 = time.perf_counter()
            df = spam.score(root, model, ["LSBR"], [0.1])
            df.to_csv(root / "spam.csv", index=False)
            times.append(time.perf_counter() - t0)
        med = float(np.median(times))
        res["score_from_png"] = {"images": 10, "repeats": a.score_repeats, "s_per_pass": round(med, 5), "p10": round(float(np.percentile(times, 10)), 5),
                                 "p90": round(float(np.percentile(times, 90)), 5), "images_per_s": round(10 / med, 1)}
print(json.dumps(res))
