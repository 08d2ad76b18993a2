"""Time the stego-key scan (ops.ws_key_search, K35) on one GPU and print one JSON line.

The accumulators are those of ONE 512x512 fixture cover embedded with LSBRK at alpha 0.1 (KB predictor, weighted); the scan is at search
alpha 0.05 over --keys candidate keys (default 2^20) around the true one, in one process:
  * range mode (key_first, count) and list mode (the same keys as a device tensor): the whole op (padding, guard, launch) between HIP
    events, median of --reps calls after a warm-up call, and the kernel alone from the events ops.KernelTimer puts around the launch;
    keys/s from the kernel's time; range and list are timed alternately;
  * a short key list over the whole frame, the second stage of a search: --stage2-keys keys (1024) with the automatic `parts` against one
    owner per key (parts 1), median of --reps x 4 kernel times, alternating;
  * the same search with what the library had before K35: ops.lsbr_key_mask per key and torch masked sums, on --baseline-keys keys,
    wall clock around the loop ending in a synchronise; its keys/s and the ratio;
  * the kernel's 32 x 32 -> 64 bit products per second (20 per quad of pixels and key) and their share of the chip's vector issue rate,
    256 CUs x 4 SIMDs x 32 lanes per cycle at 2.4 GHz, the rate of a full-rate vector instruction; and the same share if the 64-bit
    multiply-add a product compiles to issues at a quarter of that rate, as 32-bit integer multiplies do on earlier CDNA parts (an
    assumption: the rate of that instruction on this chip was not measured).  The products are not all the kernel does.
The device sums are checked against tests/keysearch_np.py and against the mask-per-key search on the first keys, and the true key must
come out on top.
Usage: python tools/bench_keysearch.py [--keys 1048576] [--reps 5] [--baseline-keys 2000] [--stage2-keys 1024]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch

import keysearch_np
from ws_unet_amd import filters, ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import keysearch, locate

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--baseline-keys", type=int, default=2000)
ap.add_argument("--stage2-keys", type=int, default=1024)
a = ap.parse_args()
H = W = 512
KEY, FIRST = 2 ** 40 + 12345, 2 ** 40
assert FIRST <= KEY < FIRST + a.keys
cover = torch.from_numpy(np.ascontiguousarray(imread4_u8(ROOT / "tests" / "golden" / "cover_6.png")[..., 3])[None]).to("cuda")
stego = ops.embed_lsbr_keyed(cover, torch.tensor([77], dtype=torch.int64, device="cuda"), KEY, ops.lsbr_key_threshold(0.1))[0]
acc = locate.ResidualAccumulator(H, W, "cuda").add(stego, filters.get_filter_estimator(filter_name="KB", flatten=False), weighted=1)
thr = ops.lsbr_key_threshold(0.05)
keys = torch.arange(a.keys, dtype=torch.int64, device="cuda") + FIRST
modes = {"range": dict(key_first=FIRST, count=a.keys), "list": dict(keys=keys)}


modes |= {f"stage2_parts{p}": dict(keys=keys[:a.stage2_keys], parts=p) for p in (0, 1)}
SCANS = ("range", "list")


def scan(mode):
    return ops.ws_key_search(acc.num, acc.den, H, W, alpha_threshold=thr, **modes[mode])


def timed(mode):
    """one call: (ms of the whole op between events, ms of the kernel launch alone)"""
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    scan(mode)
    e1.record()
    e1.synchronize()
    ops.set_timer(None)
    (_, _, s, e), = [r for r in timer.records if r[0] == "ws_key_search"]
    return e0.elapsed_time(e1), s.elapsed_time(e)


for mode in modes:
    scan(mode)
torch.cuda.synchronize()
samples = {mode: [] for mode in modes}
for _ in range(a.reps):
    for mode in SCANS:
        samples[mode].append(timed(mode))
for _ in range(4 * a.reps):
    for mode in modes:
        if mode not in SCANS:
            samples[mode].append(timed(mode))
quads = H * W // 4
out = {"shape": [H, W], "keys": a.keys, "search_alpha": 0.05, "reps": a.reps}
for mode in SCANS:
    s = samples[mode]
    op_ms, kernel_ms = float(np.median([v[0] for v in s])), float(np.median([v[1] for v in s]))
    products = 20.0 * quads * a.keys / (kernel_ms * 1e-3)
    out[mode] = {"op_ms": round(op_ms, 3), "kernel_ms": round(kernel_ms, 3), "kernel_ms_all": [round(v[1], 3) for v in s],
                 "keys_per_s": round(a.keys / kernel_ms * 1e3, 1), "keys_per_s_whole_op": round(a.keys / op_ms * 1e3, 1),
                 "products_per_s": float(f"{products:.4g}"), "share_of_vector_issue_rate": round(products / (256 * 4 * 32 * 2.4e9), 4),
                 "share_of_quarter_rate_multiplies": round(4 * products / (256 * 4 * 32 * 2.4e9), 4)}
for mode in modes:
    if mode not in SCANS:
        ms = float(np.median([v[1] for v in samples[mode]]))
        out[mode] = {"keys": a.stage2_keys, "kernel_ms": round(ms, 4), "keys_per_s": round(a.stage2_keys / ms * 1e3, 1)}

# the search as the library offered it before: one mask per key, two masked sums
n = a.baseline_keys
num, den = acc.num, acc.den


def by_masks(count):
    sn = torch.empty(count, dtype=torch.int64, device="cuda")
    sd = torch.empty(count, dtype=torch.int64, device="cuda")
    for j in range(count):
        m = ops.lsbr_key_mask(FIRST + j, thr, H, W)[1:-1, 1:-1].to(torch.int64)
        sn[j] = (num * m).sum()
        sd[j] = (den * m).sum()
    return sn, sd


by_masks(50)
torch.cuda.synchronize()
t0 = time.perf_counter()
base = by_masks(n)
torch.cuda.synchronize()
sec = time.perf_counter() - t0
out["mask_per_key"] = {"keys": n, "seconds": round(sec, 3), "keys_per_s": round(n / sec, 1)}
out["kernel_over_mask_per_key"] = {mode: round(out[mode]["keys_per_s"] / (n / sec), 1) for mode in SCANS}

got = [scan(mode) for mode in SCANS]
short = [scan(mode) for mode in modes if mode not in SCANS]
assert all(torch.equal(t, got[0][i][:a.stage2_keys]) for pair in short for i, t in enumerate(pair)), "the short list's sums differ"
assert all(torch.equal(got[0][i], got[1][i]) for i in (0, 1)), "range and list mode differ"
assert torch.equal(got[0][0][:n], base[0]) and torch.equal(got[0][1][:n], base[1]), "kernel and mask-per-key sums differ"
want = keysearch_np.key_sums(*keysearch_np.frames(num.cpu().numpy(), den.cpu().numpy()), keysearch_np.key_range(FIRST, 8), thr)
assert np.array_equal(got[0][0][:8].cpu().numpy(), want[0]) and np.array_equal(got[0][1][:8].cpu().numpy(), want[1]), "kernel and numpy sums differ"
score = keysearch.scores(*got[0])
best = int(torch.argmax(torch.nan_to_num(score, nan=-1e9)))
assert best == KEY - FIRST, f"the true key is not on top: {best}"
out["true_key_score"] = round(float(score[best]), 4)
out["true_key_z"] = round(float(keysearch.standardise(score)[best]), 1)
print(json.dumps(out))
