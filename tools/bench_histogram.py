"""Time the kernels of the histogram attacks (ops.hist_segments, K58; ops.adjacency_hist, K59; ops.downsample2x2, K60) on one GPU and
print one JSON line.

  * K58 with 1 and 100 segments (and, without a torch formulation, with 4096: the most passes per workgroup), K59 and K60 on --batches (1 / 32 / 256) resident 512x512 planes of three kinds: the five fixture covers
    tiled, a constant plane (every update of K58 / K59 on one bin) and a uniform-noise plane (no two neighbouring updates of K59 share a
    bin);
  * beside each its torch formulation on the same planes: one torch.bincount of (image * S + s) * 256 + x for K58, one of
    image * 65536 + u * 256 + v for K59, the four-slice integer sum for K60; checked equal to the kernels' output;
  * beside them ops.spam_counts (K36), the nearest existing kernel that reads a plane once into LDS bins;
  * everything ALTERNATED in one process: a round times every (kind, function) once between HIP events (--inner back-to-back calls of a
    kernel, fewer of a torch formulation), --rounds rounds; reported: the median ms per call with the 10th and 90th percentile of the
    rounds, the ratio torch / kernel and kernel / K36, and each kind's time over the covers';
  * histogram.outputs whole per detector at --outputs-batch planes (wall clock with a device synchronise, host statistics included), and
    beside it the count kernels alone: the difference is the share of torch's FFT, the read-back and the host.
Usage: python tools/bench_histogram.py [--batches 1 32 256] [--rounds 9] [--inner 10] [--outputs-batch 32]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from ws_unet_amd import histogram, ops
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[1, 32, 256])
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--outputs-batch", type=int, default=32)
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])
H = W = 512
SEG_OF_T = (torch.arange(H * W, dtype=torch.int64, device="cuda") * 100) // (H * W)


def torch_segments(x, segments):
    n = x.shape[0]
    idx = x.reshape(n, -1).to(torch.int64) + torch.arange(n, device=x.device)[:, None] * (segments * 256)
    if segments > 1:
        idx = idx + SEG_OF_T[None, :] * 256
    return torch.bincount(idx.reshape(-1), minlength=n * segments * 256).reshape(n, segments, 256)


def torch_adjacency(x):
    n = x.shape[0]
    idx = x[:, :, :-1].to(torch.int64) * 256 + x[:, :, 1:].to(torch.int64) + torch.arange(n, device=x.device)[:, None, None] * 65536
    return torch.bincount(idx.reshape(-1), minlength=n * 65536).reshape(n, 256, 256)


def torch_downsample(x):
    s = x[:, 0::2, 0::2].to(torch.int32) + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]
    return (s >> 2).to(torch.uint8)


FUNCS = {"hist_segments_1": (lambda x: ops.hist_segments(x, 1), lambda x: torch_segments(x, 1)),
         "hist_segments_100": (lambda x: ops.hist_segments(x, 100), lambda x: torch_segments(x, 100)),
         "hist_segments_4096": (lambda x: ops.hist_segments(x, 4096), None),      # segments of 64 pixels: 128 passes per workgroup
         "adjacency_hist": (ops.adjacency_hist, torch_adjacency),
         "downsample2x2": (ops.downsample2x2, torch_downsample),
         "spam_counts": (ops.spam_counts, None)}


def timed(fn, x, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn(x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def stats(samples):
    return {"ms": round(float(np.median(samples)), 4), "p10": round(float(np.percentile(samples, 10)), 4), "p90": round(float(np.percentile(samples, 90)), 4)}


result = {"shape": [H, W], "rounds": a.rounds, "inner": a.inner, "batches": {}}
for batch in a.batches:
    rng = np.random.default_rng(46)
    planes = {"covers": torch.from_numpy(covers[np.arange(batch) % 5].copy()).to("cuda"),
              "constant": torch.full((batch, H, W), 77, dtype=torch.uint8, device="cuda"),
              "noise": torch.from_numpy(rng.integers(0, 256, (batch, H, W), dtype=np.uint8)).to("cuda")}
    runs = [(kind, name, which, fn) for kind in planes for name, pair in FUNCS.items() for which, fn in zip(("kernel", "torch"), pair) if fn is not None]
    for kind, name, which, fn in runs:                                  # warm-up, and the formulations against the kernels
        out = fn(planes[kind])
        if which == "torch":
            assert torch.equal(out, FUNCS[name][0](planes[kind])), f"{name} on {kind}: the kernel and the torch formulation differ"
    torch.cuda.synchronize()
    samples = {(kind, name, which): [] for kind, name, which, _ in runs}
    for _ in range(a.rounds):
        for kind, name, which, fn in runs:
            samples[(kind, name, which)].append(timed(fn, planes[kind], a.inner if which == "kernel" else max(1, a.inner // 5)))
    table = {}
    for kind in planes:
        k36 = float(np.median(samples[(kind, "spam_counts", "kernel")]))
        table[kind] = {}
        for name in FUNCS:
            row = {"kernel": stats(samples[(kind, name, "kernel")])}
            ms = row["kernel"]["ms"]
            if (kind, name, "torch") in samples:
                row["torch"] = stats(samples[(kind, name, "torch")])
                row["torch_over_kernel"] = round(row["torch"]["ms"] / ms, 2)
            row["over_k36"] = round(ms / k36, 3)
            row["over_covers"] = round(ms / float(np.median(samples[("covers", name, "kernel")])), 3)
            row["pixel_GB_per_s"] = round(batch * H * W / ms / 1e6, 1)
            table[kind][name] = row
    result["batches"][str(batch)] = table
    del planes

# the detectors whole, and the count kernels alone
x = torch.from_numpy(covers[np.arange(a.outputs_batch) % 5].copy()).to("cuda")
det = {}
for detector in histogram.DETECTORS:
    whole, counts = [], []
    for r in range(a.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        histogram.outputs(x, detector)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        histogram.tables(x, detector)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r:                                                           # the first round warms up (the FFT plans)
            whole.append((t1 - t0) * 1e3)
            counts.append((t2 - t1) * 1e3)
    det[detector] = {"outputs": stats(whole), "count_kernels": stats(counts),
                     "fft_and_host_share": round(1. - float(np.median(counts)) / float(np.median(whole)), 3)}
result["outputs"] = {"batch": a.outputs_batch, "detectors": det}
print(json.dumps(result))
