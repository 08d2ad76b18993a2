"""Time the training-batch assembly on one GPU and print one JSON line.

48 resident uint8 planes of 512x512 (16 covers, two twins each) -> the 64 samples of a batch (cover, stego interleaved; inputs and targets):
  (a) parent  the assembly the pair loader used before wsu_pair_batch_f32: ops.u8_to_unit over every plane, then two fp32 index gathers
  (b) op0     wsu_pair_batch_f32 with op = 0 for every sample (the same bits as (a): asserted before anything is timed)
  (c) flips   wsu_pair_batch_f32 with ops uniform over 0..3, one per pair
  (d) d4      wsu_pair_batch_f32 with ops uniform over 0..7, one per pair
Per case: the median of --reps timings after a warm-up, each --inner back-to-back calls between two HIP events (one call is tens of
microseconds: a window of one would measure the events), repeated --repeats times (median of the medians, and their min / max as the spread), and the achieved bytes/s on the case's algorithmic traffic (every plane read once, every output written once;
(a) also writes and re-reads the fp32 planes).  (a)-(d) run with their index arrays resident, the kernels alone; `d4_wrapper` is (d)
through ops.pair_batch, with the validation and the upload of the 9-byte-per-sample index block that the loader pays.
Usage: python tools/bench_pair_batch.py [--size 512] [--reps 20] [--inner 20] [--repeats 5]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from ws_unet_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda")
ncov, pairs = 16, 32
planes = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (3 * ncov, a.size, a.size), dtype=np.uint8)).to(dev)
idx_in = np.array([j for i in range(pairs) for j in (i % ncov, ncov + i)])
idx_cov = np.array([i % ncov for i in range(pairs) for _ in (0, 1)])
ti, tc = torch.from_numpy(idx_in).to(dev), torch.from_numpy(idx_cov).to(dev)
rng = np.random.default_rng(1)
op = {"op0": np.zeros(2 * pairs, np.uint8), "flips": np.repeat(rng.integers(0, 4, pairs), 2).astype(np.uint8),
      "d4": np.repeat(rng.integers(0, 8, pairs), 2).astype(np.uint8)}


def parent():
    unit = ops.u8_to_unit(planes)[:, None]
    return unit[ti], unit[tc]


lib = _lib.load()
ti32, tc32 = ti.int(), tc.int()
x = torch.empty((2 * pairs, 1, a.size, a.size), dtype=torch.float32, device=dev)
c = torch.empty_like(x)


def kernel(op_dev):
    _lib.check(lib.wsu_pair_batch_f32(planes.data_ptr(), planes.shape[0], a.size, a.size, ti32.data_ptr(), tc32.data_ptr(), op_dev.data_ptr(),
                                      2 * pairs, 1, x.data_ptr(), c.data_ptr(), torch.cuda.current_stream().cuda_stream), "wsu_pair_batch_f32")


cases = {"parent": parent, **{k: (lambda v=torch.from_numpy(v).to(dev): kernel(v)) for k, v in op.items()},
         "d4_wrapper": lambda: ops.pair_batch(planes, idx_in, idx_cov, op["d4"])}
hw, n = a.size * a.size, 2 * pairs
traffic = {k: planes.shape[0] * hw + 2 * n * 4 * hw for k in cases}
traffic["parent"] = planes.shape[0] * hw * 5 + 2 * 2 * n * 4 * hw


def median_ms(fn):
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
    return float(np.median(ms))


want = parent()
got = ops.pair_batch(planes, idx_in, idx_cov, op["op0"])
assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "op = 0 is not the parent's assembly"
out = {"planes": int(planes.shape[0]), "samples": n, "size": a.size, "reps": a.reps, "inner": a.inner, "repeats": a.repeats, "cases": {}}
for k, fn in cases.items():
    meds = [median_ms(fn) for _ in range(a.repeats)]
    m = float(np.median(meds))
    out["cases"][k] = {"ms": round(m, 4), "ms_min": round(min(meds), 4), "ms_max": round(max(meds), 4), "bytes": traffic[k],
                       "GB_per_s": round(traffic[k] / m / 1e6, 1)}
print(json.dumps(out))
