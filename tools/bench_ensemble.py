"""Time the float64 subspace Gram kernel (ops.subspace_gram, K53) and a whole Ensemble.fit on one GPU and print one JSON line.

  * K53 beside the torch baseline in the same process, alternated sample by sample after both were warmed at the shape: the baseline is,
    per learner, A = zt.index_select(0, idx_l); (A * w_l) @ A.T in float64 (a gathered copy, a full product).  Shape: n_rows 10 000,
    d 16 718, d_sub in --d-subs (500, 2 000), L 8.  Median, p10 and p90 of --reps samples between HIP events -> ms, useful flop/s
    counting n_rows d_sub (d_sub + 1) per learner for BOTH (the baseline executes about twice that), torch_over_k53;
  * a register-only loop of v_mfma_f64_16x16x4_f64 of the same library (wsu_mfma_f64_loop: 4 waves per workgroup, 4 accumulators per
    wave, 4 workgroups per CU's worth of grid), timed in the same run -> mfma_loop_tflops, and K53's share of THAT MEASURED LOOP
    (`share_of_mfma_loop`); no FP64 matrix peak is on record to quote instead;
  * the results are compared first (lower triangles within the rounding bound of the sum, against each other);
  * --fit: one whole Ensemble.fit (L 51, d_sub --fit-d-sub) on 2 x 5 000 rows of the same d, with the device stages synchronised, split
    into gram, solve, projection and host threshold, beside the wall clock of the call.
A line per stage goes to stderr as it ends.  It fails without a GPU.
Usage: python tools/bench_ensemble.py [--d-subs 500 2000] [--learners 8] [--reps 20] [--fit] [--fit-d-sub 500]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from ws_unet_amd import _lib, ensemble, ops

ap = argparse.ArgumentParser()
ap.add_argument("--n-rows", type=int, default=10000)
ap.add_argument("--d", type=int, default=16718)
ap.add_argument("--d-subs", nargs="+", type=int, default=[500, 2000])
ap.add_argument("--learners", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--fit", action="store_true")
ap.add_argument("--fit-d-sub", nargs="+", type=int, default=[500])
ap.add_argument("--fit-learners", type=int, default=51)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_ensemble.py measures on a GPU"
T0 = time.perf_counter()


def stage(text):
    print(f"[{time.perf_counter() - T0:7.1f} s] {text}", file=sys.stderr, flush=True)


def sample_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms, flops):
    ms = np.asarray(ms)
    med = float(np.median(ms))
    return {"ms": round(med, 4), "p10": round(float(np.percentile(ms, 10)), 4), "p90": round(float(np.percentile(ms, 90)), 4),
            "useful_tflops": round(flops / med / 1e9, 3)}


rng = np.random.default_rng(0)
n, d, L = a.n_rows, a.d, a.learners
X = rng.standard_normal((n, d))
X[n // 2:, ::7] += 0.05                                                      # two classes that differ a little in every seventh feature
Z = torch.from_numpy(X - X.mean(axis=0)).cuda()
zt = Z.T.contiguous()
del Z
stage(f"zt ({d}, {n}) float64 on the device")
result = {"device": torch.cuda.get_device_name(0), "n_rows": n, "d": d, "learners": L, "reps": a.reps, "shapes": {}}

# the register-only loop of the f64 MFMA
cus = torch.cuda.get_device_properties(0).multi_processor_count
blocks, iters = 4 * cus, 20000
sink = torch.empty(blocks * 256, dtype=torch.float64, device="cuda")
loop = _lib.load().wsu_mfma_f64_loop
run_loop = lambda: _lib.check(loop(sink.data_ptr(), blocks, iters, ops._stream()), "wsu_mfma_f64_loop")
for _ in range(2):
    run_loop()
torch.cuda.synchronize()
loop_ms = [sample_ms(run_loop) for _ in range(10)]
loop_flops = blocks * 4 * iters * 4 * 2048.
loop_tflops = loop_flops / float(np.median(loop_ms)) / 1e9
result["mfma_loop"] = {"blocks": blocks, "iters": iters, "ms": round(float(np.median(loop_ms)), 4), "p10": round(float(np.percentile(loop_ms, 10)), 4),
                       "p90": round(float(np.percentile(loop_ms, 90)), 4), "tflops": round(loop_tflops, 3)}
stage(f"register-only f64 MFMA loop: {loop_tflops:.2f} Tflop/s on {cus} CUs")

for ds in a.d_subs:
    idx = torch.from_numpy(np.stack([np.sort(rng.permutation(d)[:ds]) for _ in range(L)]).astype(np.int32)).cuda()
    wt = torch.from_numpy(np.stack([np.bincount(rng.integers(0, n, n), minlength=n) for _ in range(L)]).astype(np.int32)).cuda()
    out = torch.empty((L, ds, ds), dtype=torch.float64, device="cuda")
    ref = torch.empty_like(out)
    wf = wt.double()

    def k53():
        ops.subspace_gram(zt, idx, wt, out=out)

    def baseline():
        for l in range(L):
            A = zt.index_select(0, idx[l].long())
            torch.matmul(A * wf[l], A.T, out=ref[l])

    for _ in range(2):                                                      # warm both at this shape
        k53()
        baseline()
    torch.cuda.synchronize()
    scale = torch.sqrt(torch.diagonal(ref, dim1=1, dim2=2))
    worst = float(((out - ref).abs() / (scale[:, :, None] * scale[:, None, :])).max())
    assert worst <= 2 * (n + 2) * 2.0 ** -53, f"K53 and the torch baseline differ by {worst} of sqrt(G_aa G_bb) at d_sub {ds}"
    assert torch.equal(out, out.transpose(1, 2))
    ms_k, ms_t = [], []
    for _ in range(a.reps):                                                 # alternated
        ms_k.append(sample_ms(k53))
        ms_t.append(sample_ms(baseline))
    flops = float(L) * n * ds * (ds + 1)
    r = {"k53": stats(ms_k, flops), "torch": stats(ms_t, flops), "largest_difference_over_sqrt_GaaGbb": worst}
    r["torch_over_k53"] = round(r["torch"]["ms"] / r["k53"]["ms"], 3)
    r["share_of_mfma_loop"] = round(r["k53"]["useful_tflops"] / loop_tflops, 3)
    result["shapes"][str(ds)] = r
    stage(f"d_sub {ds}: K53 {r['k53']['ms']} ms ({r['k53']['useful_tflops']} useful Tflop/s, {r['share_of_mfma_loop']} of the measured MFMA loop), "
          f"torch {r['torch']['ms']} ms, torch / K53 {r['torch_over_k53']}")
    del out, ref, idx, wt, wf

if a.fit:
    m = ensemble.Ensemble(a.fit_learners, a.fit_d_sub, 0.1, 0)
    m.profile = True
    small = ensemble.Ensemble(3, 8, 0.1, 0)
    small.fit(X[:64, :64], X[n // 2:n // 2 + 64, :64])                      # warm torch's solver and the kernel
    t0 = time.perf_counter()
    m.fit(X[:n // 2], X[n // 2:])
    wall = time.perf_counter() - t0
    result["fit"] = {"learners": a.fit_learners, "d_sub": a.fit_d_sub, "rows": n, "wall_s": round(wall, 3),
                     **{k + "_s": round(v, 4) for k, v in m.timings.items()},
                     "other_s": round(wall - sum(m.timings.values()), 3), "oob_errors": m.oob_errors}
    stage(f"Ensemble.fit L {a.fit_learners} d_sub {a.fit_d_sub}: {wall:.2f} s wall; " + ", ".join(f"{k} {v:.3f} s" for k, v in m.timings.items()))

print(json.dumps(result))
