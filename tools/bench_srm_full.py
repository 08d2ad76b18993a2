"""Time the SRM fan and EDGE count kernels (ops.srm_fan_counts, K54; ops.srm_edge_counts, K55) on one GPU and print one JSON line.

  * K54 and K55 on 1, 32 and 256 (--batches) resident 512x512 planes of three kinds -- the five fixture covers tiled, a constant plane,
    uniform noise: median of --reps samples between HIP events after warm-up, each sample --inner back-to-back calls (the output's memset
    and the kernel) -> ms per call, images/s, bin updates per second (400 and 264 per pixel);
  * the same counts from a torch composition on the device in the same process (the members' residuals from shifted slices, the digit in
    integers, torch.minimum / torch.maximum over a set, the bin indices of both halves, one torch.bincount per table over the whole
    batch): what a user could do without the kernels; checked equal first, timed the same way with fewer samples.  THE GATE (K50's): each
    kernel must be faster than this composition on all three kinds of plane at every batch, or the script fails;
  * K50 (ops.srm_minmax_counts: 236 bin updates per pixel) on the same inputs in the same process, as the yardstick for bin updates per
    second; the ratios and constant_over_covers are reported, not gated;
  * --score-repeats R: `srm.score` end to end from PNG files over the five fixture covers and their LSBR 0.1 twins with submodels='full',
    R times after one warm-up pass, by the wall clock -> images/s; and with submodels='linear' and 'all', alternated pass by pass with
    the `srm.py` of another commit given as --parent-srm FILE (loaded into this process as a second module of the package): both
    medians and spreads.
Usage: python tools/bench_srm_full.py [--batches 1 32 256] [--reps 50] [--inner 10] [--score-repeats 10] [--parent-srm FILE]"""
import argparse
import importlib.util
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

import srm_edge_np as edge_np
import srm_fans_np as fans_np
from ws_unet_amd import ops, srm
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batches", nargs="*", type=int, default=[1, 32, 256])
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--score-repeats", type=int, default=0)
ap.add_argument("--parent-srm", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_srm_full.py measures on a GPU"
H = W = 512
KERNELS = {"k54": (ops.srm_fan_counts, fans_np, ops.SRM_FAN_TABLES), "k55": (ops.srm_edge_counts, edge_np, ops.SRM_EDGE_TABLES)}
UPDATES50 = 2 * len(ops.SRM_MINMAX_TABLES)
gold = ROOT / "tests" / "golden"
covers = np.stack([imread4_u8(gold / f"cover_{k}.png")[..., 3] for k in (6, 7, 8, 9, 10)])


def torch_counts(x, ref):
    """(N,T,625) int64 of the restatement `ref`'s tables: shifted slices, the integer digit, minimum / maximum over the set, one bincount
    per table"""
    n, h, w = x.shape
    xi = x.to(torch.int32)
    base = (torch.arange(n, device=x.device, dtype=torch.int64) * ops.SRM_BINS)[:, None]
    out, residuals = [], {}
    for cls, q2, name, scan in ref.TABLES:
        if (cls, name) not in residuals:
            u, dn, l, rt = ref.reach(cls, name)
            hh, ww = h - u - dn, w - l - rt
            members = []
            for member in ref.SETS[name]:
                R = torch.zeros((n, hh, ww), dtype=torch.int32, device=x.device)
                for (dr, dc), wt in ref.CLASSES[cls][1][member].items():
                    R += wt * xi[:, u + dr:u + dr + hh, l + dc:l + dc + ww]
                members.append((R.abs() * 4, R.sign()))
            residuals[cls, name] = members
        digits = [sign * torch.clamp((mag4 + q2) // (2 * q2), max=2) for mag4, sign in residuals[cls, name]]
        lo, hi = digits[0], digits[0]
        for d in digits[1:]:
            lo, hi = torch.minimum(lo, d), torch.maximum(hi, d)
        idx = []
        for d in (lo + 2, 2 - hi):
            hh, ww = d.shape[1:]
            runs = [d[:, :, k:ww - 3 + k] for k in range(4)] if scan == "h" else [d[:, k:hh - 3 + k, :] for k in range(4)]
            idx.append((((runs[0] * 5 + runs[1]) * 5 + runs[2]) * 5 + runs[3]).reshape(n, -1).to(torch.int64) + base)
        out.append(torch.bincount(torch.cat(idx, dim=1).flatten(), minlength=n * ops.SRM_BINS).view(n, ops.SRM_BINS))
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
        inner = a.inner if batch < 256 else max(1, a.inner // 5)
        out50 = torch.empty((batch, len(ops.SRM_MINMAX_TABLES), ops.SRM_BINS), dtype=torch.int64, device="cuda")
        r = {"k50": stats(samples_ms(lambda: ops.srm_minmax_counts(x, out=out50), inner, a.reps), batch, UPDATES50)}
        del out50
        for k, (op, ref, tables) in KERNELS.items():
            updates = 2 * len(tables)
            got = op(x)
            # the composition holds a set's members for the whole batch: at 256 planes in slabs of 32
            tc_fn = lambda: torch.cat([torch_counts(x[i:i + 32], ref) for i in range(0, batch, 32)])
            assert torch.equal(got, tc_fn()), f"batch {batch} {name}: {k} and the torch composition differ"
            assert np.array_equal(got[:1].cpu().numpy(), ref.counts(x[:1].cpu().numpy())), f"batch {batch} {name}: {k} and numpy differ"
            out = torch.empty((batch, len(tables), ops.SRM_BINS), dtype=torch.int64, device="cuda")
            r[k] = stats(samples_ms(lambda: op(x, out=out), inner, a.reps), batch, updates)
            r[f"torch_{k}"] = stats(samples_ms(tc_fn, 1, max(2, a.reps // 10), warm=0), batch, updates)   # (the equality check above was its warm-up)
            r[f"torch_over_{k}"] = round(r[f"torch_{k}"]["ms"] / r[k]["ms"], 1)
            r[f"{k}_over_k50_updates_per_s"] = round(r[k]["G_updates_per_s"] / r["k50"]["G_updates_per_s"], 3)
            gate.append((batch, name, k, r[k]["ms"], r[f"torch_{k}"]["ms"]))
            del out, got
        row[name] = r
    for k in ("k50", *KERNELS):
        row[f"constant_over_covers_{k}"] = round(row["constant"][k]["ms"] / row["covers"][k]["ms"], 3)
    res["batches"][str(batch)] = row
    del inputs
    torch.cuda.empty_cache()


def wall(times, images):
    med = float(np.median(times))
    return {"images": images, "repeats": len(times), "s_per_pass": round(med, 5), "p10": round(float(np.percentile(times, 10)), 5),
            "p90": round(float(np.percentile(times, 90)), 5), "images_per_s": round(images / med, 1)}


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

        def passes(module, model, **kw):
            t0 = time.perf_counter()
            module.score(root, model, ["LSBR"], [0.1], **kw).to_csv(root / "srm.csv", index=False)
            return time.perf_counter() - t0

        t0 = time.perf_counter()
        model = srm.fit(root, ["LSBR"], [0.1], submodels="full")
        res["fit_full_from_png_s"] = round(time.perf_counter() - t0, 4)
        passes(srm, model, submodels="full")                                   # warm-up
        res["score_full_from_png"] = wall([passes(srm, model, submodels="full") for _ in range(a.score_repeats)], 10)
        modules = {"this": srm}
        if a.parent_srm:
            spec = importlib.util.spec_from_file_location("ws_unet_amd.srm_parent", a.parent_srm)
            modules["parent"] = importlib.util.module_from_spec(spec)
            sys.modules[spec.name] = modules["parent"]
            spec.loader.exec_module(modules["parent"])
        for sub in ("linear", "all"):
            trees = {k: (module, module.fit(root, ["LSBR"], [0.1], submodels=sub)) for k, module in modules.items()}
            if a.parent_srm:
                assert np.array_equal(trees["parent"][1].w, trees["this"][1].w), f"the {sub} model differs from the parent's"
            times = {k: [] for k in trees}
            for k, (module, m) in trees.items():
                passes(module, m, submodels=sub)                               # warm-up
            for rep in range(a.score_repeats):                                 # alternated pass by pass, the first of a pair in turn
                for k, (module, m) in list(trees.items())[::1 if rep % 2 == 0 else -1]:
                    times[k].append(passes(module, m, submodels=sub))
            res[f"score_{sub}_from_png"] = {k: wall(v, 10) for k, v in times.items()}
res["gate_faster_than_torch"] = all(k < t for *_, k, t in gate)
print(json.dumps(res))
slower = [g for g in gate if not g[3] < g[4]]
assert not slower, f"a kernel is not faster than the torch composition: {slower}"
