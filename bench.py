#!/usr/bin/env python3
"""Headline benchmark: 512x512 grayscale images/sec of UNet predict (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run does what the headline needs and no more: it sets up, warms up, times the K steps, writes the outputs if asked and
prints the result line (with the roofline figures of the timed steps themselves).  `--full` adds the legs that take runs of
their own -- the other precision modes, the batch-1 latency, the train step, the CPU baseline with `mae_vs_cpu_oracle` and
the MAE on trained-like weights (each can be left out again with its --no-* option); they run after the timed steps, so
they change neither the timing nor the dumped outputs.

N = 1 runs in this process.  N > 1 without a torch.distributed.run environment launches N fresh rank processes itself
(`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py ...`, before this
process has touched the GPU), relays rank 0's JSON line and exits with the children's return code; when the driver
launches it under torch.distributed.run the RANK / WORLD_SIZE environment is used as is.

Workload (`config.workload`): BASELINE.json configs[1] -- `unet_2` forward-only predict on a batch of 32 synthetic
512x512x1 images per GPU, inputs already resident in HBM as the fp32 (N,1,H,W) tensor the model boundary takes.
One step = one forward pass over one batch.  Multi-GPU = batch sharding: each rank predicts its own 32 images (weak
scaling), no data-path collective; a barrier brackets the timed region and the slowest rank's time is used.

Precision: default mode 'f16f4p' (exact f16 products on the f16 matrix pipe + the two residual cross terms of the 3x3 convs as one
block-scaled fp4 operand pair per tap pair, fp32 accumulate; planar activation storage fed by LDS-DMA) -- the fastest mode that meets
the 1e-4 MAE gate against the fp32 CPU oracle (2.1e-5; `mae_vs_cpu_oracle` is measured in every --full run); the other modes ('f16f8p' =
the cross terms in e4m3: MAE 4e-6; 'f16f8' = that arithmetic on NHWC storage, 'bf16', 'f32', 'bf16x3', 'bf16x3s') are measured in a --full
run with fewer steps (`other_modes`).

Extra JSON objects on the one line rank 0 prints (all but `roofline` only with --full):
  roofline      dominant kernel = conv3x3 implicit GEMM: algorithmic FLOPs / HIP-event launch time vs the dense f16/bf16 MFMA
                peak; `per_layer` = every launch of the forward with max(t_flop, t_byte) at the vendor peaks against its
                measured time, their sum, and the HBM-bound transposed convs against 8 TB/s
  cpu_baseline  the CPU oracle (torch-CPU restatement of the reference) on a bounded sample of the same images, batch 1 with
                autograd on exactly like the reference's infere_single; `cpu_baseline_best_effort` = the same model under
                no_grad at batch 8 (what a careful CPU user would run), so that the speed-up is not inflated
  train_step    BASELINE.json configs[2]: fwd + L1WS + bwd + AdamW at batch 64 of 512x512 (N = 1 only)
  latency_b1    the reference's call pattern (one image per call): GPU / wall time of a batch-1 forward and, per layer, the share of the
                256 CUs the persistent grid occupies (N = 1 only)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

DEFAULT_MODE = "f16f4p"        # = ws_unet_amd's default inference mode (model/unet.py)
PEAK = {"bf16x3": 2.5e15, "bf16x3s": 2.5e15, "f16f8": 2.5e15, "f16f8p": 2.5e15, "f16f8q": 2.5e15, "f16f4p": 2.5e15, "bf16": 2.5e15, "f32": 157.3e12}     # dense MFMA peaks, MI355X_MICROARCH.md
HBM_PEAK = 8.0e12
NUM_CU = 256
TRAIN_FLOP_PER_IMAGE_512 = 606.0e9        # 3 x forward minus the e11 data gradient


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default=os.environ.get("WSU_BENCH_MODE", DEFAULT_MODE), choices=["bf16x3", "bf16x3s", "f16f8", "f16f8p", "f16f8q", "f16f4p", "bf16", "f32"])
    ap.add_argument("--batch", type=int, default=32, help="images per GPU per step")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure the other precision modes, the batch-1 latency, the train step, the CPU baseline "
                         "(mae_vs_cpu_oracle) and the MAE on trained-like weights (N = 1 only); the --no-* options leave single legs out")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-modes", action="store_true")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--no-trained-mae", action="store_true")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned (the (B,1,H,W) fp32 prediction of rank 0) as DIR/output.npy; "
                         "above 60 MB only the first images that fit are written.  The inputs are seeded, so two builds can be compared output for output")
    ap.add_argument("--detail", default=None, help="write the full result (per-layer tables, notes) as JSON to this file; the printed line is the compact form (< 8 KB)")
    ap.add_argument("--train-batch", type=int, default=64)
    ap.add_argument("--rehearse", action="store_true",
                    help="launcher rehearsal without GPUs: the ranks form a gloo group, run the barrier / max-over-ranks timing code around an "
                         "empty step and rank 0 prints a line marked rehearsal (tests/test_host_logic.py; never a measurement)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    return args


# ---------------------------------------------------------------------------------------------------------------------
# N > 1 launched as plain `python bench.py --gpus N`: spawn the ranks BEFORE anything in this process touches the GPU
# ---------------------------------------------------------------------------------------------------------------------
def visible_gpus():
    """GPUs this process could use, counted WITHOUT touching the GPU runtime (no torch / HIP import in the launching parent): the render
    nodes the kernel driver exposes, capped by a visibility list in the environment.  None = cannot tell (let the ranks find out)."""
    import glob
    n = len(glob.glob("/dev/dri/renderD*"))
    if n == 0 and not os.path.isdir("/dev/dri"):
        return 0 if not os.path.exists("/dev/kfd") else None
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([t for t in v.split(",") if t.strip() != ""]))
    return n


def self_launch(args) -> int:
    import socket
    have = None if args.rehearse else visible_gpus()
    if have is not None and have < args.gpus:
        print(f"bench.py: --gpus {args.gpus} needs {args.gpus} GPUs, {have} visible", file=sys.stderr)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")              # dmabuf IPC: RCCL needs it on this pool
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line)
    if proc.returncode == 0 and line is None:
        print("bench.py: the rank processes printed no result line", file=sys.stderr)
        return 1
    return proc.returncode


# ---------------------------------------------------------------------------------------------------------------------
def build_model(mode, dev):
    import torch
    from ws_unet_amd import formula
    from ws_unet_amd.model import get_model
    m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode=mode)
    sd = formula.formula_state_dict(2, "he")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev)


def timed_steps(model, x, steps, warmup, use_dist, timer=None):
    import torch
    import torch.distributed as dist
    from ws_unet_amd import ops
    with torch.no_grad():
        for _ in range(warmup):
            model(x)
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        ops.set_timer(timer)
        t0 = time.perf_counter()
        for _ in range(steps):
            y = model(x)
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ops.set_timer(None)
        ops.set_layer(None)
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device=x.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    return dt, y


DUMP_LIMIT_BYTES = 60 * 10 ** 6            # below 64 MB with the .npy header


def dump_outputs(out_dir, y_host) -> dict:
    """Writes the timed path's last output as float32 DIR/output.npy: the whole batch, or its first images up to DUMP_LIMIT_BYTES."""
    import numpy as np
    a = y_host.float().numpy()
    per_image = a[0].nbytes if a.shape[0] else 1
    keep = min(a.shape[0], max(1, DUMP_LIMIT_BYTES // per_image))
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / "output.npy", np.ascontiguousarray(a[:keep]))
    return {"dir": str(d), "files": {"output": list(a[:keep].shape)}, "images": f"{keep} of {a.shape[0]}"}


def host_cpus():
    """(usable cores, how they were counted): the affinity mask, capped by the cgroup CPU quota when there is one --
    oversubscribing oneDNN's thread pool on a 16-core share of a 256-core host made the baseline 10x slower than it should be."""
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = os.cpu_count() or 1
    quota = None
    try:
        q, per = Path("/sys/fs/cgroup/cpu.max").read_text().split()[:2]
        if q != "max":
            quota = max(1, int(int(q) / int(per)))
    except Exception:
        pass
    n = aff if quota is None else min(aff, quota)
    env = os.environ.get("WSU_CPU_THREADS")
    if env:
        n = max(1, min(n, int(env)))
    return n, {"affinity": aff, "cgroup_quota": quota, "host": os.cpu_count(), "WSU_CPU_THREADS": env}


def cpu_baseline(sample_u8, budget_s=14.0):
    """Reference-faithful CPU path: batch 1 per call, autograd enabled (infere_single has no no_grad,
    src/unet/evaluate.py:48), fp32, all usable host threads.  Bounded: stops after `budget_s` seconds."""
    import numpy as np
    import torch
    from ws_unet_amd import formula
    from oracle import unet_ref
    ncpu, how = host_cpus()
    torch.set_num_threads(ncpu)
    ref = unet_ref.build_ref(2, formula.formula_state_dict(2, "he"))
    outs, times = [], []
    x_all = torch.from_numpy(sample_u8.astype(np.float32) / np.float32(255.))[:, None]
    ref(x_all[:1].clone())                                      # warm-up (oneDNN primitive creation)
    t_start = time.perf_counter()
    for i in range(x_all.shape[0]):
        t0 = time.perf_counter()
        y = ref(x_all[i:i + 1].clone())
        times.append(time.perf_counter() - t0)
        outs.append(y.detach())
        if time.perf_counter() - t_start > budget_s:
            break
    # best effort on the same cores: no autograd graph, batch 8 (SURVEY 8d / BASELINE.md section 3)
    be_times = []
    with torch.no_grad():
        xb = x_all[:8].clone()
        ref(xb)
        t_start = time.perf_counter()
        while len(be_times) < 3 or (len(be_times) < 5 and time.perf_counter() - t_start < 10.0):
            t0 = time.perf_counter()
            ref(xb)
            be_times.append(time.perf_counter() - t0)
    return {"y": torch.cat(outs), "t_med": float(np.median(times)), "n_done": len(times), "threads": torch.get_num_threads(),
            "cores_how": how, "be_t_med": float(np.median(be_times)), "be_batch": int(xb.shape[0]), "be_runs": len(be_times)}


def trained_mae_leg(dev, modes, size=512, n=2, steps=300):
    """MAE of the [0,1] output against the fp32 CPU oracle on TRAINED-LIKE weights (VERDICT r03 next #2a): unet_2 from the PyTorch-default-like
    formula init, `steps` AdamW steps of this package's trainer on synthetic cover / stego pairs (trainer.synthetic_pretrain), then `n` unseen
    512x512 images through each mode and through oracle/unet_ref on the host.  The reference ships no UNet checkpoint (.MISSING_LARGE_BLOBS)."""
    import numpy as np
    import torch
    from ws_unet_amd import formula
    from ws_unet_amd.model import get_model
    from ws_unet_amd.trainer import synthetic_pretrain
    from oracle import unet_ref
    m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode=None)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "default").items()})
    m = m.to(dev)
    t0 = time.perf_counter()
    last = synthetic_pretrain(m, steps=steps)
    t_train = time.perf_counter() - t0
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    del m
    u8 = formula.synthetic_images(n, size, size, seed=4242)
    x = torch.from_numpy(u8.astype(np.float32) / np.float32(255.))[:, None]
    ncpu, _ = host_cpus()
    torch.set_num_threads(ncpu)
    with torch.no_grad():
        ref = unet_ref.unet_forward(x.clone(), {k: v.float() for k, v in sd.items()}, 2)
    out = {"weights": f"unet_2, 'default' init + {steps} AdamW steps (L1WS, lr 1e-3) on synthetic 128x128 cover / LSBR pairs, train_mode f16f8p",
           "final_train_loss": last, "train_s": t_train, "images": n, "oracle_output_std": float(ref.std()), "mae": {}}
    for md in modes:
        mm = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode=md)
        mm.load_state_dict(sd)
        mm = mm.to(dev)
        with torch.no_grad():
            y = mm(x.to(dev)).cpu()
        out["mae"][md] = float((y - ref).abs().mean())
        del mm
    return out


def compact_line(result: dict) -> dict:
    """The printed line: the full result minus what only a reader of profiles/ needs (per-layer tables become [layer, ms, frac] triples, long
    notes go, floats keep 5 significant digits) -- the driver's record keeps the last 8 KB of stdout."""
    import copy
    r = copy.deepcopy(result)
    roof = r.get("roofline", {})
    pl = roof.get("per_layer")
    if pl:
        key = "frac_2B" if any("frac_2B" in row for row in pl["layers"]) else "frac"
        roof["per_layer"] = {k: v for k, v in pl.items() if k not in ("layers", "note")}
        roof["per_layer"]["columns"] = ["layer", "ms", key]
        roof["per_layer"]["layers"] = [[row["layer"], row["ms"], row.get(key, row.get("frac"))] for row in pl["layers"]]
    for k in ("note", "traffic_unit"):
        roof.pop(k, None)
    for sub in ("mfma_issue", "mfma_busy", "convt2x2", "fused_up", "all_conv", "whole_forward"):
        if isinstance(roof.get(sub), dict):
            roof[sub].pop("note", None)
    if isinstance(r.get("latency_b1"), dict):
        r["latency_b1"].pop("per_layer", None)
    for k in ("train_step", "train_step_products_f16f8"):
        if isinstance(r.get(k), dict) and "arithmetic" in r[k]:
            r[k]["arithmetic"] = r[k]["arithmetic"].split(":")[0]
    for k in ("cpu_baseline", "cpu_baseline_best_effort"):
        if isinstance(r.get(k), dict):
            r[k].pop("cores_counted", None)

    def rnd(o):
        if isinstance(o, float):
            return float(f"{o:.5g}")
        if isinstance(o, dict):
            return {k: rnd(v) for k, v in o.items()}
        if isinstance(o, list):
            return [rnd(v) for v in o]
        return o
    return rnd(r)


def git_blob_sha1(path: Path) -> str:
    data = path.read_bytes()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def pmc_traffic(args, algorithmic_bytes_per_launch, kernel=None):
    """HBM bytes per conv3x3 launch from the PMC counters.  They cannot be read from inside this process (rocprofv3 has to
    wrap it), so the number comes from the committed summary of two `rocprofv3 --pmc` passes of THIS command (FETCH_SIZE and
    WRITE_SIZE separately, FETCH_SIZE doubled on gfx950; tools/pmc_traffic.py), and only when workload, mode AND the git blob
    hash of the kernel source the counters were collected on match this tree: a changed kernel reports `traffic: null`."""
    out = {"traffic": None, "algorithmic_bytes_per_launch": algorithmic_bytes_per_launch}
    if (args.batch, args.size) != (32, 512):
        return out
    cands = sorted((ROOT / "profiles").glob("r*/pmc_conv3x3_traffic.json"))
    if not cands:
        return out
    with open(cands[-1]) as f:
        pmc = json.load(f)
    src = ROOT / "ws_unet_amd" / "csrc" / pmc.get("kernel_source", "conv3x3.hip")
    here = git_blob_sha1(src) if src.exists() else None
    out["traffic_source"] = str(cands[-1].relative_to(ROOT))
    if pmc.get("mode", "bf16x3") != args.mode:
        out["traffic_note"] = f"summary is for mode {pmc.get('mode')}"
        return out
    if kernel is not None and not str(pmc.get("kernel", "")).startswith(kernel):
        out["traffic_note"] = f"summary is for kernel {pmc.get('kernel')} (this mode runs {kernel}; re-run tools/profile_round.sh)"
        return out
    if pmc.get("kernel_source_blob") != here:
        out["traffic_note"] = (f"stale: counters were collected on {src.name} blob {pmc.get('kernel_source_blob')}, "
                               f"this tree has {here} (re-run tools/profile_round.sh)")
        return out
    out["traffic"] = pmc["traffic_bytes_per_launch"]
    out["traffic_unit"] = "HBM bytes per launch (PMC: 2 x FETCH_SIZE + WRITE_SIZE)"
    return out


def sq_counters(args, ckey="conv3x3_pl"):
    """Matrix-pipe busy fraction of the dominant kernel from the SQ counters (SQ_VALU_MFMA_BUSY_CYCLES / SQ_BUSY_CYCLES; rocprofv3 has to wrap
    the process, so the number comes from the committed summary of tools/profile_sq.sh -> tools/pmc_sq.py --json, and only when the git blob
    of the kernel source it was collected on equals this tree's -- like `traffic`)."""
    if (args.batch, args.size) != (32, 512) or args.mode != DEFAULT_MODE:
        return None
    cands = sorted((ROOT / "profiles").glob("r*/sq_counters.json"))
    if not cands:
        return None
    with open(cands[-1]) as f:
        sq = json.load(f)
    src = ROOT / "ws_unet_amd" / "csrc" / (ckey + ".hip")
    out = {"source": str(cands[-1].relative_to(ROOT))}
    if sq.get("meta", {}).get("kernel_source_blobs", {}).get(ckey + ".hip") != git_blob_sha1(src):
        out["note"] = f"stale: the counters were collected on another revision of {ckey}.hip (re-run tools/profile_sq.sh)"
        return out
    k = sq["kernels"].get(ckey + "_kernel", {}).get("fwd1")
    if k:
        out.update({"mfma_busy": k.get("mfma_busy"), "mfma_busy_time_based": k.get("mfma_busy_t"), "clock_GHz_profiled": k.get("clock_GHz"),
                    "wave_wait_any_share": k.get("sq_wait_any_share"), "wave_wait_inst_share": k.get("sq_wait_inst_any_share"),
                    "wave_active_share": k.get("sq_active_inst_any_share"),
                    "note": f"SQ_VALU_MFMA_BUSY_CYCLES / (32 x SQ_BUSY_CYCLES) over the {ckey} launches of this command under rocprofv3 --pmc "
                            "(product libwsu.so; profiled passes run ~3 % below the un-profiled clock)"})
    return out


def per_layer_roofline(timer, mode):
    """Every launch of the forward against max(t_flop, t_byte) at the vendor peaks ('per layer and as the sum')."""
    rows, t_meas, t_roof, t_roof2 = [], 0.0, 0.0, 0.0
    for name, d in timer.per_layer().items():
        t_flop = d["flops"] / PEAK[mode]
        t_byte = d["bytes"] / HBM_PEAK
        roof = max(t_flop, t_byte)
        t = d["avg_ms"] * 1e-3
        row = {"layer": name, "kernel": d["kernel"], "ms": round(d["avg_ms"], 4), "gflop": round(d["flops"] / 1e9, 1),
               "mbytes": round(d["bytes"] / 1e6, 1), "bound": "mfma" if t_flop >= t_byte else "hbm",
               "roof_ms": round(roof * 1e3, 4), "frac": round(roof / t, 4) if t > 0 else None,
               "tflops": round(d["flops"] / t / 1e12, 1) if t > 0 else None, "hbm_GBps": round(d["bytes"] / t / 1e9, 1) if t > 0 else None}
        if "bytes_2B" in d:                                          # SURVEY 8d's byte model (2 B per element) beside the format's own 3 B
            roof2 = max(t_flop, d["bytes_2B"] / HBM_PEAK)
            row.update({"mbytes_2B": round(d["bytes_2B"] / 1e6, 1), "roof_ms_2B": round(roof2 * 1e3, 4), "frac_2B": round(roof2 / t, 4) if t > 0 else None})
            t_roof2 += roof2
        else:
            t_roof2 += roof
        if "tiles" in d:                                             # persistent kernels: work items against the 256 CUs
            row.update({"tiles": int(d["tiles"]), "steps_per_tile": int(d["steps_per_tile"]), "cu_occupied": round(min(d["tiles"], NUM_CU) / NUM_CU, 3),
                        "tile_waves": round(d["tiles"] / NUM_CU, 2)})
        rows.append(row)
        t_meas += t
        t_roof += roof
    return {"layers": rows, "sum_ms": round(t_meas * 1e3, 4), "sum_roof_ms": round(t_roof * 1e3, 4),
            "frac": round(t_roof / t_meas, 4) if t_meas > 0 else None,
            "sum_roof_ms_2B": round(t_roof2 * 1e3, 4), "frac_2B": round(t_roof2 / t_meas, 4) if t_meas > 0 else None,
            "note": "roof = max(algorithmic FLOPs / dense MFMA peak, algorithmic bytes / 8 TB/s) per launch; bytes = inputs once + "
                    "outputs once + weights in the mode's storage format (3 B per element in 'f16f8p'); the *_2B columns price the same "
                    "traffic at SURVEY 8d's 2 B per element, which lowers the HBM-bound rows"}


def latency_b1_leg(dev, mode, size=512, reps=40, warmup=8):
    """The reference's own call pattern: one image per call (src/unet/evaluate.py:31-52, batch is always 1).  GPU time of a batch-1 forward
    (sum of the launches' HIP-event times), wall time of a synchronised call, and per layer how many of the 256 CUs the persistent grids
    occupy (e31 / e32 of unet_2 at 512x512 have 128 tiles)."""
    import numpy as np
    import torch
    from ws_unet_amd import formula, ops
    u8 = formula.synthetic_images(1, size, size, seed=4242)
    x = ops.u8_to_unit(torch.from_numpy(u8).to(dev))[:, None].contiguous()
    model = build_model(mode, dev)
    with torch.no_grad():
        for _ in range(warmup):
            model(x)
        torch.cuda.synchronize()
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            model(x)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        timer = ops.KernelTimer()
        ops.set_timer(timer)
        for _ in range(reps):
            model(x)
        torch.cuda.synchronize()
        ops.set_timer(None)
        ops.set_layer(None)
        # back-to-back calls without a sync in between: what a caller that queues images gets
        t0 = time.perf_counter()
        for _ in range(reps):
            model(x)
        torch.cuda.synchronize()
        queued = (time.perf_counter() - t0) / reps
    pl = per_layer_roofline(timer, mode)
    gpu_ms = pl["sum_ms"]
    return {"workload": f"unet_2 forward, batch=1, {size}x{size}x1, mode {mode} (the reference's infere_single call pattern)",
            "gpu_ms_per_image": gpu_ms, "wall_ms_per_image_synchronised": float(np.median(walls)) * 1e3, "wall_ms_per_image_queued": queued * 1e3,
            "images_per_s_queued": 1.0 / queued, "launches_per_forward": len(pl["layers"]),
            "tflops_algorithmic": 202.2e9 * (size / 512.0) ** 2 / (gpu_ms * 1e-3) / 1e12,
            "per_layer": [{k: r[k] for k in ("layer", "ms", "tiles", "steps_per_tile", "cu_occupied", "tile_waves", "tflops", "hbm_GBps") if k in r} for r in pl["layers"]]}


def train_step_leg(dev, batch, size, steps=5, warmup=3, train_mode=None, train_products=None):
    """BASELINE.json configs[2]: unet_2 fwd + L1WS + bwd + AdamW on synthetic cover/stego pairs resident in HBM."""
    import numpy as np
    import torch
    from ws_unet_amd import formula, ops
    from ws_unet_amd.model import get_model
    from ws_unet_amd.trainer import Trainer
    m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode="f16f8p")
    if train_mode:
        m.train_mode = train_mode
    if train_products:
        m.train_products = train_products
    m.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "default").items()})
    m = m.to(dev)
    cov = formula.synthetic_images(batch, size, size, seed=5)
    st = np.stack([formula.lsbr_embed(c, 0.4, seed=i) if i % 2 else c for i, c in enumerate(cov)])
    covers = ops.u8_to_unit(torch.from_numpy(cov).to(dev))[:, None].contiguous()
    inputs = ops.u8_to_unit(torch.from_numpy(st).to(dev))[:, None].contiguous()
    alphas = torch.tensor([0.4 if i % 2 else 0.0 for i in range(batch)], device=dev)
    tr = Trainer(m, loss="l1ws", lr=1e-4)
    for _ in range(warmup):
        tr.train_step(inputs, covers, alphas)
    torch.cuda.synchronize()
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    t0 = time.perf_counter()
    for _ in range(steps):
        loss, _ = tr.train_step(inputs, covers, alphas)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ops.set_timer(None)
    ks = timer.summary()
    top = sorted(ks.items(), key=lambda kv: -kv[1]["total_ms"])[:3]
    flop = TRAIN_FLOP_PER_IMAGE_512 * (size / 512.0) ** 2 * batch
    res = {"workload": f"unet_2 fwd + L1WS + bwd + AdamW, batch={batch} synthetic {size}x{size} cover/stego pairs (BASELINE.json configs[2])",
           "arithmetic": (f"train_mode={m.train_mode} train_products={m.train_products}: planar activations (3 bytes per element), fp32 accumulation; "
                          "forward in the f16f8 arithmetic of the predict path; the backward matrix kernels (3x3 and transposed-conv data / weight gradients) multiply "
                          + ("the f16 parts only (exact f16 products; include/wsu.h WSU_PRODUCTS_F16) and gradient tensors hold f16 values (2 bytes per element)"
                             if m.train_products == "f16" else "f16 products + both fp8 residual cross terms; gradient tensors f16 + e4m3 residual (3 bytes per element)")
                          if m.train_mode == "f16f8p"
                          else f"train_mode={m.train_mode} fwd={m.train_fwd_mode} bwd={m.train_bwd_mode} (fp32 storage and accumulation)"),
           "steps": steps, "warmup": warmup, "ms_per_step": dt / steps * 1e3, "images_per_s": batch * steps / dt,
           "tflops_algorithmic": flop * steps / dt / 1e12, "frac_of_mfma_peak": flop * steps / dt / PEAK["bf16x3"],
           "loss": float(loss.item()), "peak_mem_GB": torch.cuda.max_memory_allocated() / 2 ** 30,
           "kernels_ms_per_step": {k: round(v["total_ms"] / steps, 3) for k, v in sorted(ks.items(), key=lambda kv: -kv[1]["total_ms"])},
           "top3": [{"kernel": k, "ms_per_step": round(v["total_ms"] / steps, 3), "share_of_kernel_time": round(v["total_ms"] / max(1e-9, sum(x["total_ms"] for x in ks.values())), 3)}
                    for k, v in top]}
    del tr, m, covers, inputs
    torch.cuda.empty_cache()
    return res


def rehearse(args, rank, world):
    """The launch / rendezvous / barrier / max-over-ranks / rank-0-prints plumbing of the real run on CPU tensors over gloo."""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    dist.barrier()
    t = torch.tensor([time.perf_counter() - t0 + 1e-3 * rank], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(json.dumps({"metric": "rehearsal (no GPU work, not a measurement)", "value": None, "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "max_rank_time_s": t.item(), "gloo_world_size": dist.get_world_size()}))
    dist.destroy_process_group()


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    import numpy as np
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.rehearse:
        return rehearse(args, rank, world)
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback for the product path)"
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit(f"bench.py: rank {rank} needs GPU {local_rank}, {torch.cuda.device_count()} visible")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # Under torch.distributed.run (RANK set) the RCCL process group is always created, also for one rank, so the
    # barrier / max-reduce code below is the same code at every N.
    use_dist = world > 1 or ("RANK" in os.environ and "MASTER_PORT" in os.environ)
    rccl_world = None
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        rccl_world = dist.get_world_size()

    from ws_unet_amd import formula, ops
    # each rank gets its own shard of the synthetic image stream (global index = rank*batch + i)
    u8 = formula.synthetic_images(args.batch, args.size, args.size, seed=1000 + rank)
    x = ops.u8_to_unit(torch.from_numpy(u8).to(dev))[:, None].contiguous()        # (B,1,H,W) fp32 resident in HBM

    model = build_model(args.mode, dev)
    timer = ops.KernelTimer()
    dt, y = timed_steps(model, x, args.steps, args.warmup, use_dist, timer)
    imgs = world * args.batch * args.steps
    value = imgs / dt

    result = None
    if rank == 0:
        ks = timer.summary()
        ckey = next(k for k in ("conv3x3_q", "conv3x3_pl", "conv3x3") if k in ks)     # the 3x3 conv kernel of this mode ('f16f4p': csrc/conv3x3_q.hip)
        conv = ks[ckey]
        achieved = conv["flops"] / (conv["total_ms"] * 1e-3)
        roofline = {
            "bound": "mfma", "kernel": ckey + "_kernel", "achieved": achieved / 1e12, "peak": PEAK[args.mode] / 1e12,
            "unit": "TFLOP/s", "frac": achieved / PEAK[args.mode], "traffic": None,
            "avg_launch_ms": conv["avg_ms"], "launches": conv["launches"],
            "algorithmic_gflop_per_launch": conv["flops"] / conv["launches"] / 1e9,
            "hbm_GBps_algorithmic": conv["bytes"] / (conv["total_ms"] * 1e-3) / 1e9,
            "note": "algorithmic FLOPs = 2*9*Cin*Cout*N*H*W summed over this kernel's conv3x3 launches of a forward (9; 7 when the decoder blocks' first convs run fused with their transposed convs: roofline.fused_up) "
                    "(the split modes issue extra MFMAs per product -- bf16x3: 3 bf16; f16f8: 1 f16 + one fp8 instruction per tap pair -- they are not counted)",
        }
        # matrix-pipe occupancy next to the algorithmic fraction: one unit = one 32x32x16 bf16/f16 MFMA (32 cycles, 32 768 FLOP); per
        # 16-channel chunk and 32x32 output tile a product costs 9 units of work, the modes issue 27 (bf16x3: 3 per tap), 19 (f16f8: 9
        # f16 + 5 fp8 instructions of 2 units), 9 (bf16) -- the fused first layer and the 16x16x32 shape issue the same unit counts
        units = {"bf16x3": 27 / 9, "bf16x3s": 27 / 9, "f16f8": 19 / 9, "f16f8p": 19 / 9, "f16f4p": 14 / 9, "bf16": 1.0}.get(args.mode)       # f16f8q mixes 19 and 15
        if units is not None:
            roofline["mfma_issue"] = {"units_per_product": units, "tflops_equivalent": achieved * units / 1e12,
                                      "frac_of_peak": achieved * units / PEAK[args.mode],
                                      "note": "matrix-pipe time actually issued (split terms included) against the same dense bf16 peak"}
        if "conv3x3_up_q" in ks:
            # the decoder blocks' fused entries (transposed conv + concat + first 3x3 conv in one launch, csrc/conv3x3_qu.hip): priced at the
            # ALGORITHMIC work of the two reference ops they replace (the kernel itself executes 512 instead of 576 + 64 multiply-adds per
            # output and low-resolution channel pair), and the whole 3x3-conv family together
            fu = ks["conv3x3_up_q"]
            ach = fu["flops"] / (fu["total_ms"] * 1e-3)
            roofline["fused_up"] = {"kernel": "conv3x3_qu_kernel", "bound": "mfma", "achieved": ach / 1e12, "peak": PEAK[args.mode] / 1e12, "unit": "TFLOP/s",
                                    "frac": ach / PEAK[args.mode], "avg_launch_ms": fu["avg_ms"], "launches": fu["launches"],
                                    "algorithmic_gflop_per_launch": fu["flops"] / fu["launches"] / 1e9,
                                    "note": "algorithmic FLOPs = nn.ConvTranspose2d(k2,s2) + the 3x3 conv over cat[xu, skip] (unet.py:177-179,183-185), both ops of the reference"}
            tot_f, tot_t = conv["flops"] + fu["flops"], conv["total_ms"] + fu["total_ms"]
            roofline["all_conv"] = {"achieved": tot_f / (tot_t * 1e-3) / 1e12, "frac": tot_f / (tot_t * 1e-3) / PEAK[args.mode], "ms_per_step": tot_t / args.steps,
                                    "note": "conv3x3_q_kernel + conv3x3_qu_kernel launches together"}
        # the whole forward against the same peak: every launch's algorithmic FLOPs (3x3 convs, transposed convs, first layer, head) over the
        # step's wall time -- the number a change of kernel boundaries (fusions) cannot move by re-labelling work
        tot_flops = sum(v["flops"] for v in ks.values())
        roofline["whole_forward"] = {"achieved": tot_flops / dt / 1e12, "frac": tot_flops / dt / PEAK[args.mode], "gflop_per_image": tot_flops / (args.batch * args.steps) / 1e9,
                                     "note": "sum of all launches' algorithmic FLOPs / wall time of the timed steps"}
        roofline.update(pmc_traffic(args, conv["bytes"] / conv["launches"], ckey + "_kernel"))
        busy = sq_counters(args, ckey)
        if busy is not None and "mfma_issue" in roofline:
            roofline["mfma_busy"] = busy
        roofline["per_layer"] = per_layer_roofline(timer, args.mode)
        ctk = "convt2x2_pl" if "convt2x2_pl" in ks else "convt2x2"
        if ctk in ks:
            ct = ks[ctk]
            bw = ct["bytes"] / (ct["total_ms"] * 1e-3)
            roofline["convt2x2"] = {"bound": "hbm", "achieved": bw / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": bw / HBM_PEAK,
                                    "avg_launch_ms": ct["avg_ms"], "launches": ct["launches"],
                                    "note": "transposed 2x2 convs (upconv3, upconv4): algorithmic bytes (input once + 4x-pixel output once + weights) / HIP-event time"}
        gpu_ms = {k: round(v["total_ms"] / args.steps, 3) for k, v in ks.items()}
        result = {
            "metric": "512x512 grayscale images/sec (UNet predict)", "value": value, "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"bf16x3": "bf16x3 (bf16 MFMA on split fp32 operands, fp32 accumulate)",
                      "bf16x3s": "bf16x3 (bf16 MFMA on split fp32 operands, fp32 accumulate; activations stored as their hi/lo halves)",
                      "f16f8": "f16f8 (f16 MFMA on the f16 halves + block-scaled fp8 MFMA on the residual cross terms, fp32 accumulate)",
                      "f16f8p": "f16f8 (f16 MFMA on the f16 halves + block-scaled fp8 MFMA on the residual cross terms, fp32 accumulate; planar storage, LDS-DMA pipeline)",
                      "f16f8q": "f16f8 on planar storage with one cross term on the first conv of each decoder block",
                      "f16f4p": "f16 MFMA on the f16 halves + ONE block-scaled fp4 (e2m1) MFMA per tap pair for both residual cross terms (per-pixel / per-(co, tap) E8M0 scales), fp32 accumulate; planar storage",
                      "bf16": "bf16", "f32": "f32"}[args.mode],
            "data": "synthetic",
            "config": {"workload": f"unet_2 forward-only predict, batch={args.batch}/GPU synthetic {args.size}x{args.size}x1 "
                                   "(BASELINE.json configs[1]), formula 'he' weights, inputs resident in HBM",
                       "mode": args.mode, "global_batch": world * args.batch, "parallelism": f"batch-shard x{world}",
                       "rccl_world_size": rccl_world},
            "roofline": roofline,
            "kernel_ms_per_step": gpu_ms,
        }

    # --full: the legs beyond the headline, each a run of its own after the timed steps (rank 0 only, N = 1 only)
    full = rank == 0 and world == 1 and args.full

    # other precision modes, same process, fewer steps
    if full and not args.no_other_modes:
        other = {}
        for md in [m for m in ("bf16", "f32", "bf16x3", "bf16x3s", "f16f8", "f16f8p", "f16f8q", "f16f4p") if m != args.mode]:
            mm = build_model(md, dev)
            st = max(4, args.steps // 2)
            d2, y2 = timed_steps(mm, x, st, 3, False)                  # 3 warm-up steps: with one, the first timed steps still carried the clock ramp and read 10 % low
            other[md] = {"images_per_s": args.batch * st / d2, "ms_per_step": d2 / st * 1e3, "_y": y2[:4].cpu()}
            del mm
        result["other_modes"] = other

    y_host = y.cpu() if rank == 0 else None
    if rank == 0 and args.dump_outputs:
        result["dumped_outputs"] = dump_outputs(args.dump_outputs, y_host)
    del model, y
    torch.cuda.empty_cache()

    if full and not args.no_latency:
        try:
            result["latency_b1"] = latency_b1_leg(dev, args.mode, args.size)
        except Exception as e:
            result["latency_b1"] = {"error": f"{type(e).__name__}: {e}"}

    if full and not args.no_train_step:
        try:
            result["train_step"] = train_step_leg(dev, args.train_batch, args.size)
            # the same step with the forward's f16f8 arithmetic in the backward matrix kernels too (train_products='f16f8', the round-2 arithmetic)
            r2 = train_step_leg(dev, args.train_batch, args.size, steps=3, warmup=2, train_products="f16f8")
            result["train_step_products_f16f8"] = {k: r2[k] for k in ("arithmetic", "steps", "warmup", "ms_per_step", "images_per_s", "tflops_algorithmic", "loss", "kernels_ms_per_step")}
        except Exception as e:                                       # the headline line must survive (e.g. a smaller card)
            result["train_step"] = {"error": f"{type(e).__name__}: {e}"}

    if full and not args.no_cpu_baseline:
        nsample = 16
        cb = cpu_baseline(u8[:nsample])
        ref_y, n_done = cb["y"], cb["n_done"]
        mae = (y_host[:n_done] - ref_y).abs().mean().item()
        result["cpu_baseline"] = {
            "value": 1.0 / cb["t_med"], "unit": "images/s", "cores": cb["threads"], "kind": "port",
            "sample": f"{n_done} of the same 512x512 images, batch 1 per call, autograd on (reference-faithful "
                      f"infere_single), torch-CPU fp32 restatement of the reference (oracle/unet_ref.py); median {cb['t_med']:.3f} s/image",
            "cores_counted": cb["cores_how"],
        }
        result["cpu_baseline_best_effort"] = {
            "value": cb["be_batch"] / cb["be_t_med"], "unit": "images/s", "cores": cb["threads"], "kind": "port",
            "sample": f"the first {cb['be_batch']} of the same images as ONE batch under torch.no_grad(), same model and threads; "
                      f"median of {cb['be_runs']} runs, {cb['be_t_med']:.3f} s/batch",
        }
        result["mae_vs_cpu_oracle"] = mae
        result["speedup_vs_cpu"] = value / (1.0 / cb["t_med"])
        result["speedup_vs_cpu_best_effort"] = value / (cb["be_batch"] / cb["be_t_med"])
        if "other_modes" in result:
            for md, o in result["other_modes"].items():
                k = min(4, n_done)
                o["mae_vs_cpu_oracle"] = (o.pop("_y")[:k] - ref_y[:k]).abs().mean().item()
    if full and not args.no_trained_mae:
        try:
            tm = trained_mae_leg(dev, [args.mode] + [m for m in ("f16f8p", "f32") if m != args.mode], args.size)
            result["trained_weights"] = tm
            result["mae_vs_cpu_oracle_trained"] = tm["mae"][args.mode]
        except Exception as e:                                       # the headline line must survive
            result["trained_weights"] = {"error": f"{type(e).__name__}: {e}"}
    if rank == 0:
        for o in result.get("other_modes", {}).values():
            o.pop("_y", None)
        if args.detail:
            with open(args.detail, "w") as fh:
                json.dump(result, fh)
        line = json.dumps(compact_line(result))
        if len(line) > 8000:                                         # last resort: the tables that are in --detail anyway
            slim = compact_line(result)
            slim.get("roofline", {}).pop("per_layer", None)
            slim.pop("train_step_products_f16f8", None)
            line = json.dumps(slim)
        print(line)
    if use_dist:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
