"""Inference modes side by side in ONE process -- python tools/bench_modes.py [--modes f16f4p,f16p,bf16] [--rounds 2] [--window 3] [--out file.json]
bench.py's configuration (unet_2, batch 32 at 512x512, the 'he' formula weights, inputs resident in HBM); the modes take turns, round by round, each
with a warm-up and a timed window of at least `--window` seconds, so that clock and thermal drift hit them alike.  Per mode: images/s and ms per
step (median over the rounds, and every round), per-layer kernel ms (ops.KernelTimer over a few extra steps), the 3x3-conv fraction of the 2.5 PF
dense peak (algorithmic FLOPs of the 3x3 convs and of the fused decoder entries over their kernel time) and the MAE of the [0,1] output against
oracle.unet_ref on 2 images.  Prints one JSON document."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from ws_unet_amd import formula, ops  # noqa: E402
from ws_unet_amd.model import get_model  # noqa: E402

PEAK = 2.5e15                      # dense f16 / bf16 MFMA peak of the MI355X (MI355X_MICROARCH.md), as bench.py
CONV_KERNELS = ("conv3x3_q", "conv3x3_up_q", "conv3x3_h", "conv3x3_up_h", "conv3x3")      # KernelTimer names of the 3x3-conv families


def build(mode, dev):
    m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode=mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "he").items()})
    return m.to(dev)


def window(model, x, warmup, seconds):
    with torch.no_grad():
        for _ in range(warmup):
            model(x)
        torch.cuda.synchronize()
        steps, t0 = 0, time.perf_counter()
        while True:
            model(x)
            steps += 1
            if steps % 4 == 0:
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= seconds:
                    return steps, dt


def per_layer(model, x, steps=3):
    timer = ops.KernelTimer()
    with torch.no_grad():
        model(x)
        torch.cuda.synchronize()
        ops.set_timer(timer)
        for _ in range(steps):
            model(x)
        torch.cuda.synchronize()
        ops.set_timer(None)
        ops.set_layer(None)
    layers = {k: round(v["avg_ms"], 4) for k, v in timer.per_layer().items()}
    ks = timer.summary()
    conv = [ks[k] for k in CONV_KERNELS if k in ks]
    flops, ms = sum(c["flops"] for c in conv), sum(c["total_ms"] for c in conv)
    return {"layers_ms": layers, "kernels_ms_per_step": {k: round(v["total_ms"] / steps, 4) for k, v in ks.items()},
            "conv3x3_ms_per_step": round(ms / steps, 4), "conv3x3_frac_of_peak": round(flops / (ms * 1e-3) / PEAK, 4) if ms > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="f16f4p,f16p,bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.window >= 3.0, "timed windows of at least 3 s"
    dev = torch.device("cuda:0")
    modes = args.modes.split(",")
    u8 = formula.synthetic_images(args.batch, args.size, args.size, seed=1000)
    x = ops.u8_to_unit(torch.from_numpy(u8).to(dev))[:, None].contiguous()          # resident in HBM, as bench.py
    models = {md: build(md, dev) for md in modes}
    rounds = {md: [] for md in modes}
    for _ in range(args.rounds):
        for md in modes:
            steps, dt = window(models[md], x, args.warmup, args.window)
            rounds[md].append({"steps": steps, "s": round(dt, 3), "images_per_s": round(args.batch * steps / dt, 1)})
    from oracle import unet_ref
    xs = x[:2].cpu()
    with torch.no_grad():
        ref = unet_ref.unet_forward(xs.clone(), unet_ref.to_torch_state(formula.formula_state_dict(2, "he")), 2)
    result = {"config": {"model": "unet_2", "weights": "he", "batch": args.batch, "size": args.size, "rounds": args.rounds,
                         "warmup": args.warmup, "window_s": args.window, "device": torch.cuda.get_device_name(0)}, "modes": {}}
    for md in modes:
        ips = statistics.median(r["images_per_s"] for r in rounds[md])
        with torch.no_grad():
            y = models[md](x[:2]).cpu()
        result["modes"][md] = {"images_per_s": round(ips, 1), "ms_per_step": round(args.batch / ips * 1e3, 3), "rounds": rounds[md],
                               **per_layer(models[md], x), "mae_vs_oracle_2img": float((y.double() - ref.double()).abs().mean()),
                               "mode_after": models[md].mode}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
