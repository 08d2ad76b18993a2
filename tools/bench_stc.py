"""Time the syndrome-trellis kernels (K40-K42) on one GPU and measure the coding loss of the code, print one JSON line.

  * (a) on --batch and on --big resident 512x512 cover planes (the five fixture covers tiled) and on one plane alone, at --alpha and constraint heights
    7 and 10, along the keyed path with the 'pm1' change: ms per call between HIP events around --inner calls back to back, median of
    --reps such samples after warm-up, of K41's forward pass (ops.stc_embed phases=1), its walk back (phases=2) and K42; of the keyed path
    (K40 + torch.sort); and of stc.embed whole (cost K20 + path + K41 + one read-back of the flags).  Per image: the call / the batch.
  * (b) the coding loss on the five fixture covers at alpha 0.4 / 0.2 / 0.1 over the HILL cost: the STC's cost D (K41's `cost`: the sum of
    the changed pixels' costs) against the expected cost D* of the binary payload-limited sender at the same payload (flip probabilities
    exp(-lambda rho) / (1 + exp(-lambda rho)), lambda by a float64 bisection on the host until the entropy is alpha H W bits): D / D* - 1,
    and the changes per pixel of both.  Nothing is gated on these figures.
Usage: python tools/bench_stc.py [--batch 32] [--reps 7] [--inner 1] [--alpha 0.4] [--heights 7 10] [--big 256]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from ws_unet_amd import embed, ops, stc
from ws_unet_amd.imread import imread4_u8

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--big", type=int, default=256, help="a second batch size: one workgroup per compute unit (0: skip)")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=1)
ap.add_argument("--alpha", type=float, default=0.4)
ap.add_argument("--heights", type=int, nargs="+", default=[7, 10])
a = ap.parse_args()
gold = ROOT / "tests" / "golden"
dev = torch.device("cuda")
covers = np.stack([np.ascontiguousarray(imread4_u8(gold / f"cover_{k}.png")[..., 3]) for k in (6, 7, 8, 9, 10)])
n = a.batch
x = torch.from_numpy(covers[np.arange(max(n, a.big)) % 5].copy()).to(dev)
nmax, hh, ww = x.shape
hw = hh * ww
seed_list = [embed.image_seed(f"{i}.png") for i in range(nmax)]
seeds = torch.tensor(seed_list, dtype=torch.int64, device=dev)


def sample_ms(fn):
    """median, p10, p90 of the time of one call, from --reps samples of --inner calls back to back"""
    for _ in range(2):
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
    return [round(float(v), 4) for v in (np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90))]


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------
rho = ops.hill_cost_f64(x)
path = stc.key_path(seeds, hh, ww, dev)
k = int(round(a.alpha * hw))
msg = stc.random_message(seed_list, k, dev)
lib = ops._lib.load()
timing = {"keyed_path_k40_and_sort": sample_ms(lambda: stc.key_path(seeds[:n], hh, ww, dev)), "cost_f64_k20": sample_ms(lambda: ops.hill_cost_f64(x[:n]))}
for h in a.heights:
    cols = torch.from_numpy(stc.columns(h, -(-hw // k)).view(np.int32)).to(dev)
    for nb in sorted({1, n, nmax}):
        ws = torch.empty(nb * ops.stc_workspace_bytes(hw, h), dtype=torch.uint8, device=dev)
        args = (x[:nb], rho[:nb], msg[:nb], cols, seeds[:nb])
        kw = dict(h=h, path=path[:nb], change="pm1", workspace=ws)
        stego, cost, changes, ok = ops.stc_embed(*args, **kw)
        assert bool(ok.all()) and torch.equal(ops.stc_extract(stego, cols, k, h=h, path=path[:nb]), msg[:nb])
        out_stego, out_changes = torch.empty_like(stego), torch.empty_like(changes)

        def backward():                                                   # phase 2 alone, on the costs and take bits of the call above
            ops.check(lib.wsu_stc_embed(x.data_ptr(), rho.data_ptr(), msg.data_ptr(), cols.data_ptr(), path.data_ptr(), seeds.data_ptr(), 1, h, k,
                                        2, out_stego.data_ptr(), cost.data_ptr(), out_changes.data_ptr(), ok.data_ptr(), ws.data_ptr(),
                                        ws.numel(), nb, hh, ww, ops._stream()), "wsu_stc_embed")
        f = sample_ms(lambda: ops.stc_embed(*args, **kw, phases=1))
        b = sample_ms(backward)
        assert torch.equal(out_stego, stego) and torch.equal(out_changes, changes)
        e = sample_ms(lambda: ops.stc_extract(stego, cols, k, h=h, path=path[:nb]))
        whole = sample_ms(lambda: stc.embed(x[:nb], msg[:nb], seeds=seed_list[:nb], h=h, change="pm1", workspace_cap=ws.numel()))
        timing[f"h{h}_batch{nb}"] = {"forward_ms": f, "backward_ms": b, "extract_ms": e, "stc_embed_whole_ms": whole,
                                    "forward_ms_per_image": round(f[0] / nb, 4), "backward_ms_per_image": round(b[0] / nb, 4),
                                    "forward_ns_per_position": round(f[0] * 1e6 / hw, 2) if nb == 1 else None,
                                    "workspace_mib": ws.numel() >> 20, "changes_per_pixel": round(float(changes.double().mean()) / hw, 5)}
        del ws


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------
def binary_sender(r, bits):
    """(expected cost, expected changes) of the sender that flips pixel i with probability exp(-lam r_i) / (1 + exp(-lam r_i)), lam such
    that the entropy of the flips is `bits`: float64 bisection of log2(lam)"""
    r = r.reshape(-1)

    def at(lam):
        t = lam * r
        e = np.exp(-t)
        p = e / (1.0 + e)
        hbits = (np.log1p(e) + np.where(e > 0, t * e, 0.0) / (1.0 + e)) / np.log(2.0)
        return hbits.sum(), (p * r).sum(), p.sum()
    lo, hi = -60.0, 40.0
    for _ in range(80):
        mid = (lo + hi) / 2
        if at(2.0 ** mid)[0] >= bits:
            lo = mid
        else:
            hi = mid
    return at(2.0 ** lo)


x5 = torch.from_numpy(covers).to(dev)
rho5 = ops.hill_cost_f64(x5)
rho5_np = rho5.cpu().numpy()
seeds5 = [embed.image_seed(f"{c}.png") for c in (6, 7, 8, 9, 10)]
loss = {}
for alpha in (0.4, 0.2, 0.1):
    bits = int(round(alpha * hw))
    opt = [binary_sender(rho5_np[i], bits) for i in range(5)]
    row = {"bits": bits, "binary_sender_cost": [round(float(o[1]), 3) for o in opt],
           "binary_sender_changes_per_pixel": round(float(np.mean([o[2] for o in opt])) / hw, 5)}
    for h in a.heights:
        _, changes, cost, ok = stc.embed(x5, alpha, rho=rho5, h=h, seeds=seeds5)
        assert bool(ok.all())
        ratio = cost.cpu().numpy() / np.array([o[1] for o in opt])
        row[f"h{h}"] = {"stc_cost": [round(float(v), 3) for v in cost.tolist()], "coding_loss_per_image": [round(float(v - 1), 4) for v in ratio],
                        "coding_loss_mean": round(float(ratio.mean() - 1), 4), "changes_per_pixel": round(float(changes.double().mean()) / hw, 5),
                        "bits_per_change": round(bits / float(changes.double().mean()), 3)}
    loss[f"alpha_{alpha}"] = row
print(json.dumps({"batch": n, "alpha": a.alpha, "ms_median_p10_p90": timing, "coding_loss_hill_cost_5_covers": loss}))
