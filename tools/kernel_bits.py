"""Bit-level record of the matrix kernels through the model: SHA-256 of the unet_2 forward output in every precision mode, of the default
mode under each kernel-organisation switch, and of the flat gradient and parameter buffers after one train step per training arithmetic.
Fixed seeds; every case runs in a fresh child process (the library and the model read their switches once).

  python tools/kernel_bits.py OUT.json          run every case and write {case: sha256}
  python tools/kernel_bits.py --compare A B     cases side by side; exit status 1 unless every hash is equal

Two builds of libwsu are compared by running the first form twice, once with WSU_LIB pointing at the other build (the Python package is
the same, the C ABI decides what is compared).  profiles/r13 has such a pair."""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FORWARD_MODES = ("f16f4p", "f16f8p", "f16p", "f16f8", "bf16x3", "bf16x3s", "bf16", "f32")
SWITCHES = ("WSU_FUSE_UP=0", "WSU_FUSE_FIRST_Q=1", "WSU_Q_ROWS=4", "WSU_PL_MSPLIT=0")
TRAIN = (("f16f8p", "f16"), ("f16f8p", "f16f8"), ("bf16x3", None), ("f32", None))
# (batch, h, w): a grid smaller than the device (the half-block work items of the planar kernels) with partial edge tiles, and one larger than it
SHAPES = ((3, 72, 100), (2, 256, 320))
CASES = [f"fwd {m}" for m in FORWARD_MODES] + [f"fwd f16f4p {s}" for s in SWITCHES] + [f"train {m} {p or '-'}" for m, p in TRAIN]


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(case: str) -> dict:
    import numpy as np
    import torch
    from ws_unet_amd import formula, ops
    from ws_unet_amd.model import get_model
    dev, out = torch.device("cuda"), {}
    kind, mode = case.split()[:2]
    sd = {k: torch.from_numpy(v) for k, v in formula.formula_state_dict(2, "default").items()}
    if kind == "fwd":
        m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode=mode)
        m.load_state_dict(sd)
        m = m.to(dev)
        for n, h, w in SHAPES:
            x = ops.u8_to_unit(torch.from_numpy(formula.synthetic_images(n, h, w, seed=21)).to(dev))[:, None].contiguous()
            with torch.no_grad():
                out[f"{case} {n}x{h}x{w}"] = sha(m(x))
    else:
        from ws_unet_amd.trainer import Trainer
        products = case.split()[2]
        m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode="f32" if mode == "f32" else "f16f8p")
        m.load_state_dict(sd)
        m = m.to(dev)
        m.train_mode = mode
        if products != "-":
            m.train_products = products
        n, h, w = 4, 128, 160
        cov = formula.synthetic_images(n, h, w, seed=5)
        st = np.stack([formula.lsbr_embed(c, 0.4, seed=i) if i % 2 else c for i, c in enumerate(cov)])
        covers = ops.u8_to_unit(torch.from_numpy(cov).to(dev))[:, None].contiguous()
        inputs = ops.u8_to_unit(torch.from_numpy(st).to(dev))[:, None].contiguous()
        alphas = torch.tensor([0.4 if i % 2 else 0.0 for i in range(n)], device=dev)
        tr = Trainer(m, loss="l1ws", lr=1e-4)
        tr.train_step(inputs, covers, alphas)
        out[f"{case} flat_grad"] = sha(tr.opt.flat_grad)
        out[f"{case} flat_param"] = sha(tr.opt.flat_param)
    torch.cuda.synchronize()
    return out


def main(out_path) -> None:
    rows = {}
    for case in CASES:
        env = dict(os.environ)
        for tok in case.split():
            if "=" in tok:
                k, v = tok.split("=")
                env[k] = v
        r = subprocess.run([sys.executable, __file__, "--case", case], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:                                     # nothing more is started on the GPU after a failed case
            sys.exit(f"case {case!r} failed with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
        rows.update(json.loads(r.stdout.strip().splitlines()[-1]))
        print(case, "ok", flush=True)
    Path(out_path).write_text(json.dumps(rows, indent=0) + "\n")
    print(f"{len(rows)} rows -> {out_path}")


def compare(path_a, path_b) -> int:
    a, b = json.loads(Path(path_a).read_text()), json.loads(Path(path_b).read_text())
    assert list(a) == list(b), "the two files hold different rows"
    for row in a:
        print(f"{row:52s} {'equal' if a[row] == b[row] else 'DIFFERENT'}")
    return 0 if a == b else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        print(json.dumps(run_case(sys.argv[2])))
    elif len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) == 2:
        main(sys.argv[1])
    else:
        sys.exit(__doc__)
