"""+-1 embedding simulators on the device: LSBM and HILL twins of cover images (wsu_ternary_entropy, wsu_embed_ternary, wsu_embed_lsbm;
include/wsu.h K37-K39).  Not part of the reference, and separate from `embed`, whose five methods all flip LSBs.

  * `simulate(cover_u8, stego_method, alpha, seeds)` on resident (N,H,W) uint8 planes;
  * `write_dataset(data_dir, stego_method, alpha)` / `python -m ws_unet_amd.embed_pm1 --data DIR --stego-method HILL --alphas .4 .2`
    writes `stego_<METHOD>_alpha_<a>_independent_images/<stem>.png` and its files.csv beside the covers, as embed.write_dataset does;
  * `spam.extract(..., simulate=True)` makes these twins of the uploaded covers.

LSBM is LSB matching (T. Sharp, "An implementation of key-based digital signal steganography", IH 2001): a message of alpha bits per pixel
changes a fraction alpha / 2 of the pixels by +1 or -1, the sign random, inwards at 0 and 255; alpha in [0, 1].  Its realisation is a
function of (seed, alpha, pixel index, whether the pixel is 0 or 255) alone.

HILL is the payload-limited sender (T. Filler, J. Fridrich, "Gibbs construction in steganography", IEEE TIFS 5(4), 2010) over the HILL cost
(B. Li, M. Wang, J. Huang, X. Li, ICIP 2014; ops.hill_cost_f64): pixel i changes by +1 and by -1 with probability exp(-lambda rho_i) / Z_i
each, and lambda is solved per image so that the entropy of the changes is the payload m = alpha H W bits (ops.ternary_lambda); alpha in
[0, log2 3).  The lower end of the bracket is used, so the capacity is never short of the payload.  This simulates optimal coding; no
syndrome-trellis code is run.

Not checked: no run was compared with another implementation (conseal, stegolab: neither is at hand).  Making the +1 change wet at 255
and the -1 change wet at 0, and taking the costs from the cover alone with the same cost for both directions, is the common convention
as remembered.
"""
from __future__ import annotations

import argparse
import math
import pathlib
import typing

import numpy as np
import torch

from . import embed, fabrika

METHODS = ("LSBM", "HILL")
ALPHA_MAX = {"LSBM": 1.0, "HILL": math.log2(3.0)}                   # HILL: below it; LSBM: up to it


def method_name(stego_method: str) -> str:
    """'LSBM' / 'HILL', matched case-insensitively."""
    m = str(stego_method).upper()
    if m not in METHODS:
        raise NotImplementedError(f"stego method {stego_method!r} is not a +-1 simulator here: choose one of {' / '.join(METHODS)}")
    return m


def _alphas(method: str, alpha, n: int) -> np.ndarray:
    a = np.asarray(alpha, dtype=np.float64)
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
        raise ValueError(f"alpha must be a scalar or one value per image ({n}), got shape {a.shape}")
    a = np.broadcast_to(a, (n,))
    top = ALPHA_MAX[method]
    if not np.all((a >= 0) & ((a <= top) if method == "LSBM" else (a < top))):
        raise ValueError(f"alpha outside {'[0, 1]' if method == 'LSBM' else '[0, log2 3)'} for {method!r}: {alpha!r}")
    return a


def simulate(cover_u8: torch.Tensor, stego_method: str, alpha, seeds, *, rho: typing.Optional[torch.Tensor] = None):
    """cover_u8: (N,H,W) uint8 on the device; alpha: bits per pixel, a scalar or one value per image; seeds: one 64-bit integer per image
    (embed.image_seed) -> (stego (N,H,W) uint8, changes (N) int64), both on the device.  'HILL' takes an optional `rho` =
    ops.hill_cost_f64(cover_u8) made earlier (several alphas of the same covers), reads back one flag per image and raises ValueError
    naming the images whose capacity is short of alpha H W bits; alpha == 0 gives the cover."""
    from . import ops
    method = method_name(stego_method)
    if not (isinstance(cover_u8, torch.Tensor) and cover_u8.dim() == 3 and cover_u8.dtype == torch.uint8):
        raise ValueError("simulate: cover_u8 must be an (N,H,W) uint8 tensor")
    n, h, w = cover_u8.shape
    a = _alphas(method, alpha, n)
    if seeds is None:
        raise ValueError(f"simulate: {method!r} needs one seed per image (embed.image_seed)")
    s = np.array([int(v) % 2 ** 64 for v in (seeds.tolist() if isinstance(seeds, (torch.Tensor, np.ndarray)) else seeds)], dtype=np.uint64)
    if s.shape != (n,):
        raise ValueError(f"simulate: {s.shape[0] if s.ndim else 1} seeds for {n} images")
    dev = cover_u8.device
    seeds_dev = torch.from_numpy(s.view(np.int64)).to(dev)
    if method == "LSBM":
        t = np.array([ops.lsbm_threshold(v) for v in a], dtype=np.uint32)
        return ops.embed_lsbm(cover_u8, seeds_dev, torch.from_numpy(t.view(np.int32)).to(dev))
    if rho is None:
        rho = ops.hill_cost_f64(cover_u8)
    m = torch.from_numpy(a * np.float64(h * w)).to(dev)
    lam, _, ok = ops.ternary_lambda(cover_u8, rho, m)
    short = np.nonzero(~ok.cpu().numpy())[0]
    if short.size:
        raise ValueError(f"simulate: 'HILL' cannot carry the payload in image(s) {short.tolist()} of the batch: alpha {a[short].tolist()} "
                         f"exceeds their capacity (log2 3 bits per pixel at most, 1 bit for a pixel at 0 or 255)")
    lam = torch.where(m > 0, lam, torch.full_like(lam, math.inf))           # no payload: no change, whatever the costs
    return ops.embed_ternary(cover_u8, rho, lam, seeds_dev)


# ---- whole data sets --------------------------------------------------------------------------------------------------------

def folder_name(stego_method: str, alpha: float) -> str:
    """`stego_<METHOD>_alpha_<a>_independent_images`, embed.folder_name's scheme."""
    return f"stego_{method_name(stego_method)}_alpha_{float(alpha)}_independent_images"


def _write_chunk(fnames, kws, *, stego_method, alphas, stream, out_dir, prefetched=None):
    """One chunk of covers -> their twins at every alpha, written as 8-bit gray PNGs; one list of files.csv rows per cover."""
    from PIL import Image
    from . import ops
    planes = prefetched[0] if prefetched is not None else embed._prefetch(fnames, kws)[0]
    cover = torch.from_numpy(np.ascontiguousarray(planes)).to("cuda")
    method = method_name(stego_method)
    rho = ops.hill_cost_f64(cover) if method == "HILL" else None
    seeds = [embed.image_seed(f, stream) for f in fnames]
    rows = [[] for _ in fnames]
    for a in alphas:
        try:
            stego = simulate(cover, method, a, seeds, rho=rho)[0].cpu().numpy()
        except ValueError as e:
            raise ValueError(f"{e} (the batch: {[pathlib.Path(f).name for f in fnames]})") from e
        folder = folder_name(method, a)
        (pathlib.Path(out_dir) / folder).mkdir(parents=True, exist_ok=True)
        for i, f in enumerate(fnames):
            name = f"{folder}/{pathlib.Path(f).stem}.png"
            Image.fromarray(stego[i]).save(pathlib.Path(out_dir) / name)
            rows[i].append({"name": name, "height": stego.shape[1], "width": stego.shape[2], "stego_method": method, "alpha": float(a)})
    return rows


_write_covers = fabrika.precovers(iterator="batched", convert_to=None, ignore_missing=True)(
    fabrika.shared_kwargs(_write_chunk, ("stego_method", "alphas", "stream", "out_dir"), embed._prefetch))


def write_dataset(data_dir, stego_method: str, alpha, *, split: typing.Optional[str] = None, stream: int = 0) -> typing.List[pathlib.Path]:
    """Twins of every cover of `data_dir` (images*/files.csv, or the rows of `split`) at `alpha` (one value or several), written beside
    the covers; returns the folders.  A folder's files.csv lists exactly the files of this call."""
    import pandas as pd
    data_dir = pathlib.Path(data_dir)
    method = method_name(stego_method)
    alphas = [float(a) for a in np.atleast_1d(np.asarray(alpha, dtype=np.float64))]
    _alphas(method, alphas, len(alphas))
    rows = _write_covers(data_dir, split=split, stego_method=method, alphas=alphas, stream=int(stream), out_dir=str(data_dir))
    folders = []
    for j, a in enumerate(alphas):
        folder = data_dir / folder_name(method, a)
        pd.DataFrame([r[j] for r in rows], columns=["name", "height", "width", "stego_method", "alpha"]).to_csv(folder / "files.csv", index=False)
        folders.append(folder)
    return folders


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Write simulated +-1 stego twins of a data set's covers (LSBM / HILL, made on the GPU).")
    ap.add_argument("--data", required=True, help="data set directory (images*/files.csv)")
    ap.add_argument("--stego-method", required=True, help=" / ".join(METHODS))
    ap.add_argument("--alphas", type=float, nargs="+", required=True, help="payloads in bits per pixel: LSBM [0, 1], HILL [0, log2 3)")
    ap.add_argument("--split", default=None, help="a split CSV of the data set: only its covers")
    ap.add_argument("--stream", type=int, default=0, help="realisation number (embed.image_seed)")
    ns = ap.parse_args(argv)
    for folder in write_dataset(ns.data, ns.stego_method, ns.alphas, split=ns.split, stream=ns.stream):
        print(folder)


if __name__ == "__main__":
    main()
