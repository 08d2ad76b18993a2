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

from . import embed

METHODS = ("LSBM", "HILL")
ALPHA_RANGE = {"LSBM": "[0, 1]", "HILL": "[0, log2 3)"}             # of embed.ALPHA_RANGES


def method_name(stego_method: str) -> str:
    """'LSBM' / 'HILL', matched case-insensitively."""
    m = str(stego_method).upper()
    if m not in METHODS:
        raise NotImplementedError(f"stego method {stego_method!r} is not a +-1 simulator here: choose one of {' / '.join(METHODS)}")
    return m


def simulate(cover_u8: torch.Tensor, stego_method: str, alpha, seeds, *, rho: typing.Optional[torch.Tensor] = None):
    """cover_u8: (N,H,W) uint8 on the device; alpha: bits per pixel, a scalar or one value per image; seeds: one 64-bit integer per image
    (embed.image_seed) -> (stego (N,H,W) uint8, changes (N) int64), both on the device.  'HILL' takes an optional `rho` =
    ops.hill_cost_f64(cover_u8) made earlier (several alphas of the same covers), reads back one flag per image and raises ValueError
    naming the images whose capacity is short of alpha H W bits; alpha == 0 gives the cover."""
    from . import ops
    method = method_name(stego_method)
    n, h, w = embed.planes_shape("simulate", cover_u8)
    a = embed.alpha_values(alpha, ALPHA_RANGE[method], n, whose=f" for {method!r}")
    dev = cover_u8.device
    seeds_dev = embed.seeds_tensor("simulate", seeds, n, dev, method)
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
    """`stego_<METHOD>_alpha_<a>_independent_images` (embed.twin_folder)."""
    return embed.twin_folder(method_name(stego_method), alpha)


def write_dataset(data_dir, stego_method: str, alpha, *, split: typing.Optional[str] = None, stream: int = 0) -> typing.List[pathlib.Path]:
    """Twins of every cover of `data_dir` (images*/files.csv, or the rows of `split`) at `alpha` (one value or several), written beside
    the covers; returns the folders.  A folder's files.csv lists exactly the files of this call."""
    from . import ops
    method = method_name(stego_method)

    def make(cover, a, seeds, rho):
        return simulate(cover, method, a, seeds, rho=rho)[0], {}

    return embed.write_twins(data_dir, method, embed.payload_list(ALPHA_RANGE[method], alpha, whose=f" for {method!r}"), make,
                             prepare=ops.hill_cost_f64 if method == "HILL" else None, split=split, stream=stream)


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
