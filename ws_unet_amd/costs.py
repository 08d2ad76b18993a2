"""S-UNIWARD and WOW on the device: the two wavelet costs beside HILL (wsu_wavelet_cost_f64; include/wsu.h K48), the simulated ternary
sender over them and a real message under them.  Not part of the reference, and a module of its own: `embed_pm1`, `stc` and `stc_ml`
keep their methods, which all use the HILL cost.

  * `cost_map(cover_u8, 'HILL' | 'SUNIWARD' | 'WOW')`: the (N,H,W) float64 cost plane of resident uint8 planes;
  * `simulate(cover_u8, 'SUNIWARD' | 'WOW', alpha, seeds)`: embed_pm1's payload-limited +-1 sender over that cost (ops.ternary_lambda,
    ops.embed_ternary; alpha in [0, log2 3));
  * `embed(cover_u8, 'SUNIWARDT' | 'WOWT', message, seeds=...)` / `extract(stego_u8, layers, seeds=...)`: stc_ml's two-layer
    syndrome-trellis code under that cost; the receiver needs no cost;
  * `write_dataset` / `extract_dataset` and `python -m ws_unet_amd.costs embed --data DIR --stego-method WOW --alphas .4 .2` (or
    `--stego-method WOWT --message FILE`) / `... extract --data DIR --stego-method WOWT --alpha A --out DIR2` write and read
    `stego_<METHOD>_alpha_<a>_independent_images` beside the covers, as the sibling modules do; the `...T` folders' files.csv has
    stc_ml's columns `bits_high` and `bits_low`.

S-UNIWARD is V. Holub, J. Fridrich, T. Denemark, "Universal distortion function for steganography in an arbitrary domain", EURASIP JIS
2014; WOW is V. Holub, J. Fridrich, "Designing steganographic distortion using directional filters", WIFS 2012.  Both filter the cover
with the three directional Daubechies-8 kernels, weigh each coefficient (1 / (|W| + sigma), resp. |W|), project the weights back with
the absolute kernels, and merge the three bands (their sum, resp. the sum of their reciprocals).  include/wsu.h gives the exact
definition and tests/costs_np.py restates it in numpy; the kernel equals the restatement bit for bit.

Not checked: no run was compared with another implementation (the authors' MATLAB, conseal, pywt, stegolab: none is at hand).  The
clamps (1e8, 1e10), the pad of 16, sigma = 1 and the alignment of the two filter passes are the published code as remembered; the
alignment is pinned only by the identity rho[i,j] = D(X, X +- e_ij) of UNIWARD (tests/test_costs_host.py).
"""
from __future__ import annotations

import math
import pathlib
import typing

import numpy as np
import torch

from . import embed as _embed
from . import stc, stc_ml

# The Daubechies-8 orthonormal scaling filter, minimum phase (tools/db8_taps.py derives it and rounds it so that the float64 values' eight
# moments vanish to 2.4e-13; csrc/wavelet_cost.hip holds the same literals)
DB8 = (
    0.054415842243104008, 0.31287159091429984, 0.67563073629728998, 0.58535468365420684,
    -0.015829105256349302, -0.28401554296154691, 0.00047248457391328307, 0.12874742662047847,
    -0.017369301001807547, -0.044088253930794755, 0.013981027917398282, 0.0087460940474057766,
    -0.0048703529934515741, -0.00039174037337694705, 0.00067544940645056922, -0.00011747678412476953)

COSTS = ("HILL", "SUNIWARD", "WOW")
METHODS = ("SUNIWARD", "WOW", "SUNIWARDT", "WOWT")
SIMULATED = METHODS[:2]                                              # the ternary sender is simulated; the other two carry a message
ALPHA_RANGE = {"SUNIWARD": "[0, log2 3)", "WOW": "[0, log2 3)", "SUNIWARDT": "(0, log2 3)", "WOWT": "(0, log2 3)"}


def cost_name(name: str) -> str:
    """'HILL' / 'SUNIWARD' / 'WOW', matched case-insensitively."""
    c = str(name).upper()
    if c not in COSTS:
        raise NotImplementedError(f"cost {name!r} is not built here: choose one of {' / '.join(COSTS)}")
    return c


def method_name(stego_method: str) -> str:
    """'SUNIWARD' / 'WOW' / 'SUNIWARDT' / 'WOWT', matched case-insensitively."""
    m = str(stego_method).upper()
    if m not in METHODS:
        raise NotImplementedError(f"stego method {stego_method!r} is not an embedder over a wavelet cost here: choose one of {' / '.join(METHODS)}")
    return m


def method_cost(stego_method: str) -> str:
    """The cost of a method: 'SUNIWARD' or 'WOW'."""
    m = method_name(stego_method)
    return m[:-1] if m.endswith("T") else m


def cost_map(cover_u8: torch.Tensor, name: str, **params) -> torch.Tensor:
    """cover_u8: (N,H,W) uint8 on the device -> its (N,H,W) float64 cost plane.  params: `clamp` for every cost, `sigma` for 'SUNIWARD'."""
    from . import ops
    c = cost_name(name)
    if c == "HILL":
        return ops.hill_cost_f64(cover_u8, **params)
    return ops.wavelet_cost_f64(cover_u8, c.lower(), **params)


def simulate(cover_u8: torch.Tensor, stego_method: str, alpha, seeds, *, rho: typing.Optional[torch.Tensor] = None, **params):
    """cover_u8: (N,H,W) uint8 on the device; stego_method 'SUNIWARD' or 'WOW'; alpha: bits per pixel in [0, log2 3), a scalar or one
    value per image; seeds: one 64-bit integer per image (embed.image_seed) -> (stego (N,H,W) uint8, changes (N) int64), both on the
    device: embed_pm1's payload-limited sender over `rho` = cost_map(cover_u8, the method's cost, **params) (made here when None).
    Raises ValueError naming the images whose capacity is short of alpha H W bits; alpha == 0 gives the cover."""
    from . import ops
    method = method_name(stego_method)
    if method not in SIMULATED:
        raise NotImplementedError(f"{method!r} carries a real message: use embed")
    n, h, w = _embed.planes_shape("simulate", cover_u8)
    a = _embed.alpha_values(alpha, ALPHA_RANGE[method], n, whose=f" for {method!r}")
    dev = cover_u8.device
    seeds_dev = _embed.seeds_tensor("simulate", seeds, n, dev, method)
    if rho is None:
        rho = cost_map(cover_u8, method, **params)
    m = torch.from_numpy(a * np.float64(h * w)).to(dev)
    lam, _, ok = ops.ternary_lambda(cover_u8, rho, m)
    short = np.nonzero(~ok.cpu().numpy())[0]
    if short.size:
        raise ValueError(f"simulate: {method!r} cannot carry the payload in image(s) {short.tolist()} of the batch: alpha {a[short].tolist()} "
                         f"exceeds their capacity (log2 3 bits per pixel at most, 1 bit for a pixel at 0 or 255)")
    lam = torch.where(m > 0, lam, torch.full_like(lam, math.inf))           # no payload: no change, whatever the costs
    return ops.embed_ternary(cover_u8, rho, lam, seeds_dev)


def embed(cover_u8: torch.Tensor, stego_method: str, message, *, h: int = 10, seeds, rho: typing.Optional[torch.Tensor] = None,
          permute: bool = True, key: int = 0, strict: bool = True, workspace_cap: typing.Optional[int] = None, **params):
    """stc_ml.embed under the cost of 'SUNIWARDT' or 'WOWT': `rho` = cost_map(cover_u8, the method's cost, **params) (made here when
    None); every other argument and the five results (stego, changes, distortion, ok, layers) are stc_ml.embed's."""
    method = method_name(stego_method)
    if method in SIMULATED:
        raise NotImplementedError(f"{method!r} simulates its sender: use simulate, or {method + 'T'!r} for a real message")
    if rho is None:
        rho = cost_map(cover_u8, method_cost(method), **params)
    return stc_ml.embed(cover_u8, message, rho=rho, h=h, seeds=seeds, permute=permute, key=key, strict=strict, workspace_cap=workspace_cap)


def extract(stego_u8: torch.Tensor, layers, *, h: int = 10, seeds, permute: bool = True, key: int = 0):
    """stc_ml.extract: the receiver needs no cost, so the method does not matter."""
    return stc_ml.extract(stego_u8, layers, h=h, seeds=seeds, permute=permute, key=key)


# ---- whole data sets --------------------------------------------------------------------------------------------------------

def folder_name(stego_method: str, alpha: float) -> str:
    """`stego_<METHOD>_alpha_<a>_independent_images` (embed.twin_folder)."""
    return _embed.twin_folder(method_name(stego_method), alpha)


def write_dataset(data_dir, stego_method: str, alpha=None, *, message: typing.Optional[bytes] = None, h: int = 10,
                  split: typing.Optional[str] = None, stream: int = 0, **params) -> typing.List[pathlib.Path]:
    """Twins of every cover of `data_dir` (images*/files.csv, or the rows of `split`), written beside the covers; returns the folders.
    'SUNIWARD' / 'WOW': `alpha`, one value or several in [0, log2 3).  'SUNIWARDT' / 'WOWT': either `alpha` (in (0, log2 3): k =
    round(alpha H W) random bits per image) or `message` (bytes, the same in every image; the folder's alpha is 8 len(message) / (H W),
    so the covers must share one size), at constraint height `h`; the files.csv then has each image's layer lengths in `bits_high` and
    `bits_low`.  params: cost_map's (`sigma`, `clamp`); the cost plane is made once per chunk of covers.  A folder's files.csv lists
    exactly the files of this call.  An image that cannot carry the payload raises ValueError naming its batch."""
    method = method_name(stego_method)
    cost = method_cost(method)

    def prepare(cover):
        return cost_map(cover, cost, **params)

    if method in SIMULATED:
        if message is not None:
            raise ValueError(f"{method!r} simulates its sender and takes no message: use {method + 'T'!r}")

        def make(cover, a, seeds, rho):
            return simulate(cover, method, a, seeds, rho=rho)[0], {}

        return _embed.write_twins(data_dir, method, _embed.payload_list(ALPHA_RANGE[method], alpha, whose=f" for {method!r}"), make,
                                  prepare=prepare, split=split, stream=stream)
    payloads = _embed.payload_list(ALPHA_RANGE[method], alpha, message, with_message=True)
    h = stc.check_height("write_dataset: ", h)

    def make(cover, msg, seeds, rho):
        stego, _, _, _, layers = embed(cover, method, msg, rho=rho, h=h, seeds=seeds)
        layers = layers.cpu().numpy()
        return stego, {"bits_high": [int(v) for v in layers[:, 0]], "bits_low": [int(v) for v in layers[:, 1]]}

    return _embed.write_twins(data_dir, method, payloads, make, prepare=prepare, columns=stc_ml.COLUMNS[len(_embed.CSV_COLUMNS):], split=split,
                              stream=stream)


def extract_dataset(data_dir, stego_method: str, alpha: float, out_dir, *, h: int = 10, stream: int = 0,
                    batch_size: int = 32) -> typing.List[pathlib.Path]:
    """stc_ml.extract_dataset for the folder of ('SUNIWARDT' | 'WOWT', alpha): every image's `bits_high` + `bits_low` message bits, packed,
    to `out_dir/<stem>.bin`; returns the files."""
    method = method_name(stego_method)
    if method in SIMULATED:
        raise NotImplementedError(f"{method!r} twins are simulated and hold no message: read {method + 'T'!r} folders")

    def read(stego, seeds, rows):
        layers = np.stack([rows["bits_high"].to_numpy(np.int64), rows["bits_low"].to_numpy(np.int64)], axis=1)
        got, ks = extract(stego, layers, h=h, seeds=seeds)
        return [b[:int(k)] for b, k in zip(got.cpu().numpy(), ks.cpu().numpy())]

    return _embed.read_twins(data_dir, folder_name(method, alpha), out_dir, read, stream=stream, batch_size=batch_size)


def main(argv=None) -> None:
    ap, p_embed, _ = stc.cli_parser("Write stego twins of a data set's covers under the S-UNIWARD or the WOW cost, and read messages back; both on "
                                    "the GPU.  SUNIWARD / WOW simulate the payload-limited +-1 sender (--alphas only); SUNIWARDT / WOWT embed a "
                                    "message with a two-layer syndrome-trellis code.", METHODS,
                                    "payloads in bits per pixel: [0, log2 3) simulated, (0, log2 3) random bits for the ...T methods")
    p_embed.add_argument("--sigma", type=float, default=1.0, help="S-UNIWARD's stabilising constant")
    ns = ap.parse_args(argv)
    if ns.command == "embed":
        method = method_name(ns.stego_method)
        params = {"sigma": ns.sigma} if method_cost(method) == "SUNIWARD" else {}
        message = pathlib.Path(ns.message).read_bytes() if ns.message else None
        for folder in write_dataset(ns.data, method, ns.alphas, message=message, h=ns.h, split=ns.split, stream=ns.stream, **params):
            print(folder)
    else:
        for f in extract_dataset(ns.data, ns.stego_method, ns.alpha, ns.out, h=ns.h, stream=ns.stream):
            print(f)


if __name__ == "__main__":
    main()
