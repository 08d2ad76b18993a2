"""Syndrome-trellis codes on the device: a message that is really carried (wsu_philox_words, wsu_stc_embed, wsu_stc_extract; include/wsu.h
K40-K42).  Not part of the reference, and separate from `embed` and `embed_pm1`, whose adaptive methods only simulate their coding.

  * `embed(cover_u8, message, seeds=...)` / `extract(stego_u8, k, seeds=...)` on resident (N,H,W) uint8 planes;
  * `write_dataset(data_dir, stego_method, alpha)` / `python -m ws_unet_amd.stc embed --data DIR --stego-method STCR --alphas .4 .2`
    writes `stego_<METHOD>_alpha_<a>_independent_images/<stem>.png` and its files.csv beside the covers, as embed.write_dataset does;
    `--message FILE` embeds the file's bytes in every cover instead of random bits;
  * `python -m ws_unet_amd.stc extract --data DIR --stego-method STCR --alpha A --bits K --out DIR2` writes each image's bytes.

The code is the binary syndrome-trellis code of T. Filler, J. Judas, J. Fridrich, "Minimizing additive distortion in steganography using
syndrome-trellis codes", IEEE TIFS 6(3), 2011: the parity-check matrix is a band of copies of a small h x w submatrix, the sender finds
the LSB vector with syndrome m and the least total cost by the Viterbi algorithm over 2^h states, the receiver multiplies.  include/wsu.h
gives the exact definition (block widths floor(n / k) or one more, the cropped bottom, ties keep the cover bit); `columns` makes the
submatrix.  'STCR' flips the LSBs that differ (LSB replacement with a cost-coded message), 'STCM' moves such a pixel by +1 or -1, the sign
from one bit of its generator word, inwards at 0 and 255 (LSB matching under an STC).  The cost is ops.hill_cost_f64 by default, so 'STCM'
is the binary single-layer relative of embed_pm1's simulated 'HILL'; the paper's ternary two-layer construction is `ws_unet_amd.stc_ml`
('STCT'), which runs two of these codes per image through the per-image-length entries ops.stc_embed_ragged / stc_extract_ragged (K43, K44).

The stego key: sender and receiver share `seeds` (embed.image_seed: file stem and stream).  The pixel path is the stable ascending sort of
the generator word embed_lsbr gives each pixel under the image's seed (`key_path`), so it depends on (seed, H, W) alone; a random message
(`message` given as alpha) comes from the same generator under another stream (`MESSAGE_STREAM`).

Not checked: no run was compared with another implementation (the authors' C++ toolbox is not at hand); tests/stc_np.py compares the
restated definition with a brute-force search over all stego vectors instead.
"""
from __future__ import annotations

import argparse
import pathlib
import typing

import numpy as np
import torch

from . import embed as _embed

METHODS = ("STCR", "STCM")
CHANGE = {"STCR": "flip", "STCM": "pm1"}
MAX_H = 10
MESSAGE_STREAM = 0x5354434D                                          # xored into the seed's stream word for a random message


def method_name(stego_method: str) -> str:
    """'STCR' / 'STCM', matched case-insensitively."""
    m = str(stego_method).upper()
    if m not in METHODS:
        raise NotImplementedError(f"stego method {stego_method!r} is not a syndrome-trellis embedder here: choose one of {' / '.join(METHODS)}")
    return m


def folder_name(stego_method: str, alpha: float) -> str:
    """`stego_<METHOD>_alpha_<a>_independent_images` (embed.twin_folder)."""
    return _embed.twin_folder(method_name(stego_method), alpha)


# ---- the code's pieces on the host ----------------------------------------------------------------------------------------------------

def _philox4x32_10(c0: np.ndarray, k0: int, k1: int) -> np.ndarray:
    """(G) uint32 counters (c0, 0, 0, 0) under the key (k0, k1) -> (G, 4) uint32 words: wsu_philox.h on the host."""
    c = [np.asarray(c0, dtype=np.uint64), np.zeros(len(c0), np.uint64), np.zeros(len(c0), np.uint64), np.zeros(len(c0), np.uint64)]
    lo = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def columns(h: int, wmax: int, key: int = 0) -> np.ndarray:
    """The h x wmax submatrix as `wmax` h-bit integers (uint32): column t has bit 0 and bit h - 1 set (so every block reaches its own and
    its h-th message bit) and its h - 2 middle bits are entry t mod 2^(h-2) of a permutation of 0 .. 2^(h-2) - 1: the stable ascending
    order of the first 2^(h-2) words of Philox4x32-10 under `key`.  Columns are pairwise distinct while wmax <= 2^max(h - 2, 0); past
    that they repeat with that period (h = 1 and h = 2 have one column, 1 and 3)."""
    h, wmax, key = int(h), int(wmax), int(key)
    if not 1 <= h <= MAX_H:
        raise ValueError(f"columns: constraint height h={h} outside 1..{MAX_H}")
    if wmax < 1 or not 0 <= key < 2 ** 64:
        raise ValueError(f"columns: wmax={wmax} must be positive and key={key} in [0, 2^64)")
    mid = 1 << max(h - 2, 0)
    words = _philox4x32_10(np.arange((mid + 3) // 4), key & 0xFFFFFFFF, key >> 32).reshape(-1)[:mid]
    perm = np.argsort(words, kind="stable").astype(np.uint32)
    middle = perm[np.arange(wmax) % mid] << np.uint32(1) if h > 2 else np.zeros(wmax, np.uint32)
    return (middle | np.uint32(1) | np.uint32(1 << (h - 1))).astype(np.uint32)


def block_widths(n: int, k: int) -> np.ndarray:
    """The k block widths floor((i + 1) n / k) - floor(i n / k): each floor(n / k) or one more, n in all."""
    edges = np.arange(int(k) + 1, dtype=np.int64) * int(n) // int(k)
    return np.diff(edges)


bits_from_bytes, bytes_from_bits = _embed.bits_from_bytes, _embed.bytes_from_bits       # (they live beside the twin writer that uses them)


# ---- on the device ------------------------------------------------------------------------------------------------------------------------

_seeds = _embed.seeds_tensor                                         # (its name while it lived here: callers outside the package, such as
                                                                     # tests written against the earlier layout, still reach it; one definition)


def key_path(seeds, h: int, w: int, device=None) -> torch.Tensor:
    """The keyed pixel paths: int32 (N, h w), per image the raster indices in stable ascending order of the pixels' generator words under
    the image's seed (ops.philox_words; the sort is torch.sort on the device, as in ops.interior_order)."""
    from . import ops
    dev = torch.device("cuda") if device is None else device
    s = seeds if isinstance(seeds, torch.Tensor) and seeds.is_cuda else _embed.seeds_tensor("key_path", seeds, len(seeds), dev)
    words = ops.philox_words(s, h, w).reshape(s.shape[0], -1).to(torch.int64) & 0xFFFFFFFF
    return torch.sort(words, dim=1, stable=True).indices.to(torch.int32).contiguous()


def random_message(seeds, k: int, device=None) -> torch.Tensor:
    """(N,k) uint8 of 0 / 1: bit 0 of the first k generator words under each seed with MESSAGE_STREAM xored into its stream word."""
    from . import ops
    dev = torch.device("cuda") if device is None else device
    s = _embed.seeds_tensor("random_message", seeds, len(seeds), dev) ^ (MESSAGE_STREAM << 32)
    return (ops.philox_words(s, 1, int(k)).reshape(s.shape[0], -1) & 1).to(torch.uint8).contiguous()


def _columns_dev(h: int, n: int, k: int, key: int, dev) -> torch.Tensor:
    return torch.from_numpy(columns(h, -(-n // k), key).view(np.int32)).to(dev)


def embed(cover_u8: torch.Tensor, message, *, rho: typing.Optional[torch.Tensor] = None, h: int = 10, seeds, change: str = "flip",
          permute: bool = True, key: int = 0, strict: bool = True, workspace_cap: typing.Optional[int] = None):
    """cover_u8: (N,H,W) uint8 on the device; message: an (N,k) uint8 tensor of 0 / 1 (on the device or not), or a payload alpha in (0, 1]
    bits per pixel, which stands for k = round(alpha H W) bits of `random_message`; rho: (N,H,W) float64 costs (ops.hill_cost_f64(cover)
    when None; +inf = wet); h: the constraint height 1..10 (2^h states: a higher code is nearer the bound and slower); seeds: one 64-bit
    integer per image; change: 'flip' or 'pm1'; permute: embed along `key_path(seeds)` (False: in raster order); key: the submatrix'
    key (`columns`) -> (stego (N,H,W) uint8, changes (N) int64, cost (N) float64, ok (N) bool), all on the device.  cost is the total
    cost of the changes, the least any stego with this message can have under this code.  An image whose wet pixels leave no solution
    has ok False and stego = cover; with `strict` (the default) the flags are read back and such images raise ValueError by index."""
    from . import ops
    n, hh, ww = _embed.planes_shape("embed", cover_u8)
    dev = cover_u8.device
    if isinstance(message, torch.Tensor):
        if message.dtype != torch.uint8 or message.dim() != 2 or message.shape[0] != n:
            raise ValueError(f"embed: message must be an ({n}, k) uint8 tensor of 0 / 1 or a payload in bits per pixel")
        msg = message.to(dev).contiguous()
    else:
        alpha = float(_embed.alpha_values(float(message), "(0, 1]", who="embed: ")[0])
        k = int(round(alpha * hh * ww))
        if k < 1:
            raise ValueError(f"embed: alpha {alpha} is less than one bit in {hh} x {ww} pixels")
        msg = random_message(seeds, k, dev)
    if change not in ops.STC_CHANGES:
        raise ValueError(f"embed: change {change!r} is not one of {' / '.join(ops.STC_CHANGES)}")
    s = _embed.seeds_tensor("embed", seeds, n, dev)
    k = msg.shape[1]
    if not 1 <= k <= hh * ww:
        raise ValueError(f"embed: k={k} message bits outside 1..{hh * ww}")
    if rho is None:
        rho = ops.hill_cost_f64(cover_u8)
    path = key_path(s, hh, ww, dev) if permute else None
    stego, cost, changes, ok = ops.stc_embed(cover_u8, rho, msg, _columns_dev(h, hh * ww, k, key, dev), s, h=h, path=path, change=change,
                                             workspace_cap=workspace_cap)
    ok = ok.to(torch.bool)
    if strict:
        bad = np.nonzero(~ok.cpu().numpy())[0]
        if bad.size:
            raise ValueError(f"embed: the code has no solution in image(s) {bad.tolist()} of the batch: too many wet pixels for {k} bits "
                             f"at constraint height {h}")
    return stego, changes, cost, ok


def extract(stego_u8: torch.Tensor, k: int, *, h: int = 10, seeds, permute: bool = True, key: int = 0) -> torch.Tensor:
    """The k message bits of every stego image: (N,k) uint8 of 0 / 1 on the device.  h, seeds, permute and key as `embed` was given them."""
    from . import ops
    n, hh, ww = _embed.planes_shape("extract", stego_u8, "stego_u8")
    k = int(k)
    if not 1 <= k <= hh * ww:
        raise ValueError(f"extract: k={k} message bits outside 1..{hh * ww}")
    dev = stego_u8.device
    s = _embed.seeds_tensor("extract", seeds, n, dev)
    path = key_path(s, hh, ww, dev) if permute else None
    return ops.stc_extract(stego_u8, _columns_dev(h, hh * ww, k, key, dev), k, h=h, path=path)


# ---- whole data sets --------------------------------------------------------------------------------------------------------

def check_height(who: str, h) -> int:
    if not 1 <= int(h) <= MAX_H:
        raise ValueError(f"{who}constraint height h={h} outside 1..{MAX_H}")
    return int(h)


def write_dataset(data_dir, stego_method: str, alpha=None, *, message: typing.Optional[bytes] = None, h: int = 10,
                  split: typing.Optional[str] = None, stream: int = 0) -> typing.List[pathlib.Path]:
    """Stego twins of every cover of `data_dir` (images*/files.csv, or the rows of `split`), written beside the covers; returns the
    folders.  Either `alpha` (one value or several, in (0, 1]: k = round(alpha H W) random bits per image) or `message` (bytes, the same in
    every image; the folder's alpha is 8 len(message) / (H W), so the covers must share one size).  A folder's files.csv lists exactly the
    files of this call.  An image in which the code has no solution raises ValueError naming its batch."""
    from . import ops
    method = method_name(stego_method)
    payloads = _embed.payload_list("(0, 1]", alpha, message, with_message=True)
    h = check_height("", h)

    def make(cover, msg, seeds, rho):
        return embed(cover, msg, rho=rho, h=h, seeds=seeds, change=CHANGE[method])[0], {}

    return _embed.write_twins(data_dir, method, payloads, make, prepare=ops.hill_cost_f64, split=split, stream=stream)


def extract_dataset(data_dir, stego_method: str, alpha: float, bits: int, out_dir, *, h: int = 10, stream: int = 0,
                    batch_size: int = 32) -> typing.List[pathlib.Path]:
    """Reads `bits` message bits from every image the folder of (stego_method, alpha) lists in its files.csv and writes them, packed by
    bytes_from_bits, to `out_dir/<stem>.bin`; returns the files.  Images are read in batches of one size."""
    def read(stego, seeds, rows):
        return extract(stego, bits, h=h, seeds=seeds).cpu().numpy()

    return _embed.read_twins(data_dir, folder_name(stego_method, alpha), out_dir, read, stream=stream, batch_size=batch_size)


def cli_parser(description: str, methods, alphas_help: str, method_default: typing.Optional[str] = None):
    """The command line stc and stc_ml share: `embed` (--alphas or --message, --split) and `extract` (--alpha, --out), both with --data,
    --stego-method, --h and --stream -> (the parser, its embed subparser, its extract subparser) for the caller's own options."""
    ap = argparse.ArgumentParser(description=description)
    sub = ap.add_subparsers(dest="command", required=True)
    for name in ("embed", "extract"):
        p = sub.add_parser(name)
        p.add_argument("--data", required=True, help="data set directory (images*/files.csv)")
        p.add_argument("--stego-method", required=method_default is None, default=method_default, help=" / ".join(methods))
        p.add_argument("--h", type=int, default=10, help="constraint height 1..10")
        p.add_argument("--stream", type=int, default=0, help="realisation number (embed.image_seed): part of the stego key")
    p = sub.choices["embed"]
    what = p.add_mutually_exclusive_group(required=True)
    what.add_argument("--alphas", type=float, nargs="+", help=alphas_help)
    what.add_argument("--message", help="a file whose bytes every cover carries")
    p.add_argument("--split", default=None, help="a split CSV of the data set: only its covers")
    p = sub.choices["extract"]
    p.add_argument("--alpha", type=float, required=True, help="the payload the folder is named after")
    p.add_argument("--out", required=True, help="directory for the recovered bytes, <stem>.bin per image")
    return ap, sub.choices["embed"], sub.choices["extract"]


def cli_embed(ns, write) -> None:
    """The `embed` command of cli_parser's arguments through a module's write_dataset."""
    message = pathlib.Path(ns.message).read_bytes() if ns.message else None
    for folder in write(ns.data, ns.stego_method, ns.alphas, message=message, h=ns.h, split=ns.split, stream=ns.stream):
        print(folder)


def main(argv=None) -> None:
    ap, _, p = cli_parser("Embed a message in a data set's covers with a syndrome-trellis code over the HILL cost, and read it back (STCR "
                          "flips LSBs, STCM changes by +-1; both on the GPU).", METHODS, "payloads in bits per pixel, (0, 1]: random bits")
    p.add_argument("--bits", type=int, required=True, help="message bits to read from each image")
    ns = ap.parse_args(argv)
    if ns.command == "embed":
        cli_embed(ns, write_dataset)
    else:
        for f in extract_dataset(ns.data, ns.stego_method, ns.alpha, ns.bits, ns.out, h=ns.h, stream=ns.stream):
            print(f)


if __name__ == "__main__":
    main()
