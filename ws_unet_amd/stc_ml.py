"""The ternary two-layer syndrome-trellis embedder on the device: a real message carried by +-1 changes (wsu_stc_embed_ragged,
wsu_stc_extract_ragged, wsu_stc_layer_high / _low / _compose; include/wsu.h K43-K47).  Not part of the reference, and separate from `stc`,
whose two methods run one binary code, and from `embed_pm1`, whose 'HILL' only simulates the optimal ternary sender.

  * `embed(cover_u8, message, seeds=...)` / `extract(stego_u8, layers, seeds=...)` on resident (N,H,W) uint8 planes;
  * `write_dataset(data_dir, 'STCT', alpha)` / `python -m ws_unet_amd.stc_ml embed --data DIR --alphas .4 .2` writes
    `stego_STCT_alpha_<a>_independent_images/<stem>.png` and its files.csv beside the covers, as stc.write_dataset does; the csv has the
    columns `bits_high` and `bits_low` (k1, k0 of each image), which the receiver needs; `--message FILE` embeds the file's bytes;
  * `python -m ws_unet_amd.stc_ml extract --data DIR --alpha A --out DIR2` reads them and writes each image's bytes.

The construction is that of T. Filler, J. Judas, J. Fridrich, "Minimizing additive distortion in steganography using syndrome-trellis
codes", IEEE TIFS 6(3), 2011, sections V-VI, for two layers: the sender whose +-1 changes have the probabilities exp(-lambda rho) / Z
(lambda from ops.ternary_lambda at the payload, as embed_pm1's 'HILL') is split by the chain rule into the second-lowest bit plane and
the LSB plane given it.  Each plane is one binary syndrome-trellis code (stc's, K41) whose costs are the log-odds of that plane's flips;
the first carries k1 = floor(its entropy) bits, the second the other k0 = k - k1.  include/wsu.h gives the exact definition, and
tests/stc_ml_np.py restates it in numpy.  Both codes run along `stc.key_path(seeds)` with `stc.columns(h, ., key)`; k1 differs from image
to image, which is what the ragged entry points are for (one workgroup per image whatever its length).

Kept short on purpose: the costs are symmetric (one rho for both directions); when a layer has no solution (payloads near 1 bit per
pixel, many wet pixels) the image is reported, no smaller payload is tried; the columns are stc's untuned ones.  Not checked: no run was
compared with another implementation of syndrome-trellis codes.
"""
from __future__ import annotations

import pathlib
import typing

import numpy as np
import torch

from . import embed as _embed
from . import stc

METHODS = ("STCT",)
ALPHA_RANGE = "(0, log2 3)"                                          # of embed.ALPHA_RANGES
REASONS = ("the payload exceeds the capacity", "the high layer has no solution", "the low layer has no solution")


def method_name(stego_method: str = "STCT") -> str:
    """'STCT', matched case-insensitively."""
    m = str(stego_method).upper()
    if m not in METHODS:
        raise NotImplementedError(f"stego method {stego_method!r} is not a two-layer syndrome-trellis embedder here: choose {' / '.join(METHODS)}")
    return m


def folder_name(stego_method: str, alpha: float) -> str:
    """`stego_STCT_alpha_<a>_independent_images` (embed.twin_folder)."""
    return _embed.twin_folder(method_name(stego_method), alpha)


def _columns_for(h: int, n: int, lengths: torch.Tensor, key: int, dev) -> torch.Tensor:
    """The column table for the shortest positive length among `lengths` (read back: the table's size depends on it)."""
    pos = lengths[lengths > 0]
    shortest = int(pos.min().item()) if pos.numel() else n
    return torch.from_numpy(stc.columns(h, -(-n // max(1, min(shortest, n))), key).view(np.int32)).to(dev)


def embed(cover_u8: torch.Tensor, message, *, rho: typing.Optional[torch.Tensor] = None, h: int = 10, seeds, permute: bool = True,
          key: int = 0, strict: bool = True, workspace_cap: typing.Optional[int] = None):
    """cover_u8: (N,H,W) uint8 on the device; message: an (N,k) uint8 tensor of 0 / 1 (on the device or not), or a payload alpha in
    (0, log2 3) bits per pixel, which stands for k = round(alpha H W) bits of `stc.random_message`; k >= 2.  rho: (N,H,W) float64 costs, one
    for both directions (ops.hill_cost_f64(cover) when None; +inf = wet); h, seeds, permute, key, workspace_cap as stc.embed ->
    (stego (N,H,W) uint8, changes (N) int64, distortion (N) float64, ok (N) bool, layers (N,2) int64 = [k1, k0]), all on the device.
    distortion is the sum of rho over the changed pixels.  The receiver needs `layers`.

    An image is not ok, and its stego is the cover, for one of three reasons: the payload exceeds its capacity (ops.ternary_lambda's
    flag), the high layer's code has no solution, or the low layer's has none.  With `strict` (the default) the flags are read back and
    such images raise ValueError by index and reason.

    The host waits for the device once between the layers: the high layer's entropies decide the lengths k1, and the column table's
    size depends on the shortest of them.  Besides that only `strict` reads anything back."""
    from . import ops
    n, hh, ww = _embed.planes_shape("embed", cover_u8)
    hw = hh * ww
    dev = cover_u8.device
    h = stc.check_height("embed: ", h)
    if isinstance(message, torch.Tensor):
        if message.dtype != torch.uint8 or message.dim() != 2 or message.shape[0] != n:
            raise ValueError(f"embed: message must be an ({n}, k) uint8 tensor of 0 / 1 or a payload in bits per pixel")
        msg = message.to(dev).contiguous()
    else:
        alpha = float(_embed.alpha_values(float(message), ALPHA_RANGE, who="embed: ")[0])
        msg = None
    k = msg.shape[1] if msg is not None else int(round(alpha * hw))
    if k < 2:
        raise ValueError(f"embed: k={k} message bits; two layers need at least 2")
    s = _embed.seeds_tensor("embed", seeds, n, dev)
    if msg is None:
        msg = stc.random_message(seeds, k, dev)
    if rho is None:
        rho = ops.hill_cost_f64(cover_u8)
    lam, _, fits = ops.ternary_lambda(cover_u8, rho, torch.full((n,), float(k), dtype=torch.float64, device=dev))
    u1, rho1, ent = ops.stc_layer_high(cover_u8, rho, lam)
    k1 = torch.clamp(torch.floor(ent), 0, k - 1).to(torch.int32)
    k0 = k - k1
    cols = _columns_for(h, hw, torch.cat([k1, k0]), key, dev)                       # (the read-back)
    path = stc.key_path(s, hh, ww, dev) if permute else None
    y1, _, _, ok1 = ops.stc_embed_ragged(u1, rho1, msg, cols, s, ks=k1, h=h, path=path, workspace_cap=workspace_cap)
    u0, rho0 = ops.stc_layer_low(cover_u8, rho, lam, y1, k1)
    y0, _, _, ok0 = ops.stc_embed_ragged(u0, rho0, msg, cols, s, ks=k0, first=k1, h=h, path=path, workspace_cap=workspace_cap)
    stego, changes, distortion, ok = ops.stc_layer_compose(cover_u8, rho, y1, y0, k1, ok1 * fits.to(torch.uint8), ok0)
    ok = ok.to(torch.bool)
    if strict:
        flags = torch.stack([fits.to(torch.uint8), ok1, ok0]).cpu().numpy().astype(bool)
        if not flags.all():
            bad = [f"{i} ({REASONS[int(np.argmin(flags[:, i]))]})" for i in np.nonzero(~flags.all(axis=0))[0]]
            raise ValueError(f"embed: {k} bits at constraint height {h} cannot be embedded in image(s) {', '.join(bad)} of the batch")
    return stego, changes, distortion, ok, torch.stack([k1, k0], dim=1).to(torch.int64)


def extract(stego_u8: torch.Tensor, layers, *, h: int = 10, seeds, permute: bool = True, key: int = 0):
    """The message of every stego image: ((N, max k) uint8 of 0 / 1, zero past an image's k; k (N) int64), both on the device.  layers:
    (N,2) integers [k1, k0] as `embed` returned them; h, seeds, permute and key as `embed` was given them."""
    from . import ops
    n, hh, ww = _embed.planes_shape("extract", stego_u8, "stego_u8")
    hw = hh * ww
    dev = stego_u8.device
    h = stc.check_height("extract: ", h)
    lay = np.asarray(layers.cpu() if isinstance(layers, torch.Tensor) else layers).astype(np.int64)
    if lay.shape != (n, 2) or (lay < 0).any() or (lay > hw).any() or (lay[:, 1] < 1).any():
        raise ValueError(f"extract: layers must be ({n}, 2) integers [k1, k0] with 0 <= k1 <= {hw} and 1 <= k0 <= {hw}")
    s = _embed.seeds_tensor("extract", seeds, n, dev)
    both = torch.from_numpy(lay.astype(np.int32)).to(dev)
    k1, k0 = both[:, 0].contiguous(), both[:, 1].contiguous()
    cols = _columns_for(h, hw, both.reshape(-1), key, dev)
    path = stc.key_path(s, hh, ww, dev) if permute else None
    out = torch.zeros((n, int(lay.sum(axis=1).max())), dtype=torch.uint8, device=dev)
    ops.stc_extract_ragged(stego_u8, cols, ks=k1, bit=1, h=h, path=path, out=out)
    ops.stc_extract_ragged(stego_u8, cols, ks=k0, first=k1, bit=0, h=h, path=path, out=out)
    return out, (k1 + k0).to(torch.int64)


# ---- whole data sets --------------------------------------------------------------------------------------------------------

COLUMNS = [*_embed.CSV_COLUMNS, "bits_high", "bits_low"]


def write_dataset(data_dir, stego_method: str = "STCT", alpha=None, *, message: typing.Optional[bytes] = None, h: int = 10,
                  split: typing.Optional[str] = None, stream: int = 0) -> typing.List[pathlib.Path]:
    """Stego twins of every cover of `data_dir` (images*/files.csv, or the rows of `split`), written beside the covers; returns the
    folders.  Either `alpha` (one value or several, in (0, log2 3): k = round(alpha H W) random bits per image) or `message` (bytes, the
    same in every image; the folder's alpha is 8 len(message) / (H W), so the covers must share one size).  A folder's files.csv lists
    exactly the files of this call, with each image's layer lengths in `bits_high` and `bits_low`.  An image that cannot carry the
    payload raises ValueError naming its batch."""
    from . import ops
    method = method_name(stego_method)
    payloads = _embed.payload_list(ALPHA_RANGE, alpha, message, with_message=True)
    h = stc.check_height("write_dataset: ", h)

    def make(cover, msg, seeds, rho):
        stego, _, _, _, layers = embed(cover, msg, rho=rho, h=h, seeds=seeds)
        layers = layers.cpu().numpy()
        return stego, {"bits_high": [int(v) for v in layers[:, 0]], "bits_low": [int(v) for v in layers[:, 1]]}

    return _embed.write_twins(data_dir, method, payloads, make, prepare=ops.hill_cost_f64, columns=COLUMNS[len(_embed.CSV_COLUMNS):], split=split,
                              stream=stream)


def extract_dataset(data_dir, stego_method: str, alpha: float, out_dir, *, h: int = 10, stream: int = 0,
                    batch_size: int = 32) -> typing.List[pathlib.Path]:
    """Reads the message of every image the folder of (stego_method, alpha) lists in its files.csv, `bits_high` + `bits_low` bits each, and
    writes them, packed by stc.bytes_from_bits, to `out_dir/<stem>.bin`; returns the files.  Images are read in batches of one size."""
    def read(stego, seeds, rows):
        layers = np.stack([rows["bits_high"].to_numpy(np.int64), rows["bits_low"].to_numpy(np.int64)], axis=1)
        got, ks = extract(stego, layers, h=h, seeds=seeds)
        return [b[:int(k)] for b, k in zip(got.cpu().numpy(), ks.cpu().numpy())]

    return _embed.read_twins(data_dir, folder_name(stego_method, alpha), out_dir, read, stream=stream, batch_size=batch_size)


def main(argv=None) -> None:
    ap, _, _ = stc.cli_parser("Embed a message in a data set's covers by +-1 changes with a two-layer syndrome-trellis code over the HILL cost "
                              "(STCT), and read it back; both on the GPU.", METHODS, "payloads in bits per pixel, (0, log2 3): random bits",
                              method_default="STCT")
    ns = ap.parse_args(argv)
    if ns.command == "embed":
        stc.cli_embed(ns, write_dataset)
    else:
        for f in extract_dataset(ns.data, ns.stego_method, ns.alpha, ns.out, h=ns.h, stream=ns.stream):
            print(f)


if __name__ == "__main__":
    main()
