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

import argparse
import math
import pathlib
import typing

import numpy as np
import torch

from . import embed as _embed
from . import fabrika, stc

METHODS = ("STCT",)
ALPHA_MAX = math.log2(3.0)                                           # payloads lie below it
REASONS = ("the payload exceeds the capacity", "the high layer has no solution", "the low layer has no solution")


def method_name(stego_method: str = "STCT") -> str:
    """'STCT', matched case-insensitively."""
    m = str(stego_method).upper()
    if m not in METHODS:
        raise NotImplementedError(f"stego method {stego_method!r} is not a two-layer syndrome-trellis embedder here: choose {' / '.join(METHODS)}")
    return m


def folder_name(stego_method: str, alpha: float) -> str:
    """`stego_STCT_alpha_<a>_independent_images`, embed.folder_name's scheme."""
    return f"stego_{method_name(stego_method)}_alpha_{float(alpha)}_independent_images"


def _planes(who: str, t) -> typing.Tuple[int, int, int]:
    if not (isinstance(t, torch.Tensor) and t.dim() == 3 and t.dtype == torch.uint8):
        raise ValueError(f"{who}: an (N,H,W) uint8 tensor is expected")
    return tuple(t.shape)


def _height(who: str, h) -> int:
    if not 1 <= int(h) <= stc.MAX_H:
        raise ValueError(f"{who}: constraint height h={h} outside 1..{stc.MAX_H}")
    return int(h)


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
    n, hh, ww = _planes("embed", cover_u8)
    hw = hh * ww
    dev = cover_u8.device
    h = _height("embed", h)
    if isinstance(message, torch.Tensor):
        if message.dtype != torch.uint8 or message.dim() != 2 or message.shape[0] != n:
            raise ValueError(f"embed: message must be an ({n}, k) uint8 tensor of 0 / 1 or a payload in bits per pixel")
        msg = message.to(dev).contiguous()
    else:
        alpha = float(message)
        if not 0.0 < alpha < ALPHA_MAX:
            raise ValueError(f"embed: alpha outside (0, log2 3): {message!r}")
        msg = None
    k = msg.shape[1] if msg is not None else int(round(alpha * hw))
    if k < 2:
        raise ValueError(f"embed: k={k} message bits; two layers need at least 2")
    s = stc._seeds("embed", seeds, n, dev)
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
    n, hh, ww = _planes("extract", stego_u8)
    hw = hh * ww
    dev = stego_u8.device
    h = _height("extract", h)
    lay = np.asarray(layers.cpu() if isinstance(layers, torch.Tensor) else layers).astype(np.int64)
    if lay.shape != (n, 2) or (lay < 0).any() or (lay > hw).any() or (lay[:, 1] < 1).any():
        raise ValueError(f"extract: layers must be ({n}, 2) integers [k1, k0] with 0 <= k1 <= {hw} and 1 <= k0 <= {hw}")
    s = stc._seeds("extract", seeds, n, dev)
    both = torch.from_numpy(lay.astype(np.int32)).to(dev)
    k1, k0 = both[:, 0].contiguous(), both[:, 1].contiguous()
    cols = _columns_for(h, hw, both.reshape(-1), key, dev)
    path = stc.key_path(s, hh, ww, dev) if permute else None
    out = torch.zeros((n, int(lay.sum(axis=1).max())), dtype=torch.uint8, device=dev)
    ops.stc_extract_ragged(stego_u8, cols, ks=k1, bit=1, h=h, path=path, out=out)
    ops.stc_extract_ragged(stego_u8, cols, ks=k0, first=k1, bit=0, h=h, path=path, out=out)
    return out, (k1 + k0).to(torch.int64)


# ---- whole data sets --------------------------------------------------------------------------------------------------------

COLUMNS = ["name", "height", "width", "stego_method", "alpha", "bits_high", "bits_low"]


def _payloads(alphas, message) -> typing.List:
    """The payloads of one call: floats (alpha) or one bytes object"""
    if (alphas is None) == (message is None):
        raise ValueError("give either alpha(s) or a message, not both and not neither")
    if message is not None:
        if len(bytes(message)) < 1:
            raise ValueError("the message is empty")
        return [bytes(message)]
    out = [float(a) for a in np.atleast_1d(np.asarray(alphas, dtype=np.float64))]
    if not all(0.0 < a < ALPHA_MAX for a in out):
        raise ValueError(f"alpha outside (0, log2 3): {alphas!r}")
    return out


def _write_chunk(fnames, kws, *, payloads, stream, out_dir, height, prefetched=None):
    """One chunk of covers -> their stego images at every payload, written as 8-bit gray PNGs; one list of files.csv rows per cover."""
    from PIL import Image
    from . import ops
    planes = prefetched[0] if prefetched is not None else _embed._prefetch(fnames, kws)[0]
    cover = torch.from_numpy(np.ascontiguousarray(planes)).to("cuda")
    n, hh, ww = cover.shape
    rho = ops.hill_cost_f64(cover)
    seeds = [_embed.image_seed(f, stream) for f in fnames]
    rows = [[] for _ in fnames]
    for p in payloads:
        if isinstance(p, bytes):
            bits = stc.bits_from_bytes(p)
            if bits.size > hh * ww:
                raise ValueError(f"the message has {bits.size} bits, the images {hh * ww} pixels")
            msg, a = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(bits, (n, bits.size)))), bits.size / (hh * ww)
        else:
            msg, a = p, p
        try:
            stego, _, _, _, layers = embed(cover, msg, rho=rho, h=height, seeds=seeds)
        except ValueError as e:
            raise ValueError(f"{e} (the batch: {[pathlib.Path(f).name for f in fnames]})") from e
        stego, layers = stego.cpu().numpy(), layers.cpu().numpy()
        folder = folder_name("STCT", a)
        (pathlib.Path(out_dir) / folder).mkdir(parents=True, exist_ok=True)
        for i, f in enumerate(fnames):
            name = f"{folder}/{pathlib.Path(f).stem}.png"
            Image.fromarray(stego[i]).save(pathlib.Path(out_dir) / name)
            rows[i].append({"name": name, "height": hh, "width": ww, "stego_method": "STCT", "alpha": float(a),
                            "bits_high": int(layers[i, 0]), "bits_low": int(layers[i, 1])})
    return rows


_write_covers = fabrika.precovers(iterator="batched", convert_to=None, ignore_missing=True)(
    fabrika.shared_kwargs(_write_chunk, ("payloads", "stream", "out_dir", "height"), _embed._prefetch))


def write_dataset(data_dir, stego_method: str = "STCT", alpha=None, *, message: typing.Optional[bytes] = None, h: int = 10,
                  split: typing.Optional[str] = None, stream: int = 0) -> typing.List[pathlib.Path]:
    """Stego twins of every cover of `data_dir` (images*/files.csv, or the rows of `split`), written beside the covers; returns the
    folders.  Either `alpha` (one value or several, in (0, log2 3): k = round(alpha H W) random bits per image) or `message` (bytes, the
    same in every image; the folder's alpha is 8 len(message) / (H W), so the covers must share one size).  A folder's files.csv lists
    exactly the files of this call, with each image's layer lengths in `bits_high` and `bits_low`.  An image that cannot carry the
    payload raises ValueError naming its batch."""
    import pandas as pd
    data_dir = pathlib.Path(data_dir)
    method_name(stego_method)
    payloads = _payloads(alpha, message)
    h = _height("write_dataset", h)
    rows = _write_covers(data_dir, split=split, payloads=payloads, stream=int(stream), out_dir=str(data_dir), height=h)
    folders = []
    for j in range(len(payloads)):
        names = {pathlib.Path(r[j]["name"]).parent.name for r in rows}
        if len(names) != 1:
            raise ValueError(f"the covers differ in size, so one message gives several payloads: {sorted(names)}")
        folder = data_dir / names.pop()
        pd.DataFrame([r[j] for r in rows], columns=COLUMNS).to_csv(folder / "files.csv", index=False)
        folders.append(folder)
    return folders


def extract_dataset(data_dir, stego_method: str, alpha: float, out_dir, *, h: int = 10, stream: int = 0,
                    batch_size: int = 32) -> typing.List[pathlib.Path]:
    """Reads the message of every image the folder of (stego_method, alpha) lists in its files.csv, `bits_high` + `bits_low` bits each, and
    writes them, packed by stc.bytes_from_bits, to `out_dir/<stem>.bin`; returns the files.  Images are read in batches of one size."""
    import pandas as pd
    from .imread import read_luma_batch
    data_dir, out_dir = pathlib.Path(data_dir), pathlib.Path(out_dir)
    table = pd.read_csv(data_dir / folder_name(stego_method, alpha) / "files.csv")
    names = [str(v) for v in table["name"]]
    layers = np.stack([table["bits_high"].to_numpy(np.int64), table["bits_low"].to_numpy(np.int64)], axis=1)
    out_dir.mkdir(parents=True, exist_ok=True)
    written = []
    for a in range(0, len(names), int(batch_size)):
        chunk = names[a:a + int(batch_size)]
        stego = torch.from_numpy(np.ascontiguousarray(read_luma_batch([data_dir / v for v in chunk]))).to("cuda")
        got, ks = extract(stego, layers[a:a + len(chunk)], h=h, seeds=[_embed.image_seed(v, stream) for v in chunk])
        got, ks = got.cpu().numpy(), ks.cpu().numpy()
        for v, b, k in zip(chunk, got, ks):
            written.append(out_dir / f"{pathlib.Path(v).stem}.bin")
            written[-1].write_bytes(stc.bytes_from_bits(b[:int(k)]))
    return written


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Embed a message in a data set's covers by +-1 changes with a two-layer syndrome-trellis code "
                                             "over the HILL cost (STCT), and read it back; both on the GPU.")
    sub = ap.add_subparsers(dest="command", required=True)
    for name in ("embed", "extract"):
        p = sub.add_parser(name)
        p.add_argument("--data", required=True, help="data set directory (images*/files.csv)")
        p.add_argument("--stego-method", default="STCT", help=" / ".join(METHODS))
        p.add_argument("--h", type=int, default=10, help="constraint height 1..10")
        p.add_argument("--stream", type=int, default=0, help="realisation number (embed.image_seed): part of the stego key")
    p = sub.choices["embed"]
    what = p.add_mutually_exclusive_group(required=True)
    what.add_argument("--alphas", type=float, nargs="+", help="payloads in bits per pixel, (0, log2 3): random bits")
    what.add_argument("--message", help="a file whose bytes every cover carries")
    p.add_argument("--split", default=None, help="a split CSV of the data set: only its covers")
    p = sub.choices["extract"]
    p.add_argument("--alpha", type=float, required=True, help="the payload the folder is named after")
    p.add_argument("--out", required=True, help="directory for the recovered bytes, <stem>.bin per image")
    ns = ap.parse_args(argv)
    if ns.command == "embed":
        message = pathlib.Path(ns.message).read_bytes() if ns.message else None
        for folder in write_dataset(ns.data, ns.stego_method, ns.alphas, message=message, h=ns.h, split=ns.split, stream=ns.stream):
            print(folder)
    else:
        for f in extract_dataset(ns.data, ns.stego_method, ns.alpha, ns.out, h=ns.h, stream=ns.stream):
            print(f)


if __name__ == "__main__":
    main()
