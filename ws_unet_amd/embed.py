"""Stego simulators on the device: HILLR, LSBR, LSBRS, LSBRK and HILLRM twins of cover images (wsu_hill_cost_f64, wsu_rank_select_f64,
wsu_embed_threshold, wsu_embed_lsbr, wsu_embed_lsbr_seq, wsu_embed_lsbr_keyed, wsu_embed_threshold_lsbr; include/wsu.h K20-K23, K28, K30,
K34).

The reference ships its five covers with ready-made `stego_*` folders from a library outside its tree.  Here a covers-only data
set gets its twins from the package itself:

  * `simulate(cover_u8, stego_method, alpha, seeds)` on resident (N,H,W) uint8 planes;
  * `write_dataset(data_dir, stego_method, alpha)` / `python -m ws_unet_amd.embed --data DIR --stego-method HILLR --alphas .4 .2`
    writes `stego_<METHOD>_alpha_<a>_independent_images/<stem>.png` and its files.csv, which fabrika.stego_spatial and
    fabrika.cover_stego_spatial then list like the reference's folders;
  * `data.pairs.PairLoader(..., simulate=True)` makes the twin of every uploaded cover instead of decoding a second file.

HILLR is deterministic and reproduces the reference's files bit for bit: the LSB flips on the k + 1 pixels of lowest float64 HILL
cost, k = floor((H*W - 1) * alpha / 2); every pixel that ties with the threshold flips too (a flat image flips entirely).  LSBR
flips each LSB independently with probability alpha / 2 from Philox4x32-10 keyed by the image's seed: the realisation is a function
of (seed, alpha, pixel index) alone -- `image_seed(filename, stream)` makes it a function of the file stem and a stream number.
LSBRS is what most LSB-replacement tools do: the message goes into the first m = floor(alpha * H * W) pixels in file order, `order`
'rows' (row by row from the top) or 'rows_up' (from the bottom row, as BMP-style tools write).  A pixel on that path flips as under LSBR
at alpha = 1 with the same seed, so LSBRS at alpha = 1 is LSBR at alpha = 1, everything beyond position m is the cover, and a twin at a
smaller alpha is a prefix of one at a larger alpha (ws.estimate's placement='sequential' is the matching estimator).
LSBRK is LSB replacement under a shared stego key: the 64-bit `placement_key` selects a fraction alpha of the pixel positions, the same
in every image of the same size (ops.lsbr_key_mask), and a selected pixel flips as under LSBR at alpha = 1 with the image's seed.  So
LSBRK at alpha = 1 is LSBR at alpha = 1 and at alpha = 0 the cover (ws.locate finds the selected positions from many such images).
HILLRM is HILLR with a real message instead of its flip of every selected pixel: the pixels whose float64 HILL cost is at most the order
statistic of rank floor((H*W - 1) * alpha) are used (ties included, as HILLR flips them), and a used pixel flips as under LSBR at
alpha = 1 with the image's seed.  So about alpha / 2 of the pixels change, all among the cheapest; at alpha = 0 the twin is the cover
(ws.estimate's placement='adaptive' with flip_rate=0.5 is the matching estimator).
"""
from __future__ import annotations

import argparse
import math
import pathlib
import typing

import numpy as np
import torch

from . import fabrika

METHODS = ("LSBR", "HILLR", "LSBRS", "LSBRK", "HILLRM")
ORDERS = ("rows", "rows_up")


def method_name(stego_method: str) -> str:
    """'LSBR' / 'HILLR' / 'LSBRS' / 'LSBRK' / 'HILLRM', matched case-insensitively (the reference spells both 'LSBr' and 'LSBR')."""
    m = str(stego_method).upper()
    if m not in METHODS:
        raise NotImplementedError(f"stego method {stego_method!r} is not simulated here: choose one of {' / '.join(METHODS)}")
    return m


def image_seed(filename, stream: int = 0) -> int:
    """The 64-bit LSBR seed of an image: fabrika.filename_to_image_seed (file stem only, < 2^31) in the low word, `stream` above."""
    stream = int(stream)
    if not 0 <= stream < 2 ** 32:
        raise ValueError(f"stream {stream} outside [0, 2^32)")
    return fabrika.filename_to_image_seed(str(filename)) | (stream << 32)


def hillr_rank(alpha: float, h: int, w: int) -> int:
    """k = floor((H*W - 1) * alpha / 2) in float64: the k + 1 cheapest pixels change.  alpha == 0 -> -1 (no pixel changes)."""
    return int(np.floor((h * w - 1) * (float(alpha) / 2))) if alpha > 0 else -1


def hillrm_rank(alpha: float, h: int, w: int) -> int:
    """floor((H*W - 1) * alpha) in float64: the pixels up to the key of this rank are used by 'HILLRM'.  alpha == 0 -> -1 (none is)."""
    return int(np.floor((h * w - 1) * float(alpha))) if alpha > 0 else -1


def lsbrs_count(alpha: float, h: int, w: int) -> int:
    """m = floor(alpha * H * W) in float64: the number of path positions an LSBRS message occupies."""
    return int(np.floor(np.float64(alpha) * np.float64(h * w)))


def _check_placement_key(method: str, placement_key) -> typing.Optional[int]:
    """The 64-bit stego key of 'LSBRK' as an int; the other methods have none (None)."""
    if method != "LSBRK":
        return None
    if placement_key is None:
        raise ValueError("'LSBRK' needs placement_key: the 64-bit stego key that selects the used pixels of every image")
    k = int(placement_key)
    if not 0 <= k < 2 ** 64:
        raise ValueError(f"placement_key {placement_key!r} outside [0, 2^64)")
    return k


def _check_order(order) -> str:
    if order not in ORDERS:
        raise ValueError(f"unknown order {order!r}; choose from {ORDERS}")
    return order


# ---- what the four drivers (embed, embed_pm1, stc, stc_ml) check alike ---------------------------------------------------------------------

def planes_shape(who: str, t, name: str = "cover_u8") -> typing.Tuple[int, int, int]:
    """(N, H, W) of a batch of planes, which must be an (N,H,W) uint8 tensor."""
    if not (isinstance(t, torch.Tensor) and t.dim() == 3 and t.dtype == torch.uint8):
        raise ValueError(f"{who}: {name} must be an (N,H,W) uint8 tensor")
    return tuple(t.shape)


def seeds_tensor(who: str, seeds, n: int, dev, method: typing.Optional[str] = None) -> torch.Tensor:
    """One 64-bit seed per image (a list, an array or a tensor of integers, taken modulo 2^64) -> (N) int64 on `dev` holding them.
    method: the simulator that asks, for the message about missing seeds."""
    if seeds is None:
        raise ValueError(f"{who}: {method!r} needs one seed per image (embed.image_seed)" if method else
                         f"{who}: one seed per image is needed (embed.image_seed)")
    s = np.array([int(v) % 2 ** 64 for v in (seeds.tolist() if isinstance(seeds, (torch.Tensor, np.ndarray)) else seeds)], dtype=np.uint64)
    if s.shape != (n,):
        raise ValueError(f"{who}: {s.shape[0] if s.ndim else 1} seeds for {n} images")
    return torch.from_numpy(s.view(np.int64)).to(dev)


# the payload ranges of the methods, by the name an error message gives them: (0 excluded, the upper end, the upper end excluded)
ALPHA_RANGES = {"[0, 1]": (False, 1.0, False), "[0, log2 3)": (False, math.log2(3.0), True),
                "(0, 1]": (True, 1.0, False), "(0, log2 3)": (True, math.log2(3.0), True)}


def alpha_values(alpha, within: str, n: typing.Optional[int] = None, who: str = "", whose: str = "") -> np.ndarray:
    """alpha, a scalar or a sequence, as float64 values inside the range `within` of ALPHA_RANGES: one per image of a batch of n (a scalar
    serves all), or, with n None, the values as given.  The error reads `<who>alpha outside <within><whose>: <alpha>`."""
    a = np.asarray(alpha, dtype=np.float64)
    if n is None:
        a = np.atleast_1d(a)
    else:
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
            raise ValueError(f"alpha must be a scalar or one value per image ({n}), got shape {a.shape}")
        a = np.broadcast_to(a, (n,))
    open_low, top, open_top = ALPHA_RANGES[within]
    if not np.all(((a > 0) if open_low else (a >= 0)) & ((a < top) if open_top else (a <= top))):
        raise ValueError(f"{who}alpha outside {within}{whose}: {alpha!r}")
    return a


def payload_list(within: str, alphas, message: typing.Optional[bytes] = None, with_message: bool = False, whose: str = "") -> typing.List:
    """The payloads of one write_dataset call: floats inside `within`, or, where the method embeds real messages (with_message), one
    bytes object given instead of them."""
    if with_message:
        if (alphas is None) == (message is None):
            raise ValueError("give either alpha(s) or a message, not both and not neither")
        if message is not None:
            if len(bytes(message)) < 1:
                raise ValueError("the message is empty")
            return [bytes(message)]
    return [float(a) for a in alpha_values(alphas, within, whose=whose)]


def simulate(cover_u8: torch.Tensor, stego_method: str, alpha, seeds=None, *, key: typing.Optional[torch.Tensor] = None,
             order: str = "rows", placement_key: typing.Optional[int] = None):
    """cover_u8: (N,H,W) uint8 on the device; alpha: a scalar or one value per image -> (stego (N,H,W) uint8, changes (N) int64), both
    on the device.  'LSBR', 'LSBRS', 'LSBRK' and 'HILLRM' need `seeds`, one 64-bit integer per image (image_seed); 'HILLR' ignores them.
    'HILLR' and 'HILLRM' take an optional `key` = ops.hill_cost_f64(cover_u8) made earlier (several alphas of the same covers).  `order`
    ('rows' / 'rows_up') is the path of 'LSBRS'; the other methods have none.  `placement_key` is the shared stego key of 'LSBRK' (one alpha for the whole batch: the used
    positions are the same in every image)."""
    from . import ops
    method = method_name(stego_method)
    _check_order(order)
    placement_key = _check_placement_key(method, placement_key)
    n, h, w = planes_shape("simulate", cover_u8)
    a = alpha_values(alpha, "[0, 1]", n)
    dev = cover_u8.device
    if method == "HILLR":
        if key is None:
            key = ops.hill_cost_f64(cover_u8)
        k = torch.tensor([hillr_rank(v, h, w) for v in a], dtype=torch.int64).to(dev)
        return ops.embed_threshold(cover_u8, key, ops.rank_select_f64(key, k))
    s = seeds_tensor("simulate", seeds, n, dev, method)
    if method == "HILLRM":
        if key is None:
            key = ops.hill_cost_f64(cover_u8)
        k = torch.tensor([hillrm_rank(v, h, w) for v in a], dtype=torch.int64).to(dev)
        return ops.embed_threshold_lsbr(cover_u8, key, ops.rank_select_f64(key, k), s)
    if method == "LSBRK":
        if not np.all(a == a[0]):
            raise ValueError(f"simulate: 'LSBRK' takes one alpha for all images (one key selects one set of pixels), got {alpha!r}")
        return ops.embed_lsbr_keyed(cover_u8, s, placement_key, ops.lsbr_key_threshold(a[0]))
    if method == "LSBRS":
        m = torch.tensor([lsbrs_count(v, h, w) for v in a], dtype=torch.int64).to(dev)
        return ops.embed_lsbr_seq(cover_u8, s, m, order)
    t = np.array([ops.lsbr_threshold(v) for v in a], dtype=np.uint32)
    return ops.embed_lsbr(cover_u8, s, torch.from_numpy(t.view(np.int32)).to(dev))


# ---- whole data sets: the twin writer and reader of the four drivers ------------------------------------------------------------------------

CSV_COLUMNS = ("name", "height", "width", "stego_method", "alpha")      # of every twin folder's files.csv; a method may add its own


def twin_folder(method: str, alpha: float, suffix: str = "") -> str:
    """`stego_<METHOD>_alpha_<a><suffix>_independent_images`: the reference's folder scheme with the method in upper case, as its
    files.csv spells it (the reference's own folders say 'HILLr' / 'LSBr' beside 'HILLR' / 'LSBR' in the name column; that mismatch is
    not copied)."""
    return f"stego_{method}_alpha_{float(alpha)}{suffix}_independent_images"


def folder_name(stego_method: str, alpha: float, order: str = "rows", placement_key: typing.Optional[int] = None) -> str:
    """twin_folder for this module's methods.  The bottom-up twins of 'LSBRS' (order 'rows_up') go to
    `stego_LSBRS_alpha_<a>_rows_up_independent_images`, the twins of 'LSBRK' under the stego key K to
    `stego_LSBRK_alpha_<a>_key_<K>_independent_images`."""
    method = method_name(stego_method)
    return twin_folder(method, alpha, _folder_suffix(method, order, placement_key))


def _folder_suffix(method: str, order: str, placement_key) -> str:
    if method == "LSBRK":
        return f"_key_{_check_placement_key(method, placement_key)}"
    return "_rows_up" if method == "LSBRS" and _check_order(order) == "rows_up" else ""


def bits_from_bytes(data: bytes) -> np.ndarray:
    """bytes -> their bits as uint8 0 / 1, the most significant bit of each byte first."""
    return np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8))


def bytes_from_bits(bits) -> bytes:
    """The inverse of bits_from_bytes; a trailing group of fewer than 8 bits is dropped."""
    b = np.asarray(bits, dtype=np.uint8).reshape(-1)
    if b.size and b.max() > 1:
        raise ValueError("bytes_from_bits: bits must be 0 / 1")
    return np.packbits(b[:b.size // 8 * 8]).tobytes()


def _prefetch(fnames, kws):
    from .imread import read_luma_batch
    return (read_luma_batch(fnames),)


def _write_chunk(fnames, kws, *, method, payloads, stream, out_dir, make, prepare=None, suffix="", prefetched=None):
    """One chunk of covers -> their twins at every payload, written as 8-bit gray PNGs; one list of files.csv rows per cover.  What the
    method does is two callables: prepare(cover) -> what it makes once per chunk (its cost map; None: nothing) and make(cover, payload,
    seeds, prepared) -> (stego (N,H,W) uint8 on the device, {column: one value per image} for columns beyond CSV_COLUMNS).  A payload is
    an alpha, or a bytes message: make then gets its bits as an (N, bits) uint8 tensor, and alpha is bits per pixel.  A ValueError of
    make names the batch's files."""
    from PIL import Image
    planes = prefetched[0] if prefetched is not None else _prefetch(fnames, kws)[0]
    cover = torch.from_numpy(np.ascontiguousarray(planes)).to("cuda")
    n, hh, ww = cover.shape
    prepared = prepare(cover) if prepare is not None else None
    seeds = [image_seed(f, stream) for f in fnames]
    rows = [[] for _ in fnames]
    for p in payloads:
        a = p
        if isinstance(p, bytes):
            bits = bits_from_bytes(p)
            if bits.size > hh * ww:
                raise ValueError(f"the message has {bits.size} bits, the images {hh * ww} pixels")
            p, a = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(bits, (n, bits.size)))), bits.size / (hh * ww)
        try:
            stego, extra = make(cover, p, seeds, prepared)
        except ValueError as e:
            raise ValueError(f"{e} (the batch: {[pathlib.Path(f).name for f in fnames]})") from e
        stego = stego.cpu().numpy()
        folder = twin_folder(method, a, suffix)
        (pathlib.Path(out_dir) / folder).mkdir(parents=True, exist_ok=True)
        for i, f in enumerate(fnames):
            name = f"{folder}/{pathlib.Path(f).stem}.png"
            Image.fromarray(stego[i]).save(pathlib.Path(out_dir) / name)
            rows[i].append({"name": name, "height": hh, "width": ww, "stego_method": method, "alpha": float(a),
                            **{k: v[i] for k, v in extra.items()}})
    return rows


_write_covers = fabrika.precovers(iterator="batched", convert_to=None, ignore_missing=True)(
    fabrika.shared_kwargs(_write_chunk, ("method", "payloads", "stream", "out_dir", "make", "prepare", "suffix"), _prefetch))


def write_twins(data_dir, method: str, payloads: typing.List, make, *, prepare=None, suffix: str = "", columns=(),
                split: typing.Optional[str] = None, stream: int = 0) -> typing.List[pathlib.Path]:
    """The body of every driver's write_dataset: twins of every cover of `data_dir` (images*/files.csv, or the rows of `split`) at every
    payload (payload_list), through _write_chunk's `make` and `prepare`; returns the folders, one per payload.  A folder's files.csv lists
    exactly the files of this call, with CSV_COLUMNS and the method's own `columns`.  A bytes payload names its folder by its bits per
    pixel, so the covers must share one size."""
    import pandas as pd
    data_dir = pathlib.Path(data_dir)
    rows = _write_covers(data_dir, split=split, method=method, payloads=payloads, stream=int(stream), out_dir=str(data_dir), make=make,
                         prepare=prepare, suffix=suffix)
    folders = []
    for j, p in enumerate(payloads):
        if isinstance(p, bytes):
            names = {pathlib.Path(r[j]["name"]).parent.name for r in rows}
            if len(names) != 1:
                raise ValueError(f"the covers differ in size, so one message gives several payloads: {sorted(names)}")
            folder = data_dir / names.pop()
        else:
            folder = data_dir / twin_folder(method, p, suffix)
        pd.DataFrame([r[j] for r in rows], columns=[*CSV_COLUMNS, *columns]).to_csv(folder / "files.csv", index=False)
        folders.append(folder)
    return folders


def read_twins(data_dir, folder: str, out_dir, read, *, stream: int = 0, batch_size: int = 32) -> typing.List[pathlib.Path]:
    """The body of every driver's extract_dataset: the images `folder`'s files.csv lists, in batches of one size; read(stego (N,H,W) uint8
    on the device, seeds, the batch's rows of the csv) -> one array of message bits per image, written, packed by stc.bytes_from_bits, to
    `out_dir/<stem>.bin`; returns the files."""
    import pandas as pd
    from .imread import read_luma_batch
    data_dir, out_dir = pathlib.Path(data_dir), pathlib.Path(out_dir)
    table = pd.read_csv(data_dir / folder / "files.csv")
    names = [str(v) for v in table["name"]]
    out_dir.mkdir(parents=True, exist_ok=True)
    written = []
    for a in range(0, len(names), int(batch_size)):
        chunk = names[a:a + int(batch_size)]
        stego = torch.from_numpy(np.ascontiguousarray(read_luma_batch([data_dir / v for v in chunk]))).to("cuda")
        for v, b in zip(chunk, read(stego, [image_seed(v, stream) for v in chunk], table.iloc[a:a + len(chunk)])):
            written.append(out_dir / f"{pathlib.Path(v).stem}.bin")
            written[-1].write_bytes(bytes_from_bits(b))
    return written


def write_dataset(data_dir, stego_method: str, alpha, *, split: typing.Optional[str] = None, stream: int = 0,
                  order: str = "rows", placement_key: typing.Optional[int] = None) -> typing.List[pathlib.Path]:
    """Twins of every cover of `data_dir` (images*/files.csv, or the rows of `split`) at `alpha` (one value or several), written
    beside the covers; returns the folders.  A folder's files.csv lists exactly the files of this call.  `order`: the path of 'LSBRS';
    `placement_key`: the shared stego key of 'LSBRK'."""
    from . import ops
    method = method_name(stego_method)
    _check_order(order)
    placement_key = _check_placement_key(method, placement_key)

    def make(cover, a, seeds, key):
        return simulate(cover, method, a, seeds, key=key, order=order, placement_key=placement_key)[0], {}

    return write_twins(data_dir, method, payload_list("[0, 1]", alpha), make, prepare=ops.hill_cost_f64 if method in ("HILLR", "HILLRM") else None,
                       suffix=_folder_suffix(method, order, placement_key), split=split, stream=stream)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Write simulated stego twins of a data set's covers (HILLR / LSBR / LSBRS / LSBRK / HILLRM, made on the GPU).")
    ap.add_argument("--data", required=True, help="data set directory (images*/files.csv)")
    ap.add_argument("--stego-method", required=True, help=" / ".join(METHODS))
    ap.add_argument("--alphas", type=float, nargs="+", required=True, help="embedding rates in [0, 1]")
    ap.add_argument("--split", default=None, help="a split CSV of the data set: only its covers")
    ap.add_argument("--stream", type=int, default=0, help="LSBR / LSBRS / LSBRK / HILLRM realisation number (image_seed)")
    ap.add_argument("--order", choices=ORDERS, default="rows", help="LSBRS: the message runs row by row from the top, or from the bottom row up")
    ap.add_argument("--key", type=int, default=None, help="LSBRK: the 64-bit stego key that selects the used pixels of every image")
    ns = ap.parse_args(argv)
    for folder in write_dataset(ns.data, ns.stego_method, ns.alphas, split=ns.split, stream=ns.stream, order=ns.order, placement_key=ns.key):
        print(folder)


if __name__ == "__main__":
    main()
