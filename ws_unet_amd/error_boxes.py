"""KB-stratified absolute-error box table of the reference, results/prediction/ae_boxes_3.csv (src/error_boxes.py):

    python -m ws_unet_amd.error_boxes --data DATA --out ae_boxes_3.csv [--model-dir DIR] [--num-pixels N] [--take-num-images N] [--mode M]

How does a predictor's absolute error (AE) behave on the pixels the KB filter finds easy, and on those it finds hard?  Per predictor
the AE of every interior pixel [1:-1,1:-1] of the test split is formed (filters: |y - x @ f| in float64; UNets: |x - y*255| in
float32), image-major in fabrika's order; the pixels are cut into five slices by the anchor's (KB's) AE at the edges 0.5, 1.5, 3.5
and 7.5, and each (predictor, slice) gets min, q_25_iqr, q_25, q_50, q_75, q_75_iqr, max as pandas computes them.

The reference's slicing is restated with its off-by-one (src/error_boxes.py `plot_error`): it sorts by the anchor, cuts at
edge_j = argmin(sorted <= e_j) - 1 and takes Python slices [0:edge_0], [edge_0:edge_1], ..., [edge_3:N], so each slice hands its
last element to the next one, and with no anchor <= 0.5 (edge -1 = N-1) slices overlap.  Ranks follow the stable sort by
(anchor AE, global index).  Where the reference produces an artefact this module raises ValueError: a NaN / infinite AE (numpy's
sort and pandas' quantile would treat it differently) and images of different sizes (the reference's np.array rejects them).

Everything runs on the GPU: K16 (wsu_ae_values) writes one float32 key per pixel and predictor, K17 (wsu_ae_slices) finds the slice
boundaries, K18 (wsu_ae_select) the order statistics by an exact radix select; the host does the linear interpolation and the IQR
clip in float64, exactly as pandas does.  The keys are exact: K10's residual is float32 already, and a filter's AE is exact in
float32 when its taps are multiples of 2^-12 and 255 * (1 + sum |f|) < 2^12 (KB and AVG are; other filter taps are refused).
A fitted filter registered by name (filters.register_filter, --kernels) has arbitrary taps: its key is its float64 AE rounded to
float32.  Rounding is monotone, so each of its order statistics is the rounding of the exact one (relative error at most 2^-24); it
cannot be the anchor, whose comparisons with the edges must be exact.
"""
from __future__ import annotations

import argparse
import logging
import math
import pathlib
import typing

import numpy as np

from . import fabrika, filters, unet_run
from .hill import quantile_index
from .imread import imread4_u8
from .planes import plane_groups, upload_planes

EDGE_VALUES = (.5, 1.5, 3.5, 7.5)
STATS = ("min", "q_25_iqr", "q_25", "q_50", "q_75", "q_75_iqr", "max")
COLUMNS = ("Type", "edge_interval") + STATS
QUANTILES = (.25, .5, .75)
DATA_PATH = "../data"
UNET_RUNS = ("dropout", "LSBR")          # the reference's two UNets, <model dir>/<stego method> (labelled UNet_<config loss>)
BATCH_SIZE = 32


# ---- host pieces of the definition -------------------------------------------------------------------------------------------

def subset_residual(resid: np.ndarray, fname: str, size: typing.Optional[int]) -> np.ndarray:
    """src/error_boxes.py `subset_residual`: `size` pixels drawn with replacement by default_rng(filename_to_image_seed(fname)),
    in draw order, or all of them flattened when `size` is falsy."""
    resid = np.asarray(resid)
    if not size:
        return resid.flatten()
    sel = subset_indices(fname, resid.size, size)
    return resid[(sel // resid.shape[1], sel % resid.shape[1])]


def subset_indices(fname: str, count: int, size: int) -> np.ndarray:
    """The flat indices `subset_residual` draws: rng.integers(count, size=size) with rng = default_rng(image seed of fname)."""
    rng = np.random.default_rng(fabrika.filename_to_image_seed(fname))
    return rng.integers(count, size=size)


def filter_taps(f) -> np.ndarray:
    """A filter (8 flattened taps or a (3,3[,1]) kernel, see ops.filter_taps) -> its 9 float64 weights of x[r-1+a][c-1+b], if its AE
    is exact in float32 (taps multiples of 2^-12 and 255 * (1 + sum |f|) < 2^12: the residual is then a multiple of 2^-12 below 2^12,
    24 significant bits).  ValueError otherwise."""
    from . import ops
    t = ops.filter_taps(f, np.float64, "weights", "2d 8")
    scaled = t * 4096.0
    if not (np.all(np.isfinite(t)) and np.array_equal(scaled, np.round(scaled)) and 255.0 * (1.0 + np.abs(t).sum()) < 4096.0):
        raise ValueError(f"filter {np.asarray(f).reshape(-1).tolist()}: its AE is not exact in float32 (taps must be multiples of "
                         "2^-12 with 255 * (1 + sum |f|) < 2^12)")
    return t


def edge_labels(edges=EDGE_VALUES) -> typing.List[str]:
    """The reference's edge_interval labels: f'{lo}-{hi}' over [0] + edges + [inf] ('0-0.5', ..., '7.5-inf')."""
    vals = [0] + list(edges) + [np.inf]
    return [f"{vals[j]}-{vals[j + 1]}" for j in range(len(vals) - 1)]


def slice_ranges(counts, n: int) -> typing.List[typing.Tuple[int, int]]:
    """Rank ranges [S_j, T_j) of the reference's slices from c_j = #(anchor <= e_j) over n pixels: edge_j = c_j - 1 when
    0 < c_j < n, else -1 (argmin of an all-True or all-False mask is 0), which as a slice bound is n - 1.  Empty when S_j >= T_j."""
    bounds = [0] + [int(c) - 1 if 0 < int(c) < n else n - 1 for c in counts] + [n]
    return [(bounds[j], bounds[j + 1]) for j in range(len(bounds) - 1)]


def lerp(a: float, b: float, g: float) -> float:
    """numpy's _lerp in float64: a + (b-a)*g, or b - (b-a)*(1-g) when g >= 0.5."""
    d = b - a
    return b - d * (1.0 - g) if g >= 0.5 else a + d * g


def iqr_interval(q25: float, q75: float, lo: float, hi: float) -> typing.Tuple[float, float]:
    """_defs.iqr_interval(.25, sign=-1.5) and (.75, sign=1.5): (q_n + sign * (q75 - q25)).clip(min, max), in float64."""
    iqr = q75 - q25
    return (float(np.clip(np.float64(q25 + -1.5 * iqr), lo, hi)), float(np.clip(np.float64(q75 + 1.5 * iqr), lo, hi)))


def _frame(rows_by_type: typing.Dict[str, typing.List[dict]]):
    """The reference's frame: groupby(['Type', 'edge_interval']) order, then sort_values(['edge_interval', 'Type'])."""
    import pandas as pd
    rows = [r for t in sorted(rows_by_type) for r in sorted(rows_by_type[t], key=lambda r: r["edge_interval"])]
    df = pd.DataFrame(rows, columns=list(COLUMNS))
    return df.sort_values(["edge_interval", "Type"])


# ---- the table from device keys (K17, K18) ------------------------------------------------------------------------------------

def _table_from_keys(keys, names: typing.Sequence[str], anchor: int, edges, count: int):
    """keys: (P, >= count) float32 device tensor, one row per predictor."""
    from . import ops
    sl = ops.ae_slices(keys[anchor], [float(e) for e in edges], count).cpu().numpy().astype(np.uint64)
    counts = [int(c) for c in sl[:-1, 0]]

    def key_at(rank: int) -> typing.Tuple[int, int]:
        row = sl[-1] if rank == count - 1 else sl[[j for j, c in enumerate(counts) if 0 < c < count and c - 1 == rank][0]]
        return int(row[1]), int(row[2]) - 1

    desc, gs = [], []
    for s, t in slice_ranges(counts, count):
        size = max(0, t - s)
        kg = [quantile_index(size, q) if size else (0, 0.0) for q in QUANTILES]
        lo, hi = key_at(s) if 0 < s < t else (0, 0), key_at(t) if s < t < count else (0, 0)
        desc.append([size, int(0 < s < t), lo[0], lo[1], int(s < t < count), hi[0], hi[1]] + [k for k, _ in kg])
        gs.append([g for _, g in kg])
    out, flags = ops.ae_select(keys, anchor, np.array(desc, dtype=np.int64), count)
    flags = flags.cpu().numpy()
    for p, name in enumerate(names):
        if flags[p]:
            raise ValueError(f"predictor {name}: negative, NaN or infinite absolute error")
    v = out.cpu().numpy().view(np.float32).astype(np.float64)
    labels = edge_labels(edges)
    rows = {}
    for p, name in enumerate(names):
        rows[name] = []
        for j, label in enumerate(labels):
            row = {"Type": name, "edge_interval": label}
            if desc[j][0] == 0:                                    # pandas: explode([]) is one NaN row
                row.update({k: math.nan for k in STATS})
            else:
                o = v[p, j]
                mn, mx = float(o[0]), float(o[1])
                q = [lerp(float(o[2 + 2 * t]), float(o[3 + 2 * t]), gs[j][t]) for t in range(3)]
                lo_iqr, hi_iqr = iqr_interval(q[0], q[2], mn, mx)
                row.update({"min": mn, "q_25_iqr": lo_iqr, "q_25": q[0], "q_50": q[1], "q_75": q[2], "q_75_iqr": hi_iqr, "max": mx})
            rows[name].append(row)
    return _frame(rows)


def box_table(results: typing.Mapping[str, typing.Any], anchor: str, edges=EDGE_VALUES):
    """The table half of `plot_error(results, anchor, fname)` (no figure): the reference's DataFrame with columns COLUMNS, from a
    mapping of predictor name -> AE values (numpy arrays of any shape, flattened image-major, or float32 device tensors), all of
    one length.  Values must be finite, non-negative and exact in float32."""
    import torch
    names = list(results)
    if anchor not in results:
        raise ValueError(f"anchor {anchor!r} is not among the predictors {names}")
    if not 1 <= len(edges) <= 5:
        raise ValueError(f"1 to 5 edges, got {len(edges)}")
    flat = {}
    for name in names:
        v = results[name]
        if isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32:
            flat[name] = v.reshape(-1)
            continue
        a = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)
        if not np.all(np.isfinite(a)):
            raise ValueError(f"predictor {name}: NaN or infinite absolute error")
        a32 = a.astype(np.float32)
        if not np.array_equal(a32.astype(np.float64), a):
            raise ValueError(f"predictor {name}: values are not exact in float32")
        flat[name] = a32
    count = {int(f.numel() if isinstance(f, torch.Tensor) else f.size) for f in flat.values()}
    if len(count) != 1:
        raise ValueError(f"predictors differ in length: { {k: int(f.numel() if isinstance(f, torch.Tensor) else f.size) for k, f in flat.items()} }")
    count = count.pop()
    if count == 0:
        raise ValueError("no pixels")
    keys = torch.empty((len(names), count), dtype=torch.float32, device="cuda")
    for p, name in enumerate(names):
        f = flat[name]
        keys[p].copy_(f if isinstance(f, torch.Tensor) else torch.from_numpy(f))
    return _table_from_keys(keys, names, names.index(anchor), edges, count)


# ---- predictors and their keys (K16) ------------------------------------------------------------------------------------------

class _Pred:
    def __init__(self, name, taps=None, model=None, exact=True):
        self.name, self.taps, self.model, self.exact = name, taps, model, exact


def _resolve(name: str, spec, mode) -> _Pred:
    """A predictor spec: a filter name of filters.NAMED_FILTERS, filter taps, a UNet model / UNetEstimator, or (model_path,
    model_name) of a trained run (loaded in inference `mode`)."""
    import torch
    from .ws.estimate import UNetEstimator, as_unet_estimator
    if isinstance(spec, str):
        if spec not in filters.NAMED_FILTERS:
            raise ValueError(f"predictor {name}: unknown filter {spec!r}")
        try:
            return _Pred(name, taps=filter_taps(filters.get_coefficients(spec)))
        except ValueError:
            if spec in filters.BUILTIN_FILTERS:
                raise
        from . import ops                                           # a registered fit: float32-rounded keys (module docstring)
        return _Pred(name, taps=ops.filter_taps(filters.get_coefficients(spec), np.float64, "weights", "2d 8"), exact=False)
    if isinstance(spec, (UNetEstimator, torch.nn.Module)) or (isinstance(spec, tuple) and len(spec) == 2 and not isinstance(spec[0], (int, float))):
        return _Pred(name, model=as_unet_estimator(spec, mode).model)
    return _Pred(name, taps=filter_taps(spec))


def _keys_of(x, pred: _Pred, keys_row, offset: int, flag, idx) -> None:
    """K16 for one predictor over (N,H,W) device planes."""
    from . import ops
    if pred.taps is not None:
        ops.ae_values(x, keys_row, offset, flag, pixel_filter=pred.taps, idx=idx)
        return
    unet_run.check_unet_geometry(x.shape[1:], f"predictor {pred.name}: the UNet")
    ops.ae_values(x, keys_row, offset, flag, x_hat=unet_run.unet_plane(pred.model, x), hat_scale=255., idx=idx)


def _indices(fnames, count: int, num_pixels, device):
    import torch
    if not num_pixels:
        return None
    return torch.from_numpy(np.stack([subset_indices(f, count, num_pixels) for f in fnames]).astype(np.int64)).to(device)


def _check_flags(flags, preds) -> None:
    f = flags.cpu().numpy()
    for p, pred in enumerate(preds):
        if f[p] & 1:
            raise ValueError(f"predictor {pred.name}: NaN or infinite absolute error")
        if f[p] & 2:
            raise RuntimeError(f"predictor {pred.name}: a subset index outside the image interior")


def _groups(fnames, hw):
    """Decoded Y planes of a chunk: [(host (n,H,W) uint8 tensor, fnames)], one group for the chunk or one per image when ragged."""
    groups = plane_groups(fnames)
    for (g, fs), i in zip(groups, np.cumsum([0] + [len(f) for _, f in groups])[:-1]):
        if tuple(g.shape[1:]) != tuple(hw[i]):
            raise ValueError(f"{fs[0]}: decoded as {tuple(g.shape[1:])}, files.csv says {tuple(hw[i])}")
    return groups


def _fill(fnames, hw, per, preds, rows, keys, flags, num_pixels, batch_size, progress_on) -> None:
    """Stream the files through the batched u8 reader (decode of chunk k+1 beside the GPU work on chunk k) and write the keys of
    `preds` into keys[rows[p]] at each image's offset."""
    import torch
    chunks = [range(k, min(k + batch_size, len(fnames))) for k in range(0, len(fnames), batch_size)]
    offsets = np.concatenate([[0], np.cumsum(per)])

    def submit(chunk, groups):                                      # upload and queue K16 for every predictor; nothing is read back
        i0 = chunk[0]
        for planes, fs in groups:
            x = upload_planes(planes, "cuda")
            idx = _indices(fs, (x.shape[1] - 2) * (x.shape[2] - 2), num_pixels, x.device)
            for p, pred in enumerate(preds):
                r = rows[p]
                _keys_of(x, pred, keys[r], int(offsets[i0]), flags[r:r + 1], idx)
            i0 += len(fs)

    stage = lambda chunk: _groups([fnames[i] for i in chunk], [hw[i] for i in chunk])
    for _ in fabrika.tqdm(fabrika.pipeline(chunks, stage, submit, lambda handle: None), total=len(chunks), disable=not progress_on):
        pass
    torch.cuda.current_stream().synchronize()


def run(data_path, predictors: typing.Mapping[str, typing.Any] = None, anchor: str = "KB", split: str = "split_te.csv",
        shuffle_seed: int = 12345, take_num_images: int = None, num_pixels: int = None, iterator: str = "batched", mode: str = None,
        progress_on: bool = False, edges=EDGE_VALUES, batch_size: int = BATCH_SIZE):
    """The ae_boxes table over a data set: the cover rows of `split` (fabrika's precovers, shuffled with `shuffle_seed`, the first
    `take_num_images`), every predictor's AE written on the device (4 B per pixel and predictor, sized from files.csv), then K17 /
    K18.  `predictors`: name -> spec (see _resolve; default KB and AVG).  num_pixels: `subset_residual`'s per-image draws.
    iterator='batched' decodes and runs `batch_size` images at a time; 'python' one image at a time.  Same table either way."""
    import torch
    predictors = {"KB": "KB", "AVG": "AVG"} if predictors is None else dict(predictors)
    if anchor not in predictors:
        raise ValueError(f"anchor {anchor!r} is not among the predictors {list(predictors)}")
    if iterator not in ("batched", "python"):
        raise ValueError(f"unknown iterator {iterator!r}")
    preds = [_resolve(name, spec, mode) for name, spec in predictors.items()]
    if not preds[list(predictors).index(anchor)].exact:
        raise ValueError(f"anchor {anchor!r}: a fitted filter's AE is not exact in float32, so it cannot define the slices")
    select = fabrika.precovers(iterator=None, convert_to=None, ignore_missing=True)(lambda df, **kw: df)
    df = select(data_path, split=split, shuffle_seed=shuffle_seed, take_num_images=take_num_images)
    if df.empty:
        raise ValueError(f"no cover images selected in {data_path}")
    fnames = df["name"].tolist()
    hw = list(zip(df["height"].astype(int), df["width"].astype(int)))
    if not num_pixels and len(set(hw)) > 1:
        raise ValueError(f"images of different sizes {sorted(set(hw))}: the per-predictor AE arrays would be ragged")
    per = [num_pixels if num_pixels else (h - 2) * (w - 2) for h, w in hw]
    count = int(sum(per))
    keys = torch.empty((len(preds), count), dtype=torch.float32, device="cuda")
    flags = torch.zeros(len(preds), dtype=torch.int32, device="cuda")
    bs = batch_size if iterator == "batched" else 1
    _fill(fnames, hw, per, preds, list(range(len(preds))), keys, flags, num_pixels, bs, progress_on)
    redo = [p for p, pred in enumerate(preds) if pred.model is not None and unet_run.range_fallback(pred.model)]
    if redo:                                                       # a planar forward left its range: that model's keys once more
        flags[redo] = 0                                            # (the overflow may have stored inf in the first pass)
        _fill(fnames, hw, per, [preds[p] for p in redo], redo, keys, flags, num_pixels, bs, progress_on)
    _check_flags(flags, preds)
    return _table_from_keys(keys, [p.name for p in preds], [p.name for p in preds].index(anchor), edges, count)


# ---- the reference's per-image API ----------------------------------------------------------------------------------------------

def _ae_one(fname, pred: _Pred, num_pixels) -> np.ndarray:
    import torch
    x = torch.from_numpy(np.ascontiguousarray(imread4_u8(fname)[..., 3]))[None].cuda()
    per = num_pixels if num_pixels else (x.shape[1] - 2) * (x.shape[2] - 2)
    keys = torch.empty(per, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _keys_of(x, pred, keys, 0, flag, _indices([fname], (x.shape[1] - 2) * (x.shape[2] - 2), num_pixels, x.device))
    _check_flags(flag, [pred])
    return keys.cpu().numpy()


def _filter_residuals(fname, filter, num_pixels=None, **kw) -> np.ndarray:
    return _ae_one(fname, _Pred(str(fname), taps=filter_taps(filter)), num_pixels)


def _unet_residuals(fname, model, channels=(3,), num_pixels=None, **kw) -> np.ndarray:
    from .ws.estimate import unet_model_of
    return _ae_one(fname, _Pred("UNet", model=unet_model_of(model)), num_pixels)


# src/error_boxes.py filter_residuals / unet_residuals: one flat array per image (all interior pixels, or `num_pixels` draws).  They
# hold the absolute error: the sign of the residual never reaches the table (filter_mae / unet_mae take np.abs of it).
filter_residuals = fabrika.precovers(iterator="python", convert_to="numpy", ignore_missing=True)(_filter_residuals)
unet_residuals = fabrika.precovers(iterator="python", convert_to=None, ignore_missing=True)(_unet_residuals)


def filter_mae(model: str, channels: typing.Tuple[int], model_name: str, data_path=DATA_PATH, num_pixels: int = None,
               take_num_images: int = None, progress_on: bool = False) -> typing.Dict[str, np.ndarray]:
    """{f'{model_name}_{channels}': AE (images, pixels)} of a named filter over the test split (src/error_boxes.py `filter_mae`)."""
    if tuple(channels) != (3,):
        raise ValueError(f"channels {channels}: the AE is computed on the Y plane, channels (3,)")
    res = filter_residuals(data_path, filter=filters.get_coefficients(model_name), num_pixels=num_pixels, take_num_images=take_num_images,
                           split="split_te.csv", shuffle_seed=12345, progress_on=progress_on)
    return {f"{model_name}_{''.join(map(str, channels))}": np.abs(res)}


def unet_mae(channels, model_name, model_path, data_path=DATA_PATH, num_pixels: int = None, take_num_images: int = None,
             mode: str = None, progress_on: bool = False) -> typing.Dict[str, np.ndarray]:
    """{f'UNet_{channels}': AE (images, pixels)} of a trained UNet over the test split (src/error_boxes.py `unet_mae`)."""
    from .evaluate import get_pretrained
    model = get_pretrained(model_path, channels, model_name=model_name, mode=mode)
    res = unet_residuals(data_path, model=model, channels=channels, num_pixels=num_pixels, take_num_images=take_num_images,
                         split="split_te.csv", shuffle_seed=12345, progress_on=progress_on)
    return {f"UNet_{''.join(map(str, channels))}": np.array([np.abs(r).flatten() for r in res])}


# ---- CLI -------------------------------------------------------------------------------------------------------------------------

def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="the KB-stratified absolute-error box table (results/prediction/ae_boxes_3.csv)")
    ap.add_argument("--data", required=True, help="dataset root with images*/files.csv and the split file (the reference's ../data)")
    ap.add_argument("--out", required=True, help="output CSV (the reference writes results/prediction/ae_boxes_3.csv)")
    ap.add_argument("--model-dir", default=None, help="trained UNets in the reference's layout <dir>/{dropout,LSBR}/<run>/"
                                                      "{config.json,model/best_model.pt.tar}; UNet rows are omitted without it")
    ap.add_argument("--num-pixels", type=int, default=None, help="pixels drawn per image (subset_residual); default: all")
    ap.add_argument("--take-num-images", type=int, default=None)
    ap.add_argument("--split", default="split_te.csv")
    ap.add_argument("--mode", default=None, help="UNet inference mode (default: the package default)")
    ap.add_argument("--progress", action="store_true")
    ap.add_argument("--filters", nargs="*", default=["KB", "AVG"], help="named filters of filters.NAMED_FILTERS; KB, the anchor, must be among them")
    from .ols import add_kernels_argument
    add_kernels_argument(ap)
    return ap.parse_args(argv)


def main(argv=None) -> None:
    a = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    from .ols import register_from_args
    register_from_args(a)
    predictors = {name: name for name in a.filters}
    if a.model_dir:
        from .evaluate import trained_runs
        for method, model_name, config in trained_runs(a.model_dir, UNET_RUNS):
            predictors[f"UNet_{config['loss']}"] = (pathlib.Path(a.model_dir) / method, model_name)
    res = run(a.data, predictors, anchor="KB", split=a.split, take_num_images=a.take_num_images, num_pixels=a.num_pixels, mode=a.mode,
              progress_on=a.progress)
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res.to_csv(out, index=False)
    logging.info(f"output saved to {out}")


if __name__ == "__main__":
    main()
