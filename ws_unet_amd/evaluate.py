"""Predictor / evaluate API of the reference (src/unet/evaluate.py:31-188) on the MI355X model.

Kept verbatim in name, arguments and result layout: `infere_single`, `get_model_name`, `predict_unet`,
`predict_unet_cover`, `predict_unet_stego`, `get_model_config`, `get_pretrained`.  Differences that a
drop-in user should know:
  * the model runs on the GPU; the `device` arguments are accepted for signature compatibility but the
    model's own device is used (there is no CPU path -- the reference hard-wires CPU, evaluate.py:27);
  * `infere_single` runs without building an autograd graph (the reference forgets no_grad, :48);
  * additions: `predict_unet_batch` + `predict_unet_cover_batched` / `predict_unet_stego_batched` evaluate
    whole batches on the device and bring back 8 bytes per image (WS statistic fused in
    wsu_ws_residual_stats), with the same rows / columns / order as the per-image functions.
"""
from __future__ import annotations

import glob
import json
import logging
import pathlib
import typing
from pathlib import Path

import numpy as np
import pandas as pd
import torch

from . import fabrika, ops, planes, unet_run
from .data import get_timm_transform
from .imread import imread4_f32, imread4_u8, u8_plane
from .model import get_model
from .per_image import AHEAD_DEPTH, rows_ahead


def infere_single(
    x: np.ndarray,
    model: typing.Callable,
    device=None,
) -> np.ndarray:
    """(H,W,1) float32 in 0..255  ->  (510,510,1) float32 prediction in 0..255 (evaluate.py:31-52)."""
    parity, demosaic = getattr(model, "side_planes", (False, False))       # the planes the run was trained with (get_pretrained)
    transform = get_timm_transform(
        mean=None, std=None, grayscale=True, parity_oracle=parity, demosaic_oracle=demosaic, post_flip=False, post_rotate=False,
    )
    x_ = transform(x / 255.)[None].to(unet_run.model_device(model))
    with torch.no_grad():
        y_ = unet_run.range_retry(model, lambda: model(x_))
    y = y_.detach().cpu().numpy()[0, 0, 1:-1, 1:-1] * 255.
    return y[..., None]


def get_model_name(
    stego_method: str = "LSBR",
    model_dir: pathlib.Path = pathlib.Path("../models/unet"),
    device=None,
) -> str:
    """The single non-debug run under <model_dir>/<stego_method>/ whose config names `stego_method` and whose
    best checkpoint exists (evaluate.py:55-105).  RuntimeError unless exactly one matches."""
    found = []
    for cfg_file in map(pathlib.Path, glob.glob(str(pathlib.Path(model_dir) / stego_method / "*" / "config.json"))):
        run = cfg_file.parent.name
        with open(cfg_file) as f:
            config = json.load(f)
        try:
            ckpt = torch.load(cfg_file.parent / "model" / "best_model.pt.tar", map_location="cpu", weights_only=True)
        except FileNotFoundError:
            logging.warning(f"no model found for {run}, skipped")
            continue
        if config.get("debug", False):
            logging.warning(f"debug model {run} skipped")
            continue
        alpha = float(config["alpha"]) if config["alpha"] else config["alpha"]
        found.append({
            "model_name": run, "stego_method": config["stego_method"], "alpha": alpha, "loss": config["loss"],
            "network": config["network"], "drop_rate": config["drop_rate"], "epochs": ckpt["epoch"],
        })
    df = pd.DataFrame(found)
    if len(df):
        df = df[df.stego_method == stego_method]
    if len(df) < 1:
        raise RuntimeError(f"no model for {stego_method=} found")
    if len(df) > 1:
        raise RuntimeError(f"multiple models for {stego_method=} found")
    return df["model_name"].iloc[0]


def predict_unet(
    fname: str,
    model: torch.nn.Module,
    *,
    device=None,
    imread: typing.Callable = imread4_f32,
    **kw,
):
    """Per-image WS estimate and MAE (evaluate.py:109-139).  With this package's UNet and a 512x512 image the pixels go up as
    uint8 and only the two statistics come back (wsu_u8_to_unit_f32 -> forward -> wsu_ws_residual_stats, same float32 arithmetic);
    for any other predictor callable the reference's host formulas below are evaluated on its returned array."""
    if isinstance(model, torch.nn.Module) and hasattr(model, "forward_features") and imread is imread4_f32:
        # default reader + this package's UNet: the Y plane is decoded by libwsu_io (zlib + PNG unfilter + cv2's luma in C++, straight into a
        # pinned buffer) instead of PIL -- the same plane `imread4_f32(fname)[..., 3]` holds (tests/test_host_logic.py), 2.5x less host
        # time per image -- and rows announced ahead ride along in this row's launch (per_image.RowsAhead); files the native reader does not
        # take go through the paths below
        hit = rows_ahead.predict(fname, model)
        if hit is not None:
            return {**kw, "beta_hat": hit[0], "l1": hit[1]}
    x = imread(fname)[..., 3:]
    if isinstance(model, torch.nn.Module) and hasattr(model, "forward_features") and x.shape[:2] == (512, 512):
        xi = np.ascontiguousarray(x[..., 0])
        if xi.dtype == np.uint8 or np.array_equal(xi, np.rint(xi)):
            x_u8 = torch.from_numpy(xi.astype(np.uint8))[None].to(unet_run.model_device(model))
            beta, l1, tripped = unet_run.predict_u8_one_readback(x_u8, model)
            if tripped and unet_run.range_fallback(model):
                beta, l1, _ = unet_run.predict_u8_one_readback(x_u8, model)
            return {**kw, "beta_hat": np.float32(beta[0]), "l1": np.float32(l1[0])}
    x_hat = infere_single(x, model=model, device=device)
    x = x[1:-1, 1:-1]
    x_bar = (x.astype("uint8") ^ 1).astype("float32")          # integer LSB flip
    beta_hat = np.mean((x - x_bar) * (x - x_hat))
    l1_hat = np.mean(np.abs(x - x_hat))
    return {**kw, "beta_hat": beta_hat, "l1": l1_hat}


def _predict_unet_cover(*args, **kw):
    return predict_unet(*args, **kw)


def _predict_unet_stego(*args, **kw):
    return predict_unet(*args, **kw)


_predict_unet_cover.lookahead = _predict_unet_stego.lookahead = rows_ahead.announce
_predict_unet_cover.lookahead_reset = _predict_unet_stego.lookahead_reset = rows_ahead.reset
_predict_unet_cover.lookahead_depth = _predict_unet_stego.lookahead_depth = AHEAD_DEPTH
predict_unet_cover = fabrika.precovers(iterator="python", convert_to="pandas", ignore_missing=False, n_jobs=-1)(_predict_unet_cover)
predict_unet_stego = fabrika.stego_spatial(iterator="python", convert_to="pandas", ignore_missing=False, n_jobs=-1)(_predict_unet_stego)


# ---- batched device path ------------------------------------------------------------------------------


def submit_unet_batch(fnames, *, model: torch.nn.Module, imread: typing.Callable = imread4_u8, prefetched=None):
    """First half of predict_unet_batch: upload + launch, nothing waits for the GPU.  Returns a handle for collect_unet_batch
    (ragged / non-512 chunks go through the per-image path right here and the handle carries their rows)."""
    u8 = prefetched[0] if prefetched is not None else planes.load_planes_u8(fnames, imread)
    if u8 is None or tuple(u8.shape[1:]) != (512, 512):
        # not the planes the batched forward takes (check_unet_geometry): only the per-image path defines what happens then
        res = [predict_unet(f, model, imread=imread4_f32) for f in fnames]
        return ("host", np.array([[r["beta_hat"], r["l1"]] for r in res], dtype=np.float32))
    beta, l1 = unet_run.predict_u8_batch(planes.upload_planes(u8, unet_run.model_device(model)), model)
    return ("device", torch.stack([beta, l1], dim=1))


def collect_unet_batch(handle) -> np.ndarray:
    """Second half: (N, 2) float32 rows [beta_hat, l1] of a submitted chunk (waits for that chunk only)."""
    kind, val = handle
    return val if kind == "host" else val.cpu().numpy()


def _submit_unet_rows(fnames, kws, *, model: torch.nn.Module, imread: typing.Callable = imread4_u8, prefetched=None, **_ignored):
    return submit_unet_batch(fnames, model=model, imread=imread, prefetched=prefetched), kws


def _collect_unet_rows(handle):
    rows = collect_unet_batch(handle[0])
    return [{**kw, "beta_hat": rows[i, 0], "l1": rows[i, 1]} for i, kw in enumerate(handle[1])]


def predict_unet_batch(fnames, kws, *, model: torch.nn.Module, imread: typing.Callable = imread4_u8, device=None,
                       prefetched=None, **_ignored):
    """Batched predict_unet for `fabrika` iterator='batched': one result dict per (fname, kw).  `prefetched`: the planes of
    this chunk if the iterator already decoded them (load_planes_u8 run one chunk ahead).  Its submit / collect halves let the
    iterator launch chunk k+1 before it reads chunk k back."""
    return _collect_unet_rows(_submit_unet_rows(fnames, kws, model=model, imread=imread, prefetched=prefetched))


predict_unet_batch.submit, predict_unet_batch.collect = _submit_unet_rows, _collect_unet_rows


def _prefetch_planes(fnames, kws):
    """Decode of the next chunk beside the GPU work of the current one (fabrika iterator='batched'); a 1-tuple so that "ragged chunk"
    (None) stays distinguishable from "nothing prefetched"."""
    return (planes.load_planes_u8(fnames, kws[0].get("imread", imread4_u8)),)


def _range_guarded(iterate):
    """A data-set pass of a batched driver, then ONE look at the model's range flag: if a planar forward of the pass left the format's
    full-accuracy range, the whole pass is recomputed in 'bf16x3s' (loudly).  No per-chunk synchronisation."""
    def run(dataset, *args, **kw):
        return unet_run.range_retry(kw.get("model"), lambda: iterate(dataset, *args, **kw))
    run.__doc__ = iterate.__doc__
    return run


def _batched_pass(rows_of, fn):
    """fn over the chunks of `rows_of`'s rows (fabrika.precovers / stego_spatial), the model and reader taken out of the row kwargs."""
    return _range_guarded(rows_of(iterator="batched", convert_to="pandas", ignore_missing=False)(
        fabrika.shared_kwargs(fn, ("model", "imread", "device"), _prefetch_planes)))


predict_unet_cover_batched = _batched_pass(fabrika.precovers, predict_unet_batch)
predict_unet_stego_batched = _batched_pass(fabrika.stego_spatial, predict_unet_batch)


# ---- prediction error with the HILL-cost weighted MAE (src/predictor_error.py:19-76 `attack`): mae and wmae per image ------------------------
# A separate chain beside the WS statistics above: u8 -> /255 -> forward -> HILL cost (K12) -> 10 % quantile (K13) -> mae / wmae (K14).
# predict_unet / predict_u8_batch and what they return are untouched.

_ERROR_ROW = {"filter": "UNet", "model": "gray", "inbayer": "", "information": "Unconditional"}     # the constant fields of attack's row



def _u8_error_rows(x_u8: torch.Tensor, model: torch.nn.Module):
    """predict_u8_error_batch + one look at the range flag (recompute in 'bf16x3s' if a planar forward left its range): numpy (mae, wmae)."""
    mae, wmae = unet_run.range_retry(model, lambda: unet_run.predict_u8_error_batch(x_u8, model))
    return mae.cpu().numpy(), wmae.cpu().numpy()


def predict_unet_error(fname: str, model: torch.nn.Module, *, imread: typing.Callable = imread4_f32, channels=(3,), demosaic=None, **kw):
    """Per-image row of src/predictor_error.py:19-76 `attack` for the UNet: mae and wmae (the MAE over the 10 % of interior pixels
    with the lowest HILL cost; the reference takes HILL from stegolab2.hill.compute_rho, here the textbook cost of ws_unet_amd.hill,
    the one filters.csv pins).  The row leads with the fabrika row fields (name, height, width)."""
    x = u8_plane(np.asarray(imread(fname))[..., channels[0]], "the HILL cost is defined on 8-bit pixel values")
    mae, wmae = _u8_error_rows(torch.from_numpy(x)[None].to(unet_run.model_device(model)), model)
    return {**kw, "demosaic": demosaic, **_ERROR_ROW, "mae": float(mae[0]), "wmae": float(wmae[0]),
            "channels": "".join(map(str, channels))}


predict_unet_error_cover = fabrika.precovers(iterator="python", convert_to="pandas", ignore_missing=False)(predict_unet_error)
predict_unet_error_stego = fabrika.stego_spatial(iterator="python", convert_to="pandas", ignore_missing=False)(predict_unet_error)


def predict_unet_error_batch(fnames, kws, *, model: torch.nn.Module, imread: typing.Callable = imread4_u8, prefetched=None, **_ignored):
    """Batched predict_unet_error for fabrika iterator='batched' (Y plane): the chunk's planes come from load_planes_u8 (pinned buffer,
    decoded one chunk ahead when the iterator prefetches), go up as uint8 and run as one launch chain; ragged chunks go per image."""
    u8 = prefetched[0] if prefetched is not None else planes.load_planes_u8(fnames, imread)
    if u8 is None:
        return [predict_unet_error(f, model, **kw) for f, kw in zip(fnames, kws)]
    mae, wmae = unet_run.predict_u8_error_batch(planes.upload_planes(u8, unet_run.model_device(model)), model)
    mae, wmae = mae.cpu().numpy(), wmae.cpu().numpy()
    return [{**kw, "demosaic": None, **_ERROR_ROW, "mae": float(mae[i]), "wmae": float(wmae[i]), "channels": "3"} for i, kw in enumerate(kws)]


predict_unet_error_cover_batched = _batched_pass(fabrika.precovers, predict_unet_error_batch)
predict_unet_error_stego_batched = _batched_pass(fabrika.stego_spatial, predict_unet_error_batch)


def get_model_config(model_dir: pathlib.Path, stego_method: str, model_name: str) -> typing.Dict[str, typing.Any]:
    with open(pathlib.Path(model_dir) / stego_method / model_name / "config.json") as f:
        return json.load(f)


def trained_runs(model_dir, stego_methods):
    """(stego method, model_name, config) of the one trained run of each method under `model_dir`, found as the method is reached."""
    for method in stego_methods:
        model_name = get_model_name(stego_method=method, model_dir=pathlib.Path(model_dir))
        yield method, model_name, get_model_config(model_dir=model_dir, stego_method=method, model_name=model_name)


def get_pretrained(
    model_path,
    channels,
    *,
    model_name: str = None,
    device=None,
    mode: str = None,
):
    """Build the network named in <model_path>/<model_name>/config.json and load model/best_model.pt.tar
    (evaluate.py:162-188).  `channels` is accepted and ignored like in the reference.  Unlike the reference (which hard-codes one input
    plane) a run whose config sets `parity_oracle` / `demosaic_oracle` gets the input planes it was trained with; `model.side_planes`
    tells the evaluation drivers to build them (unet_plane, infere_single)."""
    model_path = Path(model_path)
    with open(model_path / model_name / "config.json") as f:
        config = json.load(f)
    dev = torch.device(device) if device is not None and torch.device(device).type == "cuda" else unet_run.DEVICE
    sides = (bool(config.get("parity_oracle", False)), bool(config.get("demosaic_oracle", False)))
    model = get_model(config["network"], in_channels=ops.side_plane_count(*sides), out_channels=1, channel=[0], drop_rate=0., mode=mode).to(dev)
    model.side_planes = sides
    checkpoint = torch.load(model_path / model_name / "model" / "best_model.pt.tar", map_location=dev, weights_only=True)
    model.load_state_dict(checkpoint["state_dict"])
    logging.info(f"model {model_name} loaded")
    return model


# ---- whole-dataset evaluate, batch-sharded over the ranks of a torch.distributed job -----------------------------

@fabrika.precovers(iterator=None, convert_to=None, ignore_missing=False)
def _cover_rows(df, **kw):
    return df


@fabrika.stego_spatial(iterator=None, convert_to=None, ignore_missing=False)
def _stego_rows(df, **kw):
    return df


def predict_unet_sharded(dataset, model: torch.nn.Module, *, stego_method: str = None, alpha: float = None, batch_size: int = 32,
                         **kw_iter) -> pd.DataFrame:
    """`predict_unet_cover` (stego_method None) / `predict_unet_stego` over a data set with the rows split contiguously over the
    ranks: every rank decodes and predicts its shard in batches, `(beta_hat, l1)` rows are all-gathered and every
    rank returns the full table in fabrika order with the per-image functions' columns.  Single process: same result, no
    collective."""
    from . import parallel
    dataset = pathlib.Path(dataset)
    if stego_method is None:
        df = _cover_rows(dataset, **kw_iter)
    else:
        kw = {"stego_method": stego_method, **({"alpha": alpha} if alpha is not None else {})}
        df = _stego_rows(dataset, **kw, **kw_iter)
    df = df.reset_index(drop=True)
    files = df["name"].tolist()                              # iterator=None hands over absolute paths (fabrika.py:104-110)

    def predict_shard(shard_files):                          # decode / GPU / read-back of consecutive chunks overlapped
        chunks = [shard_files[i:i + batch_size] for i in range(0, len(shard_files), batch_size)]
        rows = list(fabrika.pipeline(chunks, lambda ch: (planes.load_planes_u8(ch),), lambda ch, staged: submit_unet_batch(ch, model=model, prefetched=staged),
                                     collect_unet_batch))
        return torch.from_numpy(np.concatenate(rows)) if rows else torch.zeros((0, 2), dtype=torch.float32)

    # one look per pass, OR-ed over the ranks: everybody recomputes together
    table = unet_run.range_retry(model, lambda: parallel.evaluate_sharded(files, predict_shard, None), collective=True).cpu().numpy()
    df["name"] = [str(pathlib.Path(f).relative_to(dataset)) for f in files]
    df["beta_hat"], df["l1"] = table[:, 0], table[:, 1]
    if stego_method is not None:
        df = df.assign(stego_method=stego_method, **({"alpha": alpha} if alpha is not None else {}))
    return df


def main(argv=None) -> None:
    """The reference's `python unet/evaluate.py` (evaluate.py:190-233): covers + LSBR + HILLR stego rows of one trained model
    -> results/estimation/ws_<stego_method>.csv; run under torch.distributed.run to shard the rows over GPUs."""
    import argparse
    from . import parallel
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--data", default="../data")
    ap.add_argument("--model-dir", default="../models/unet")
    ap.add_argument("--stego-method", default="HILLR", help="which trained model: dropout | LSBR | HILLR")
    ap.add_argument("--eval-methods", nargs="*", default=["LSBR", "HILLR"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--mode", default=None)
    ap.add_argument("--u8-shards", default=None, help="directory of pre-decoded uint8 shards (written on first use by rank 0): the passes copy rows "
                                                       "out of memory-mapped .npy files instead of decoding PNGs")
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    rank, world = parallel.init_from_env()
    model_dir = pathlib.Path(a.model_dir)
    model_name = get_model_name(model_dir=model_dir, stego_method=a.stego_method)
    model = get_pretrained(model_path=model_dir / a.stego_method, channels=(3,), model_name=model_name, mode=a.mode)
    if a.u8_shards:
        sd = pathlib.Path(a.u8_shards)
        if rank == 0 and not (sd / "index.json").exists():
            rows = [_cover_rows(pathlib.Path(a.data))] + [_stego_rows(pathlib.Path(a.data), stego_method=sm) for sm in a.eval_methods]
            planes.write_u8_shards([f for df_ in rows for f in df_["name"].tolist()], sd)
        if world > 1:
            torch.distributed.barrier()
        logging.info("u8 shards: %d files indexed", planes.use_u8_shards(sd))
    import time
    t0 = time.perf_counter()
    frames = [predict_unet_sharded(a.data, model, batch_size=a.batch_size)]
    dt = time.perf_counter() - t0
    if rank == 0:                                             # the host budget of a file-fed pass, stated once (no pass is repeated for it)
        nfiles = len(frames[0])
        rate = nfiles / world / dt if dt > 0 else None
        b = planes.decode_budget([str(pathlib.Path(a.data) / n) for n in frames[0]["name"].tolist()], gpu_images_per_s=None)
        logging.info("evaluate: %d covers in %.2f s = %.0f images/s per rank end to end; PNG decode %.2f ms per image and thread, %d decode threads "
                     "per rank (usable cores %d / %d ranks on this node)%s", nfiles, dt, rate or 0.0, b["decode_ms_per_image_per_thread"] or 0.0,
                     b["decode_threads_used"], b["usable_cores"], b["local_world_size"], "; rows served from u8 shards" if a.u8_shards else "")
        if rate and b["decode_ms_per_image_per_thread"] and not a.u8_shards:
            busy = rate * b["decode_ms_per_image_per_thread"] / 1e3 / max(1, b["decode_threads_used"])
            if busy > 0.8:
                logging.warning("evaluate: the decode threads were ~%.0f %% busy at this rate: the pass is host-bound (see --u8-shards)", busy * 100)
    for sm in a.eval_methods:
        frames.append(predict_unet_sharded(a.data, model, stego_method=sm, batch_size=a.batch_size))
    df = pd.concat(frames)
    if rank == 0:
        out = pathlib.Path(a.out or f"../results/estimation/ws_{a.stego_method}.csv")
        out.parent.mkdir(parents=True, exist_ok=True)
        df.to_csv(out, index=False)
        logging.info(f"output saved to {out}")


if __name__ == "__main__":
    main()
