"""Weighted-stego (WS) payload estimator -- the caller of the UNet predictor (reference src/ws/estimate.py).

Same names and arguments: NAMED_FILTERS, attack (:55-136), attack_cover / attack_stego (:139-146), run (:149-205).
The statistic itself (local variance weights, LSB-flip residual product, clipping, bias correction) is ONE libwsu
kernel, wsu_ws_attack; there is no host implementation in this package.

  * `attack(fname, channels, pixel_estimator, ...)` is the per-image drop-in.  A `UNetEstimator` (what
    `get_unet_estimator` returns) keeps the prediction on the device; a `filters.FilterEstimator` is evaluated inside
    the kernel; any other callable is called on the host like in the reference and its (H-2,W-2,1) result uploaded.
  * `attack_batch` / `attack_cover_batched` / `attack_stego_batched` run whole batches (fabrika iterator='batched'):
    threaded PNG decode -> one u8 upload -> UNet forward(s) -> statistic -> 4 bytes per image back.
  * the model names of `structural.NAMES` ('SPA', 'RS') are no pixel predictors but whole estimators of their own (ws/structural.py:
    an exact count kernel and a float64 solve); they go through the same drivers, unweighted and without bias correction.
  * `placement='sequential'` (with `order='rows'` or 'rows_up') replaces the statistic by the changepoint estimator for payloads written
    into the first pixels of the file order (ws/sequential.py, wsu_ws_sequential): every pixel predictor works, the structural
    estimators, weighted=-1 and correct_bias do not.  The default, placement='random', is the reference's statistic.
  * `placement='adaptive'` (with `criterion='hill'` and `flip_rate`) is the changepoint estimator along the order of an adaptivity
    criterion recomputed from the image under attack (ws/adaptive.py, wsu_ws_ordered), for HILLR-style payloads; options as 'sequential'.
  * the model name 'JPEG' (ws/jpeg.py, a `jpeg.JPEGEstimator`) predicts every image by its own round trip through the JPEG quantiser it
    was once compressed with: a full-frame device prediction like a UNet's, for both placements, without bias correction.
  * `run(..., batched=True)` is `run` on the batched iterators; the joblib iterators of the reference (:139,144) cannot
    carry a GPU model into worker processes, so the per-image decorators use iterator='python'.

Numerics: the reference's `scipy.signal.convolve` takes its FFT branch for a 512x512 plane, so its mu / mu2 carry float32
FFT noise (~1e-2 absolute on mu2); the kernel evaluates the nine taps directly (exact for the default AVG kernel on
uint8 pixels).  Agreement with the reference is therefore to that noise level (tests/golden/ws_attack.npz, rel 2e-4).
"""
from __future__ import annotations

import pathlib
import typing

import numpy as np
import torch

from .. import fabrika, filters, ops
from ..imread import imread4_u8, u8_plane
from ..planes import decode_pool, load_planes_u8, upload_planes
from ..unet_run import check_unet_geometry, model_device, unet_plane
from . import adaptive, jpeg, predictors, sequential, structural

NAMED_FILTERS = filters.NAMED_FILTERS_2D


class UNetEstimator:
    """`predict(x (H,W,1) float32 0..255) -> (H-2,W-2,1)` closure of src/unet/__init__.py:110-121 as an object: callable
    like the reference's, and `.model` lets `attack` / `attack_batch` keep the prediction on the device."""

    def __init__(self, model):
        self.model = model

    def __call__(self, x: np.ndarray) -> np.ndarray:
        from ..evaluate import infere_single
        return infere_single(x, model=self.model)

    def device_arguments(self, x_u8: torch.Tensor, correct_bias: bool = False) -> dict:
        """The statistic kernels' keywords (`predictor_arguments`): the full-frame output stays on the device, scale 255; with
        correct_bias also the network applied to x_bar - x."""
        check_unet_geometry(x_u8.shape[1:], "the UNet estimator")
        y, yb = _unet_planes(self.model, x_u8, correct_bias)
        return dict(x_hat=y, hat_scale=255.0) | ({"x_bias": yb} if correct_bias else {})

    def __reduce__(self):
        # the reference ships its CPU predictor into joblib / loky workers (ws/estimate.py:139); a GPU model must not travel
        raise TypeError("UNetEstimator holds GPU state and cannot be pickled into worker processes: "
                        "use the fabrika iterators 'python' or 'batched' (ws.estimate.attack_cover / attack_cover_batched)")


# ---- what a predictor is: a filters.FilterEstimator, a UNet (a UNetEstimator, or for some drivers a bare model or the (model_path,
# model_name) of a trained run), or any other callable, run on the host like the reference's ----------------------------------------

def unet_model_of(predictor):
    """The UNet whose forward a driver runs on the device for this predictor (a UNetEstimator's, or a bare model), or None.
    (Where a predictor's planes go is unet_run.model_device of it: the UNet's device, the default GPU for None.)"""
    if isinstance(predictor, UNetEstimator):
        return predictor.model
    return predictor if isinstance(predictor, torch.nn.Module) else None


def as_unet_estimator(unet, mode: str = None):
    """None | UNetEstimator | model | (model_path, model_name) of a trained run (loaded in inference `mode`) -> UNetEstimator (None: None)."""
    if unet is None or isinstance(unet, UNetEstimator):
        return unet
    if isinstance(unet, torch.nn.Module):
        return UNetEstimator(unet)
    if isinstance(unet, tuple) and len(unet) == 2:
        from .. import get_unet_estimator
        return get_unet_estimator(model_path=unet[0], model_name=unet[1], channels=(3,), mode=mode)
    raise ValueError(f"unet: a UNetEstimator, a model or (model_path, model_name), got {type(unet).__name__}")


def _as_u8_plane(x: np.ndarray) -> np.ndarray:
    """First channel of the processed image as uint8; the LSB flip is only defined for integer pixel values."""
    return u8_plane(np.asarray(x)[..., 0], "WS attack needs integer pixel values in 0..255")


def _unet_planes(model, x_u8: torch.Tensor, correct_bias: bool):
    """Full-frame network outputs in [0,1] for x and (if needed) for x_bar - x (estimate.py:89,127)."""
    if correct_bias and any(getattr(model, "side_planes", (False, False))):
        raise NotImplementedError("bias correction (correct_bias=True, the network applied to x_bar - x) is not defined for a network "
                                  "whose input contains the parity of that difference image")
    y = unet_plane(model, x_u8)
    with torch.no_grad():
        yb = model(ops.lsb_delta_unit(x_u8)[:, None])[:, 0].contiguous() if correct_bias else None
    return y, yb


def predictor_arguments(x_u8: torch.Tensor, pixel_estimator, host_planes=None, correct_bias: bool = False) -> dict:
    """A pixel predictor as the keywords the statistic kernels take (ops.ws_attack, ops.ws_sequential, ops.ws_residual_accumulate): what
    its `device_arguments(x_u8, correct_bias)` returns, if it has that method -- every estimator listed in ws/predictors.py and the
    UNetEstimator do: `pixel_filter` (evaluated in the kernel), or a full-frame `x_hat` with its `hat_scale` and, with correct_bias, the
    `x_bias` plane of the predictor applied to x_bar - x.  Any other callable is called on `host_planes` in the reference's call pattern,
    one image at a time: `x_hat` (and `x_bias`) in interior layout, scale 1."""
    if hasattr(pixel_estimator, "device_arguments"):
        return pixel_estimator.device_arguments(x_u8, correct_bias)
    if host_planes is None:
        raise ValueError(f"a host predictor ({type(pixel_estimator).__name__}) needs the planes on the host (host_planes)")
    hats, biases = [], []
    for xf in host_planes:
        h = np.asarray(pixel_estimator(xf), dtype=np.float32)
        if h.shape[:2] != (xf.shape[0] - 2, xf.shape[1] - 2):
            raise ValueError(f"pixel_estimator returned {h.shape} for an image of {xf.shape}")
        hats.append(h[..., 0])
        if correct_bias:
            xbar = (xf.astype(np.uint8) ^ 1).astype(np.float32)
            biases.append(np.asarray(pixel_estimator(xbar - xf), dtype=np.float32)[..., 0])
    kw = dict(x_hat=torch.from_numpy(np.stack(hats)).to(x_u8.device), hat_scale=1.0)
    return kw | ({"x_bias": torch.from_numpy(np.stack(biases)).to(x_u8.device)} if correct_bias else {})


def _weights(mean_estimator, weighted) -> dict:
    """The weights as the keywords the statistic kernels take: the reference's mean estimator as a kernel array, and `weighted`."""
    return dict(mean_filter=np.asarray(mean_estimator)[..., ::-1], weighted=int(weighted))


def _changepoint(x_u8: torch.Tensor, pixel_estimator, mean_estimator, weighted, order, host_planes=None, return_curve=False, pred=None):
    """ops.ws_sequential's (k, t_max, t_all[, curve]) on the device for a batch of planes, with any pixel predictor `_stat` knows
    (pred: its predictor_arguments, where the caller has made them)."""
    pred = predictor_arguments(x_u8, pixel_estimator, host_planes) if pred is None else pred
    return ops.ws_sequential(x_u8, order=order, return_curve=return_curve, **_weights(mean_estimator, weighted), **pred)


def _stat(x_u8: torch.Tensor, pixel_estimator, mean_estimator, weighted, correct_bias, host_planes=None, placement="random",
          order="rows", criterion="hill", flip_rate=1.0) -> torch.Tensor:
    """beta_hat[N] on the device for a batch of planes."""
    _check_options(pixel_estimator, weighted, correct_bias, placement, order, criterion, flip_rate)
    if isinstance(pixel_estimator, structural.StructuralEstimator):    # no predictor, no weights: the estimator is the statistic
        structural.require_unweighted(weighted, correct_bias)
        return pixel_estimator.beta(x_u8).to(torch.float32)
    pred = predictor_arguments(x_u8, pixel_estimator, host_planes, correct_bias)
    if placement == "sequential":                                      # the changepoint k -> the change rate of the whole plane
        k = _changepoint(x_u8, pixel_estimator, mean_estimator, weighted, order, pred=pred)[0]
        beta = sequential.beta(k, x_u8.shape[1], x_u8.shape[2], order).to(torch.float32)
    elif placement == "adaptive":                                      # the changepoint along the recomputed cost order
        k = ops.ws_ordered(x_u8, adaptive.path_for(x_u8, criterion), flip_rate=flip_rate, **_weights(mean_estimator, weighted), **pred)[0]
        beta = adaptive.beta(k, x_u8.shape[1], x_u8.shape[2], flip_rate).to(torch.float32)
    else:
        beta = ops.ws_attack(x_u8, correct_bias=correct_bias, **_weights(mean_estimator, weighted if abs(int(weighted)) == 1 else 0), **pred)
    return jpeg.without_estimate(beta, pred["x_hat"]) if isinstance(pixel_estimator, jpeg.JPEGEstimator) else beta


def _check_options(pixel_estimator, weighted, correct_bias, placement="random", order="rows", criterion="hill", flip_rate=1.0) -> None:
    """An option an estimator does not have is the caller's error, not an image without an estimate (`attack` turns a ValueError of
    the statistic into beta_hat = None, as the reference does)."""
    sequential.check_placement(placement, order)
    jpeg.require_no_bias_correction(pixel_estimator, correct_bias)
    if placement == "adaptive":
        adaptive.check_options(criterion, flip_rate)
    if placement in ("sequential", "adaptive"):
        if isinstance(pixel_estimator, structural.StructuralEstimator):
            raise ValueError(f"placement={placement!r} needs a pixel predictor; the structural estimators {structural.NAMES} have none")
        if int(weighted) not in (0, 1) or correct_bias:
            raise ValueError(f"placement={placement!r} takes weighted 0 or 1 and correct_bias=False, got weighted={weighted} "
                             f"correct_bias={correct_bias}")
    elif isinstance(pixel_estimator, structural.StructuralEstimator):
        structural.require_unweighted(weighted, correct_bias)


def _placement_tail(placement, order, criterion="hill", flip_rate=1.0) -> dict:
    """The row columns of a placement other than the default: existing tables keep their columns."""
    if placement == "adaptive":
        return {"placement": placement, "criterion": criterion, "flip_rate": flip_rate}
    return {} if placement == "random" else {"placement": placement, "order": order}


def attack(
    fname: str,
    channels: typing.List[int],
    pixel_estimator: typing.Union[np.ndarray, typing.Callable],
    mean_estimator: np.ndarray = NAMED_FILTERS["AVG"],
    correct_bias: bool = False,
    weighted: bool = 1,
    imread: typing.Callable = None,
    process_image: typing.Callable = None,
    placement: str = "random",
    order: str = "rows",
    criterion: str = "hill",
    flip_rate: float = 1.0,
    **kw,
) -> dict:
    """WS estimate of one image (estimate.py:55-136): returns kw | {beta_hat, channels, weighted, correct_bias}; with
    placement='sequential' the changepoint estimate of ws/sequential.py, and the row also says placement and order; with
    placement='adaptive' that of ws/adaptive.py, and the row says placement, criterion and flip_rate."""
    _check_options(pixel_estimator, weighted, correct_bias, placement, order, criterion, flip_rate)
    x = process_image(imread(fname))                         # x_bar = process(x ^ 1) is formed on the device
    try:
        x_u8 = torch.from_numpy(_as_u8_plane(x))[None].to(model_device(unet_model_of(pixel_estimator)))
        beta_hat = _stat(x_u8, pixel_estimator, mean_estimator, weighted, correct_bias, host_planes=[x], placement=placement,
                         order=order, criterion=criterion, flip_rate=flip_rate)[0].item()
        beta_hat = np.float32(beta_hat)
    except ValueError:                                      # estimate.py:122-123
        beta_hat = None
    return kw | {
        "beta_hat": beta_hat,
        "channels": "".join(map(str, channels)),
        "weighted": weighted,
        "correct_bias": correct_bias,
    } | _placement_tail(placement, order, criterion, flip_rate)


@fabrika.precovers(iterator="python", ignore_missing=True)
def attack_cover(*args, **kw):
    return attack(*args, **kw)


@fabrika.stego_spatial(iterator="python", ignore_missing=True)
def attack_stego(*args, **kw):
    return attack(*args, **kw)


# ---- batched device path ------------------------------------------------------------------------------

def _native_planes_ok(channels, pixel_estimator, imread, process_image) -> bool:
    """The default gray pipeline (Y plane, built-in predictor) needs no host arrays: native batched decode -> pinned buffer -> device."""
    builtin = hasattr(pixel_estimator, "device_arguments") or isinstance(pixel_estimator, structural.StructuralEstimator)
    plain = process_image is None or getattr(process_image, "plane_selector", None) == (3,)
    return builtin and imread is imread4_u8 and plain and tuple(channels) == (3,)


def attack_batch(fnames, kws, *, channels, pixel_estimator, mean_estimator=NAMED_FILTERS["AVG"], correct_bias=False,
                 weighted=1, imread=imread4_u8, process_image=None, prefetched=None, placement="random", order="rows", criterion="hill",
                 flip_rate=1.0, **_ignored):
    """`attack` for a chunk of files (fabrika iterator='batched'): one result dict per (fname, kw)."""
    _check_options(pixel_estimator, weighted, correct_bias, placement, order, criterion, flip_rate)
    if _native_planes_ok(channels, pixel_estimator, imread, process_image):
        u8 = prefetched[0] if prefetched is not None else load_planes_u8(fnames, imread)
        planes = None if u8 is None else [None] * len(fnames)
    else:
        process_image = process_image or filters.get_processor_2d(channels)
        planes = list(decode_pool().map(lambda f: process_image(imread(f)), fnames))
        u8 = None
        if len({p.shape for p in planes}) != 1:
            planes = None
    if planes is None:
        process_image = process_image or filters.get_processor_2d(channels)
        return [attack(f, channels, pixel_estimator, mean_estimator, correct_bias, weighted, imread, process_image, placement, order,
                       criterion, flip_rate, **kw) for f, kw in zip(fnames, kws)]
    try:
        if u8 is None:
            u8 = torch.from_numpy(np.stack([_as_u8_plane(p) for p in planes]))
        x_u8 = upload_planes(u8, model_device(unet_model_of(pixel_estimator)))
        beta = _stat(x_u8, pixel_estimator, mean_estimator, weighted, correct_bias, host_planes=planes, placement=placement,
                     order=order, criterion=criterion, flip_rate=flip_rate).cpu().numpy()
    except ValueError:
        beta = [None] * len(fnames)
    tail = {"channels": "".join(map(str, channels)), "weighted": weighted, "correct_bias": correct_bias}
    tail |= _placement_tail(placement, order, criterion, flip_rate)
    return [kw | {"beta_hat": beta[i]} | tail for i, kw in enumerate(kws)]


_ATTACK_KEYS = ("channels", "pixel_estimator", "mean_estimator", "correct_bias", "weighted", "imread", "process_image", "placement", "order",
                "criterion", "flip_rate")


def _prefetch_native(fnames, kws):
    k0 = kws[0]
    if not _native_planes_ok(k0["channels"], k0["pixel_estimator"], k0.get("imread", imread4_u8), k0.get("process_image")):
        return None
    return (load_planes_u8(fnames, imread4_u8),)


attack_cover_batched = fabrika.precovers(iterator="batched", ignore_missing=True)(fabrika.shared_kwargs(attack_batch, _ATTACK_KEYS, _prefetch_native))
attack_stego_batched = fabrika.stego_spatial(iterator="batched", ignore_missing=True)(fabrika.shared_kwargs(attack_batch, _ATTACK_KEYS, _prefetch_native))


def resolve_predictor(model_name: str, model_path, channels):
    """A model name as (estimator, the name its rows carry): a name of ws/predictors.py under itself, any other as the trained UNet run
    `model_name` under `model_path`, whose rows are named 'UNet'."""
    estimator = predictors.by_name(model_name)
    if estimator is not None:
        return estimator, model_name
    from .. import get_unet_estimator
    return get_unet_estimator(model_path=model_path, model_name=model_name, channels=channels), "UNet"


def run(
    input_dir: pathlib.Path,
    stego_method: str,
    alpha: float,
    model_name: str,
    model_path: str,
    channels: typing.Tuple[int],
    imread: typing.Callable = imread4_u8,
    batched: bool = False,
    **kw,
):
    """WS attack over a data set with a named linear filter or a trained UNet as the pixel predictor (estimate.py:149-205), or one of
    the structural estimators of ws/structural.py ('SPA', 'RS': weighted=0, correct_bias=False) in the same rows.  placement='sequential'
    (with order='rows' / 'rows_up') among the keywords: the changepoint estimator of ws/sequential.py with the same predictors;
    placement='adaptive' (with criterion='hill' and flip_rate): the one of ws/adaptive.py along the recomputed cost order."""
    process_cover = filters.get_processor_2d(channels=channels)
    placed = (kw.get("placement", "random"), kw.get("order", "rows"), kw.get("criterion", "hill"), kw.get("flip_rate", 1.0))
    _check_options(None, kw.get("weighted", 1), kw.get("correct_bias", False), *placed)
    pixel_estimator, model_name = resolve_predictor(model_name, model_path, channels)
    _check_options(pixel_estimator, kw.get("weighted", 1), kw.get("correct_bias", False), *placed)
    if stego_method:
        fn = attack_stego_batched if batched else attack_stego
        kw_attack = {"stego_method": stego_method, "alpha": alpha}
    else:
        fn = attack_cover_batched if batched else attack_cover
        kw_attack = {}
    res = fn(
        input_dir,
        inbayer=None,
        **kw_attack,
        pixel_estimator=pixel_estimator,
        mean_estimator=NAMED_FILTERS["AVG"],
        model_name=model_name,
        channels=channels,
        process_image=process_cover,
        imread=imread,
        **kw,
    )
    res["channels"] = "".join(map(str, channels))
    res = res[~res.beta_hat.isna()]
    return res


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--data", default="../data/")
    ap.add_argument("--model-dir", default="../models/unet")
    ap.add_argument("--train-method", default="LSBR", help="stego method the l1ws UNet was trained on")
    ap.add_argument("--stego-methods", nargs="*", default=["LSBR"])
    ap.add_argument("--alphas", nargs="*", type=float, default=[.4, .2, .1])
    ap.add_argument("--filters", nargs="*", default=["AVG", "KB"],
                    help=predictors.filters_help(structural=True) + " (these with --weighted 0)")
    ap.add_argument("--losses", nargs="*", default=["l1", "l1ws"])
    ap.add_argument("--weighted", type=int, default=0)
    ap.add_argument("--correct-bias", action="store_true")
    ap.add_argument("--per-image", action="store_true", help="use the per-image iterators instead of the batched ones")
    ap.add_argument("--placement", choices=sequential.PLACEMENTS, default="random",
                    help="where the payload is assumed to lie: spread uniformly (the WS statistic), in the first pixels of the file order, or "
                         "in the pixels of lowest cost under --criterion, recomputed from each image under attack")
    ap.add_argument("--order", choices=sequential.ORDERS, default="rows", help="sequential placement: rows from the top, or from the bottom")
    ap.add_argument("--criterion", choices=adaptive.CRITERIA, default="hill", help="adaptive placement: the cost that orders the pixels")
    ap.add_argument("--flip-rate", type=float, default=1.0,
                    help="adaptive placement: the probability that a used pixel was flipped (1: HILLR flips every used pixel; 0.5: a real message)")
    ap.add_argument("--out", default=None)
    predictors.add_arguments(ap)
    return ap.parse_args(argv)


def main(argv=None) -> None:
    """The reference's `python ws/estimate.py` (estimate.py:208-275): WS estimates of the covers and of the stego images at
    alpha 0.4 / 0.2 / 0.1 with the AVG and KB filters and with the trained UNets ('l1' = dropout run, 'l1ws' = the run trained on
    --train-method), one table -> results/estimation/ws_<train-method>.csv."""
    import pandas as pd
    from .. import get_model_name
    a = parse_args(argv)
    predictors.register_from_args(a)
    model_dir = pathlib.Path(a.model_dir)
    settings = [(None, .0)] + [(sm, al) for sm in a.stego_methods for al in a.alphas]
    common = dict(demosaic=None, channels=(3,), correct_bias=a.correct_bias, weighted=a.weighted, batched=not a.per_image)
    if a.placement == "adaptive":
        common |= dict(placement=a.placement, criterion=a.criterion, flip_rate=a.flip_rate)
    elif a.placement != "random":
        common |= dict(placement=a.placement, order=a.order)
    res = []
    for stego_method, alpha in settings:
        for model_name in a.filters:
            res.append(run(input_dir=pathlib.Path(a.data), stego_method=stego_method, alpha=alpha, model_path=None,
                           model_name=model_name, **common))
    for loss in a.losses:
        train_method = a.train_method if loss == "l1ws" else "dropout"
        name = get_model_name(stego_method=train_method, model_dir=model_dir)
        for stego_method, alpha in settings:
            r = run(input_dir=pathlib.Path(a.data), stego_method=stego_method, alpha=alpha, model_path=model_dir / train_method,
                    model_name=name, **common)
            r["model_name"] = f"UNet_{loss}" + (f"_{train_method}" if loss == "l1ws" else "")
            res.append(r)
    res = pd.concat(res).reset_index(drop=True)
    res["stego_method"] = res["stego_method"].fillna("Cover") if "stego_method" in res else "Cover"
    out = pathlib.Path(a.out or f"../results/estimation/ws_{a.train_method}.csv")
    out.parent.mkdir(parents=True, exist_ok=True)
    res.to_csv(out, index=False)
    print(f"output saved to {out}")


if __name__ == "__main__":
    main()
