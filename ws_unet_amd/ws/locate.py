"""Locating a payload from WS residuals (A. D. Ker, "Locating steganographic payload via WS residuals", ACM MM&Sec 2008) beside the two
estimators of its size (ws.estimate: uniform and sequential placement).  Not part of the reference.

When many stego images were made with one stego key, the payload sits at the same pixels of all of them.  The per-pixel term of the WS
statistic, r = (s - s_bar)(s - s_hat), has expectation 1/2 at a used pixel (the LSB was replaced by a message bit: flipped half of the
time, and a flipped pixel has r = 1 + noise, an unflipped one r = noise) and 0 at an unused one, so the mean of r over the IMAGES,
weighted by 1 / (5 + var) as the statistic weights its pixels, separates the two sets; its noise is the predictor's error, which is why a
better predictor locates from fewer images.

`ResidualAccumulator` keeps the two per-pixel sums on the device as exact integers (ops.ws_residual_accumulate, K29: num in 2^-24 units
of wgt * r, den in 2^-32 units of wgt), so they depend on neither the batches the images arrive in nor their order.  It takes at most
65 536 images; then |num| < 2^53 and den < 2^53, both convert to float64 exactly, and mean = num * 256 / den is the correctly rounded
quotient of two exact integers: torch and numpy give the same bits.  `residual_mean`, `decide` and `confusion` are written once for
numpy arrays and torch tensors.

`run` walks a data set in file order with any pixel predictor ws.estimate knows and takes a decision at the image counts asked for;
`python -m ws_unet_amd.ws.locate` writes the table, the decision maps and the means.  embed's 'LSBRK' makes the matching stego images."""
from __future__ import annotations

import argparse
import pathlib
import typing

import numpy as np
import torch

from .. import fabrika, filters, ops
from ..imread import imread4_u8
from ..planes import decode_pool, load_planes_u8, upload_planes
from ..unet_run import model_device
from . import estimate, predictors, structural

MAX_IMAGES = ops.MAX_LOCATE_IMAGES
THRESHOLD = 0.25                                           # halfway between the two expectations of the mean


# ---- the mean, the two decisions and their score: numpy arrays or torch tensors ------------------------------------------------

def residual_mean(num, den):
    """int64 sums (num: 2^-24 units, den: 2^-32 units) -> float64 mean = num * 256 / den of the same kind; NaN where den = 0."""
    if isinstance(num, torch.Tensor):
        n, d = num.to(torch.float64), den.to(torch.float64)
        return torch.where(d == 0., torch.full_like(d, float("nan")), n * 256. / torch.where(d == 0., torch.ones_like(d), d))
    n, d = np.asarray(num).astype(np.float64), np.asarray(den).astype(np.float64)
    return np.where(d == 0., np.nan, n * 256. / np.where(d == 0., 1., d))


def decide(mean, threshold: typing.Optional[float] = None, count: typing.Optional[int] = None):
    """The used positions (bool, mean's shape and kind): `mean > threshold` (default 1/4), or with `count` = m the m largest means in a
    stable order -- NaN last, then the smaller (row-major) index first among equal means.  A NaN mean is never used."""
    if threshold is not None and count is not None:
        raise ValueError("decide: give threshold or count, not both")
    xp = torch if isinstance(mean, torch.Tensor) else np
    if xp is np:
        mean = np.asarray(mean, dtype=np.float64)
    nan = xp.isnan(mean)
    if count is None:
        return (mean > (THRESHOLD if threshold is None else float(threshold))) & ~nan
    m = int(count)
    if m < 0:
        raise ValueError(f"decide: count must not be negative, got {count}")
    flat = mean.reshape(-1)
    if xp is torch:
        key = torch.where(nan.reshape(-1), torch.full_like(flat, -float("inf")), flat)
        order = torch.sort(key, descending=True, stable=True)[1]
        used = torch.zeros(flat.shape, dtype=torch.bool, device=flat.device)
    else:
        order = np.argsort(-np.where(nan.reshape(-1), -np.inf, flat), kind="stable")
        used = np.zeros(flat.shape, dtype=bool)
    used[order[:m]] = True
    return used.reshape(mean.shape) & ~nan


def confusion(used, truth) -> dict:
    """Decision against ground truth (bool or 0 / 1, equal shapes, numpy or torch) -> {tp, fp, tn, fn, accuracy}: Python ints and a float."""
    if tuple(used.shape) != tuple(truth.shape):
        raise ValueError(f"confusion: decision of shape {tuple(used.shape)} against truth of shape {tuple(truth.shape)}")
    u, t = used != 0, truth != 0
    tp, fp, tn, fn = (int((a & b).sum()) for a, b in ((u, t), (u, ~t), (~u, ~t), (~u, t)))
    total = tp + fp + tn + fn
    return {"tp": tp, "fp": fp, "tn": tn, "fn": fn, "accuracy": (tp + tn) / total if total else float("nan")}


# ---- the accumulator --------------------------------------------------------------------------------------------------------------

class ResidualAccumulator:
    """The per-pixel sums of the WS residual terms over the images fed so far, for (h, w) planes, on `device`."""

    def __init__(self, h: int, w: int, device=None):
        h, w = int(h), int(w)
        if h < 3 or w < 3:
            raise ValueError(f"ResidualAccumulator: a plane of at least 3 x 3 pixels expected, got {h} x {w}")
        self.h, self.w = h, w
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.num = torch.zeros((h - 2, w - 2), dtype=torch.int64, device=self.device)
        self.den = torch.zeros((h - 2, w - 2), dtype=torch.int64, device=self.device)
        self.images = 0

    def add(self, x_u8: torch.Tensor, pixel_estimator, mean_estimator=estimate.NAMED_FILTERS["AVG"], weighted: int = 1,
            host_planes=None) -> "ResidualAccumulator":
        """Adds the terms of the (N,H,W) uint8 device planes `x_u8` under a pixel predictor of ws.estimate: an estimator with
        `device_arguments` (those listed in ws/predictors.py and a UNetEstimator; the prediction never leaves the device), or a host
        callable, which needs `host_planes` (estimate.predictor_arguments).  Nothing waits for the GPU."""
        if int(weighted) not in (0, 1):
            raise ValueError(f"ResidualAccumulator.add: weighted must be 0 or 1, got {weighted}")
        if isinstance(pixel_estimator, structural.StructuralEstimator) or pixel_estimator is None:
            raise ValueError(f"ResidualAccumulator.add needs a pixel predictor; the structural estimators {structural.NAMES} have none")
        if not (isinstance(x_u8, torch.Tensor) and x_u8.dim() == 3 and x_u8.dtype == torch.uint8):
            raise ValueError("ResidualAccumulator.add: x_u8 must be an (N,H,W) uint8 tensor")
        if tuple(x_u8.shape[1:]) != (self.h, self.w):
            raise ValueError(f"ResidualAccumulator.add: planes of {tuple(x_u8.shape[1:])} for an accumulator of {(self.h, self.w)} "
                             f"(all images of one key must have one size)")
        n = x_u8.shape[0]
        if self.images + n > MAX_IMAGES:
            raise ValueError(f"ResidualAccumulator.add: {self.images} + {n} images exceed {MAX_IMAGES}, beyond which the sums are no "
                             f"longer exact in float64")
        step = 32768                                       # (a call of the kernel takes at most 65535 images)
        for i in range(0, n, step):
            x = x_u8[i:i + step]
            pred = estimate.predictor_arguments(x, pixel_estimator, None if host_planes is None else host_planes[i:i + step])
            ops.ws_residual_accumulate(x, self.num, self.den, mean_filter=np.asarray(mean_estimator)[..., ::-1], weighted=int(weighted), **pred)
        self.images += n
        return self

    def mean(self) -> torch.Tensor:
        """float64 (H-2,W-2) on the device: the weighted mean of r over the images, NaN where no image contributed."""
        return residual_mean(self.num, self.den)

    def used(self, threshold: typing.Optional[float] = None, count: typing.Optional[int] = None) -> torch.Tensor:
        """bool (H-2,W-2) on the device: `decide` on the mean."""
        return decide(self.mean(), threshold, count)


# ---- a data set ---------------------------------------------------------------------------------------------------------------------

class _Walk:
    """The state one pass over a data set shares between its chunks: the accumulator (made at the first chunk), the counts still to
    decide at, and the decisions taken."""

    def __init__(self, pixel_estimator, weighted, at, threshold):
        self.pixel_estimator, self.weighted, self.threshold = pixel_estimator, int(weighted), threshold
        self.at = sorted({int(c) for c in at})
        if self.at and self.at[0] < 1:
            raise ValueError(f"at: image counts must be positive, got {list(at)}")
        self.acc = None
        self.decisions = []                                # (images, used (H-2,W-2) bool on the device)

    def decide(self) -> None:
        if not self.decisions or self.decisions[-1][0] != self.acc.images:
            self.decisions.append((self.acc.images, self.acc.used(threshold=self.threshold)))

    def feed(self, x_u8: torch.Tensor, host_planes=None) -> None:
        if self.acc is None:
            self.acc = ResidualAccumulator(x_u8.shape[1], x_u8.shape[2], x_u8.device)
        i = 0
        while i < x_u8.shape[0]:                           # a chunk is split where a count falls inside it
            room = x_u8.shape[0] - i
            nxt = next((c - self.acc.images for c in self.at if c > self.acc.images), room)
            n = min(room, nxt)
            self.acc.add(x_u8[i:i + n], self.pixel_estimator, weighted=self.weighted,
                         host_planes=None if host_planes is None else host_planes[i:i + n])
            i += n
            if self.acc.images in self.at:
                self.decide()


def _native(channels, imread, process_image) -> bool:
    plain = process_image is None or getattr(process_image, "plane_selector", None) == (3,)
    return imread is imread4_u8 and plain and tuple(channels) == (3,)


def _accumulate_chunk(fnames, kws, *, walk, channels, imread=imread4_u8, process_image=None, prefetched=None, **_ignored):
    """One chunk of files into the walk's accumulator; one (empty) row per file for the iterator."""
    planes = None
    if _native(channels, imread, process_image):
        u8 = prefetched[0] if prefetched is not None else load_planes_u8(fnames, imread)
    else:
        process_image = process_image or filters.get_processor_2d(channels)
        planes = list(decode_pool().map(lambda f: process_image(imread(f)), fnames))
        u8 = torch.from_numpy(np.stack([estimate._as_u8_plane(p) for p in planes])) if len({p.shape for p in planes}) == 1 else None
    if u8 is None:
        raise ValueError("ws.locate: the images of a chunk differ in size; one stego key places a payload in images of one size")
    walk.feed(upload_planes(u8, model_device(estimate.unet_model_of(walk.pixel_estimator))), planes)
    return [{} for _ in fnames]


def _accumulate_one(fname, *, walk, channels, imread=imread4_u8, process_image=None, **_ignored):
    return _accumulate_chunk([fname], [{}], walk=walk, channels=channels, imread=imread, process_image=process_image)[0]


def _prefetch(fnames, kws):
    k0 = kws[0]
    if not _native(k0["channels"], k0.get("imread", imread4_u8), k0.get("process_image")):
        return None
    return (load_planes_u8(fnames, imread4_u8),)


_KEYS = ("walk", "channels", "imread", "process_image")
_chunk = fabrika.shared_kwargs(_accumulate_chunk, _KEYS, _prefetch)
_ITERATORS = {
    (True, True): fabrika.stego_spatial(iterator="batched", convert_to=None, ignore_missing=True)(_chunk),
    (True, False): fabrika.stego_spatial(iterator="python", convert_to=None, ignore_missing=True)(_accumulate_one),
    (False, True): fabrika.precovers(iterator="batched", convert_to=None, ignore_missing=True)(_chunk),
    (False, False): fabrika.precovers(iterator="python", convert_to=None, ignore_missing=True)(_accumulate_one),
}


def pixel_predictor(model_name: str, model_path, channels):
    """A pixel predictor's name in ws/predictors.py, or a trained UNet run, as (pixel predictor, the name its rows carry)
    (estimate.resolve_predictor); the structural estimators have no per-pixel prediction and raise."""
    if model_name in structural.NAMES:
        raise ValueError(f"ws.locate needs a pixel predictor; the structural estimators {structural.NAMES} have none")
    return estimate.resolve_predictor(model_name, model_path, channels)


def walk(input_dir, stego_method, alpha, pixel_estimator, channels=(3,), weighted: int = 1, at=(), batched: bool = True,
         threshold: float = THRESHOLD, imread: typing.Callable = imread4_u8, **kw) -> _Walk:
    """One pass over the stego images of (stego_method, alpha) -- the covers for stego_method None -- in file order; the returned state
    holds the accumulator (`.acc`) and the decisions [(images, used)] at every count of `at` that was reached and at the end."""
    if int(weighted) not in (0, 1):
        raise ValueError(f"ws.locate: weighted must be 0 or 1, got {weighted}")
    state = _Walk(pixel_estimator, weighted, at, threshold)
    select = {"stego_method": stego_method, "alpha": alpha} if stego_method else {}
    _ITERATORS[(bool(stego_method), bool(batched))](pathlib.Path(input_dir), inbayer=None, **select, walk=state, channels=tuple(channels),
                                                   imread=imread, process_image=filters.get_processor_2d(channels=channels), **kw)
    state.decide()
    return state


def _rows(state: _Walk, model_name, stego_method, alpha, key) -> typing.List[dict]:
    truth = None
    if key is not None:
        if str(stego_method).upper() != "LSBRK":
            raise ValueError(f"key: only 'LSBRK' places its payload by a key, got stego_method {stego_method!r}")
        truth = ops.lsbr_key_mask(key, ops.lsbr_key_threshold(alpha), state.acc.h, state.acc.w, state.acc.device)[1:-1, 1:-1]
    rows = []
    for images, used in state.decisions:
        row = {"model_name": model_name, "stego_method": stego_method, "alpha": alpha, "weighted": state.weighted, "images": images,
               "used": int(used.sum()), "threshold": state.threshold}
        rows.append(row | (confusion(used, truth) if truth is not None else {}))
    return rows


def run(input_dir: pathlib.Path, stego_method: str, alpha: float, model_name: str, model_path: str, channels: typing.Tuple[int],
        weighted: int = 1, at: typing.Sequence[int] = (), key: typing.Optional[int] = None, batched: bool = True, return_state: bool = False,
        **kw):
    """Locates the payload of a data set's (stego_method, alpha) images with a named linear filter, 'OLSa' / 'OLSa2' or a trained UNet as
    the pixel predictor: a table with one row per image count of `at` that the set reaches and one for the whole set -- model_name,
    stego_method, alpha, weighted, images, used (pixels decided as used, mean > threshold), threshold -- and, with the stego `key` of
    'LSBRK' images, tp, fp, tn, fn, accuracy against ops.lsbr_key_mask on the interior.  return_state: also the walk (accumulator and
    decision maps).  Other keywords go to the fabrika iterators (take_num_images, split, ...)."""
    import pandas as pd
    if key is not None and str(stego_method).upper() != "LSBRK":
        raise ValueError(f"key: only 'LSBRK' places its payload by a key, got stego_method {stego_method!r}")
    pixel_estimator, name = pixel_predictor(model_name, model_path, channels)
    state = walk(input_dir, stego_method, alpha, pixel_estimator, channels, weighted, at, batched, **kw)
    res = pd.DataFrame(_rows(state, name, stego_method, alpha, key))
    return (res, state) if return_state else res


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------

def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Locate the payload shared by a data set's stego images from their WS residuals: locate.csv, "
                                             "and per predictor the decision map (8-bit PNG, 255 = used) and the residual mean (.npy).")
    ap.add_argument("--data", required=True, help="data set root with stego*/files.csv")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--stego-method", default="LSBRK")
    ap.add_argument("--alpha", type=float, required=True)
    ap.add_argument("--filters", nargs="*", default=["AVG", "KB"], help=predictors.filters_help(structural=False))
    ap.add_argument("--model-dir", default=None, help="trained UNets in the reference's layout <dir>/<train method>/<run>/; no UNet rows without it")
    ap.add_argument("--losses", nargs="*", default=["l1ws"], help="UNet runs under --model-dir: 'l1' (the dropout run), 'l1ws' (--train-method)")
    ap.add_argument("--train-method", default="LSBR", help="stego method the l1ws UNet was trained on")
    ap.add_argument("--weighted", type=int, choices=(0, 1), default=1)
    ap.add_argument("--key", type=int, default=None, help="the stego key of LSBRK images: adds the confusion counts against its positions")
    ap.add_argument("--at", type=int, nargs="*", default=[], help="image counts at which a decision is taken, beside the whole set")
    ap.add_argument("--per-image", action="store_true", help="use the per-image iterator instead of the batched one")
    predictors.add_arguments(ap)
    return ap.parse_args(argv)


def main(argv=None) -> None:
    import pandas as pd
    from PIL import Image
    a = parse_args(argv)
    predictors.register_from_args(a)
    jobs = [(name, name, None) for name in a.filters]
    if a.model_dir:
        from .. import get_model_name
        for loss in a.losses:
            method = a.train_method if loss == "l1ws" else "dropout"
            label = f"UNet_{loss}" + (f"_{method}" if loss == "l1ws" else "")
            jobs.append((label, get_model_name(stego_method=method, model_dir=pathlib.Path(a.model_dir)), pathlib.Path(a.model_dir) / method))
    out = pathlib.Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    frames = []
    for label, model_name, model_path in jobs:
        res, state = run(pathlib.Path(a.data), a.stego_method, a.alpha, model_name, model_path, (3,), weighted=a.weighted, at=a.at, key=a.key,
                         batched=not a.per_image, return_state=True)
        res["model_name"] = label
        frames.append(res)
        Image.fromarray(state.decisions[-1][1].cpu().numpy().astype(np.uint8) * 255).save(out / f"used_{label}.png")
        np.save(out / f"mean_{label}.npy", state.acc.mean().cpu().numpy())
    pd.concat(frames).reset_index(drop=True).to_csv(out / "locate.csv", index=False)
    print(f"output saved to {out / 'locate.csv'}")


if __name__ == "__main__":
    main()
