"""Linear pixel predictors and plane selectors the WS estimator is configured with.

Mirrors the pieces of the reference that `src/ws/estimate.py:149-205 run` pulls in:
  NAMED_FILTERS_2D, get_coefficients, get_filter_estimator, infere_single   src/filters/evaluate.py:22-50,118-146
  get_processor_2d                                                          src/_defs/filters.py:72-83
and the prediction-error table of the filters, results/prediction/filters.csv:
  get_filter_residuals_cover, run                                           src/filters/evaluate.py:53-115,149-205
(mae and wmae per image and filter; wmae is the MAE over the 10 % of interior pixels with the lowest HILL cost, ws_unet_amd.hill).
The OLS fits the reference's filter tooling reads (`OLS_*.csv`, `kernels.json`) are made by ws_unet_amd.ols; `register_filter` enters a
fitted filter into the two name tables below, so that every driver that looks a name up accepts it.
`infere_single` runs on the GPU (wsu_filter3x3_valid_f32); inside `ws.estimate` a `FilterEstimator` is recognised and its
taps are evaluated in the statistic kernel itself, so the prediction never exists in memory.  The same holds for the filter table:
the flattened 8-tap coefficients are evaluated inside the error kernel (wsu_prediction_error) in float64, as `x @ filter` is.
"""
import pathlib
import typing

import numpy as np

from . import fabrika
from .imread import imread4_f32, imread4_u8, u8_plane
from .planes import load_planes_u8, upload_planes

NAMED_FILTERS = {
    "KB": np.array([[-1], [+2], [-1], [+2], [-1], [+2], [-1], [+2]], dtype="float64") / 4.,
    "AVG": np.ones((8, 1)) / 8.,
}


def _k2d(rows, div):
    return np.array([rows], dtype="float32").T / div          # (3,3,1), [a][b][0] = rows[b][a] like the reference's `.T`


NAMED_FILTERS_2D = {
    "KB": _k2d([[-1, +2, -1], [+2, 0, +2], [-1, +2, -1]], 4.),
    "AVG": _k2d([[1, 1, 1], [1, 0, 1], [1, 1, 1]], 8.),
    "AVG9": _k2d([[1, 1, 1], [1, 1, 1], [1, 1, 1]], 9.),
    "1": _k2d([[0, 0, 0], [0, 1, 0], [0, 0, 0]], 1.),
}


BUILTIN_FILTERS = frozenset(NAMED_FILTERS_2D)


def kernel_2d(taps8) -> np.ndarray:
    """8 flattened taps (neighbour order x00 x01 x02 x12 x22 x21 x20 x10, the weight of x[r-1+a][c-1+b]) -> the (3,3,1) float32 kernel
    array of NAMED_FILTERS_2D (`_k2d`: applied as a true convolution, so the weights appear reversed)."""
    from .ops import _RING
    wgt = np.zeros((3, 3))
    for tap, (a, b) in zip(np.asarray(taps8, dtype="float64").reshape(8), _RING):
        wgt[a, b] = tap
    return _k2d(wgt[::-1, ::-1].T, 1.)


def register_filter(name: str, taps8) -> None:
    """Enter a fitted filter under `name`: NAMED_FILTERS[name] = the (8,1) float64 taps, NAMED_FILTERS_2D[name] = its (3,3,1) float32
    kernel (ws.estimate.NAMED_FILTERS is that dict).  Registering a fitted name again replaces it; the built-in names are refused."""
    taps = np.array(taps8, dtype="float64")
    if taps.size != 8 or not np.all(np.isfinite(taps)):
        raise ValueError(f"filter {name!r}: 8 finite taps expected, got shape {taps.shape}")
    if not isinstance(name, str) or not name or name in BUILTIN_FILTERS:
        raise ValueError(f"filter name {name!r} is empty or one of the built-in filters {sorted(BUILTIN_FILTERS)}")
    NAMED_FILTERS[name] = taps.reshape(8, 1)
    NAMED_FILTERS_2D[name] = kernel_2d(taps)


def get_coefficients(filter_name: str, flatten: bool = True) -> np.ndarray:
    return NAMED_FILTERS[filter_name] if flatten else NAMED_FILTERS_2D[filter_name]


def infere_single(x: np.ndarray, model: np.ndarray) -> np.ndarray:
    """(H,W,C) float -> (H-2,W-2,1) float32: convolve(x / 255., model[..., ::-1], 'valid')[..., :1] * 255. for a
    single-channel 3x3 kernel (the only kind the UNet comparison uses)."""
    import torch
    from . import ops
    if model.ndim != 3 or model.shape != (3, 3, 1):
        raise NotImplementedError("only (3,3,1) kernels are on the GPU path")
    x0 = np.ascontiguousarray(np.asarray(x, dtype=np.float32)[..., 0])
    y = ops.filter3x3_valid(torch.from_numpy(x0)[None].cuda(), model[..., ::-1])
    return y[0].cpu().numpy()[..., None]


class FilterEstimator:
    """`lambda x: infere_single(x, kernel)` (filters/evaluate.py:144-146) as an object, so that callers can see the taps."""

    def __init__(self, kernel: np.ndarray):
        self.kernel = kernel

    def __call__(self, x: np.ndarray) -> np.ndarray:
        return infere_single(x, self.kernel)

    def device_arguments(self, x_u8, correct_bias: bool = False) -> dict:
        """The statistic kernels' keywords (ws.estimate.predictor_arguments): the taps, evaluated in the kernel."""
        return dict(pixel_filter=np.asarray(self.kernel)[..., ::-1])


def get_filter_estimator(*args, **kw) -> typing.Callable:
    return FilterEstimator(get_coefficients(*args, **kw))


def get_processor_2d(channels: typing.List[int]) -> typing.Callable:
    """Plane selector `x[..., channels].astype('float32')` (_defs/filters.py:72-83; the Bayer offsets are all None)."""
    channels = list(channels)

    def process_gray(x: np.ndarray) -> np.ndarray:
        return x[..., channels].astype("float32")

    process_gray.plane_selector = tuple(channels)          # lets the batched WS path skip the host arrays for the Y plane
    return process_gray


# ---- prediction-error table (src/filters/evaluate.py:53-115,149-179) ------------------------------------------------------------------------
# The reference's get_processor (_defs/filters.py:39-69) turns a plane into the eight neighbours x00 x01 x02 x12 x22 x21 x20 x10 and the
# centre x11, and `y - x @ filter` is the residual; here the 8 taps go to the kernel, which reads the neighbours itself
# (ops.filter_taps), and the HILL cost is computed on the device.  conseal.hill._costmap.compute_cost of the reference is the
# textbook cost of ws_unet_amd.hill (the one that reproduces the published filters.csv).

def _plane_u8(img: np.ndarray, channel: int) -> np.ndarray:
    return u8_plane(np.asarray(img)[..., channel], "the HILL cost is defined on 8-bit pixel values")


def _device_error(x_u8_host, filter):
    """(N,H,W) uint8 host planes -> numpy (mae[N], wmae[N]) of the in-kernel filter prediction."""
    import torch
    from . import ops
    mae, wmae = ops.prediction_error(upload_planes(torch.as_tensor(x_u8_host), "cuda"), pixel_filter=filter)
    return mae.cpu().numpy(), wmae.cpu().numpy()


def _row(fname, channels, filter_name, mae, wmae, kw) -> dict:
    ch = "".join(map(str, channels))
    return {"fname": fname, f"mae_{ch}_{filter_name}": float(mae), f"wmae_{ch}_{filter_name}": float(wmae), **kw}


_ROW_KEYS = ("filter", "filter_name", "channels", "process_image", "imread")


def _residuals_one(fname, filter: np.ndarray, filter_name: str, channels: typing.Tuple[int],
                               process_image: typing.Callable = None, imread: typing.Callable = imread4_u8, **kw):
    """Row {fname, mae_<ch>_<name>, wmae_<ch>_<name>, **kw} of one image (src/filters/evaluate.py:79-115).  `process_image` is
    accepted for the reference's signature; the neighbour features are read by the kernel from plane channels[0]."""
    x = _plane_u8(imread(fname), channels[0])
    mae, wmae = _device_error(x[None], filter)
    return _row(fname, channels, filter_name, mae[0], wmae[0], kw)


get_filter_residuals_cover = fabrika.precovers(iterator="python", convert_to="pandas", ignore_missing=True)(_residuals_one)


def _residuals_batch(fnames, kws, *, filter, filter_name, channels, imread=imread4_u8, prefetched=None, **_ignored):
    """get_filter_residuals_cover for a chunk (fabrika iterator='batched'): one upload and one launch chain for the whole chunk."""
    planes = prefetched[0] if prefetched is not None else _chunk_planes(fnames, channels, imread)
    if planes is None:                                             # ragged chunk
        return [_residuals_one(f, filter, filter_name, channels, imread=imread, **kw) for f, kw in zip(fnames, kws)]
    mae, wmae = _device_error(planes, filter)
    return [_row(f, channels, filter_name, mae[i], wmae[i], kw) for i, (f, kw) in enumerate(zip(fnames, kws))]


def _chunk_planes(fnames, channels, imread):
    if tuple(channels) == (3,) and imread in (imread4_u8, imread4_f32):
        return load_planes_u8(fnames, imread4_u8)                  # native batched decode of the Y plane into a pinned buffer
    planes = [_plane_u8(imread(f), channels[0]) for f in fnames]
    return np.stack(planes) if len({p.shape for p in planes}) == 1 else None


get_filter_residuals_cover_batched = fabrika.precovers(iterator="batched", convert_to="pandas", ignore_missing=True)(fabrika.shared_kwargs(
    _residuals_batch, _ROW_KEYS, lambda fnames, kws: (_chunk_planes(fnames, kws[0]["channels"], kws[0].get("imread", imread4_u8)),)))


def run(input_dir: pathlib.Path, filter_names: typing.Sequence[str] = ("AVG", "KB"), channels=((3,),),
        imread: typing.Callable = imread4_u8, iterator: str = "python", **kw):
    """The filters.csv table (src/filters/evaluate.py:149-179): one frame per zip(channels, filter_names) pair, concatenated.
    With the default one-entry `channels` only the first filter (AVG) runs, as in the reference; its __main__ passes [[3], [3]].
    iterator='batched' sends chunks of files through one launch chain (`batch_size` images)."""
    import pandas as pd
    fn = {"python": get_filter_residuals_cover, "batched": get_filter_residuals_cover_batched}[iterator]
    res = []
    for channel, filter_name in zip(channels, filter_names):
        res.append(fn(input_dir, filter=get_coefficients(filter_name), filter_name=filter_name, channels=tuple(channel),
                      imread=imread, **kw))
    return pd.concat(res)
