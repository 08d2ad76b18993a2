"""Predictor / stego-change correlation table of the reference, results/estimation/correlation.csv (src/correlation.py):

    python -m ws_unet_amd.correlation --data DATA --out correlation.csv [--model-dir DIR]

For every cover/stego pair (LSBR, alpha 1.0 by default) a predictor estimates the cover from the STEGO image, and the table
measures how far that estimate follows the embedding change (src/correlation.py:22-59):

    d     = (x_s - x_c)[1:-1, 1:-1]          xhat = predictor(x_s)           dhat = xhat - x_c[1:-1, 1:-1]
    cov   = sum((dhat - mean dhat) * (d - mean d)) / (n - 1)                   n = (H-2)(W-2)
    cor   = cov / std(xhat) / std(d)                                           both std with ddof 0
    p     = student_t_sf(|cor| / sqrt(1 - cor^2) * sqrt(n - 2), n - 2)

The reference's quirks are restated, not fixed: the denominator takes the std of xhat, not of dhat (the identity filter "1" gives
~0.013, not 1, and |cor| can exceed 1, where the p-value is NaN); the covariance divides by n-1 and the stds by n; division
follows IEEE (x_s == x_c gives NaN, a constant prediction +-inf).  Where the reference produces an artefact, this module raises
ValueError instead: a colour image (the reference broadcasts (H-2,W-2,1) against (H-2,W-2,3)) and a cover without a stego twin
(the reference builds a path from NaN).

cor runs on the GPU (K15, wsu_pair_correlation) in float64; p is computed on the host without scipy (student_t_sf).
"""
from __future__ import annotations

import argparse
import logging
import math
import pathlib
import typing

import numpy as np

from . import fabrika, filters, unet_run
from .planes import load_planes_u8, upload_planes

MODEL_NAMES = ("1", "AVG9", "AVG", "KB")
UNET_STEGO_METHODS = ("dropout", "LSBR", "HILLR")


# ---- Student's t survival function (scipy.stats.t.sf without scipy) -----------------------------------------------------------------

_LOG_SQRT_2PI = 0.9189385332046727


def _lgammacor(x: float) -> float:
    """lgamma(x) - ((x - 1/2) log x - x + log sqrt(2 pi)) for x >= 10: the Stirling series, to double precision."""
    x2 = 1.0 / (x * x)
    return (1 / 12 + x2 * (-1 / 360 + x2 * (1 / 1260 + x2 * (-1 / 1680 + x2 * (1 / 1188 + x2 * (-691 / 360360 + x2 * (
        1 / 156 + x2 * (-3617 / 122400)))))))) / x


def _lbeta(a: float, b: float) -> float:
    """log B(a, b) without the cancellation of lgamma(a) + lgamma(b) - lgamma(a + b) at large arguments."""
    p, q = min(a, b), max(a, b)
    if q < 10:
        return math.lgamma(p) + math.lgamma(q) - math.lgamma(p + q)
    corr = _lgammacor(q) - _lgammacor(p + q)
    if p >= 10:
        corr += _lgammacor(p)
        return -0.5 * math.log(q) + _LOG_SQRT_2PI + corr + (p - 0.5) * math.log(p / (p + q)) + q * math.log1p(-p / (p + q))
    return math.lgamma(p) + corr + p - p * math.log(p + q) + (q - 0.5) * math.log1p(-p / (p + q))


def _betacf(a: float, b: float, x: float, d0: float) -> float:
    """Continued fraction of the regularized incomplete beta function (modified Lentz), for x < (a + 1) / (a + b + 2).
    d0 = 1 - (a + b) x / (a + 1), its first denominator, comes from the caller: near the bound it is a small difference of two
    numbers close to 1, which the caller forms without cancellation."""
    tiny, eps = 1e-300, 1e-16
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, d0
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 100000):
        m2 = 2 * m
        for aa in (m * (b - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = 1.0 + aa / c
            c = c if abs(c) > tiny else tiny
            h *= d * c
        if abs(d * c - 1.0) < eps:
            return h
    raise RuntimeError(f"incomplete beta continued fraction did not converge (a={a}, b={b}, x={x})")


def student_t_sf(t: float, df: float) -> float:
    """Survival function P(T > t) of Student's t with df degrees of freedom, in float64 (scipy.stats.t.sf):
    sf = I_x(df/2, 1/2) / 2 with x = df / (df + t^2), through the continued fraction of I on whichever side converges, and with
    x, 1 - x and their logs formed from r = t^2/df directly, so that neither t -> 0 at large df nor the far tail loses digits.
    NaN in, NaN out; sf(0) = 0.5, sf(inf) = 0, sf(-t) = 1 - sf(t); df <= 0 gives NaN.  Relative error against scipy: <= 1e-10 for
    df <= 4e6 wherever sf > 1e-300 (tests/test_correlation_host.py), a few 1e-10 at df ~ 1e7 (the continued fraction's terms
    cancel to ~1/df there)."""
    t, df = float(t), float(df)
    if math.isnan(t) or math.isnan(df) or df <= 0:
        return math.nan
    if t < 0:
        return 1.0 - student_t_sf(-t, df)
    if t == 0:
        return 0.5
    if math.isinf(t):
        return 0.0
    r = t * t / df
    if math.isinf(r):
        return 0.0
    a, b = 0.5 * df, 0.5
    x, xc = 1.0 / (1.0 + r), r / (1.0 + r)                        # x = df/(df+t^2) and 1 - x, each to a few ulps
    lx = -math.log1p(r)                                           # log x
    lxc = (math.log(r) - math.log1p(r)) if r > 0 else -math.inf   # log(1 - x): only its absolute error matters (it is an exponent)
    lfront = a * lx + b * lxc - _lbeta(a, b)
    if x < (a + 1.0) / (a + b + 2.0):
        d0 = ((1.0 - b) + (a + 1.0) * r) / ((1.0 + r) * (a + 1.0))          # 1 - (a+b) x / (a+1)
        return 0.5 * math.exp(lfront) * _betacf(a, b, x, d0) / a
    d0 = ((b + 1.0) + r - 0.5 * t * t) / ((1.0 + r) * (b + 1.0))            # 1 - (a+b) (1-x) / (b+1), with a r = t^2 / 2
    return 0.5 * (1.0 - math.exp(lfront) * _betacf(b, a, xc, d0) / b)


def p_value(cor, n):
    """student_t_sf(|cor| / sqrt(1 - cor^2) * sqrt(n - 2), n - 2) of src/correlation.py:52-53, evaluated in that order in float64.
    NaN-propagating: |cor| > 1 (sqrt of a negative number) and NaN cor give NaN; |cor| = 1 gives t = inf and p = 0.
    `cor`: a number or an array (the result has its shape); n: the pixel count of d."""
    c = np.asarray(cor, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.abs(c) / np.sqrt(1.0 - c ** 2) * np.sqrt(np.float64(n - 2))
    p = np.array([student_t_sf(v, n - 2) for v in t.reshape(-1)], dtype=np.float64).reshape(t.shape)
    return float(p) if p.ndim == 0 else p


# ---- GPU correlation of a batch of pairs ------------------------------------------------------------------------------------------

def correlation_u8_batch(xc_u8, xs_u8, predictor) -> typing.Tuple[np.ndarray, np.ndarray]:
    """(cor[N], p[N]) float64 numpy arrays for a batch of cover / stego planes, (N,H,W) uint8 device tensors.  The predictor is
      * a `filters.FilterEstimator`: its taps are evaluated on the stego planes inside K15 (no host convolution);
      * a `ws.estimate.UNetEstimator` or a bare model: one batched forward of the stego planes on the device, whose output K15 reads
        where it is (512 x 512 planes only: the reference's CenterCrop(512) would change the geometry);
      * any other callable: the reference's call pattern, `predictor(x_s)` per image on the host with x_s (H,W,1) float32 in
        0..255, returning (H-2,W-2[,1]); the predictions are uploaded as float32."""
    from . import ops
    from .ws.estimate import unet_model_of
    if xc_u8.dim() != 3 or xc_u8.shape != xs_u8.shape:
        raise ValueError(f"cover and stego batches differ in shape: {tuple(xc_u8.shape)} and {tuple(xs_u8.shape)}")
    n, h, w = xc_u8.shape
    model = unet_model_of(predictor)
    if isinstance(predictor, filters.FilterEstimator):
        cor = ops.pair_correlation(xc_u8, xs_u8, pixel_filter=np.asarray(predictor.kernel)[..., ::-1])
    elif model is not None:
        unet_run.check_unet_geometry((h, w), "the UNet predictor")
        cor = unet_run.range_retry(model, lambda: ops.pair_correlation(xc_u8, xs_u8, unet_run.unet_plane(model, xs_u8), hat_full=True,
                                                                      hat_scale=255.))
    else:
        import torch
        hats = []
        for x in xs_u8.cpu().numpy():
            hat = np.asarray(predictor(x[..., None].astype(np.float32)))
            if hat.shape not in ((h - 2, w - 2), (h - 2, w - 2, 1)):
                raise ValueError(f"predictor returned {hat.shape} for an image of {(h, w, 1)}; expected {(h - 2, w - 2, 1)}")
            hats.append(hat.reshape(h - 2, w - 2).astype(np.float32))
        x_hat = torch.from_numpy(np.stack(hats)).to(xc_u8.device)
        cor = ops.pair_correlation(xc_u8, xs_u8, x_hat, hat_full=False, hat_scale=1.)
    cor = cor.cpu().numpy()
    return cor, p_value(cor, (h - 2) * (w - 2))


# ---- the per-pair table (src/correlation.py:22-59 `run`) --------------------------------------------------------------------------

def _pair_paths(fname, name_c, name_s) -> typing.Tuple[pathlib.Path, pathlib.Path]:
    if not isinstance(name_s, str):
        raise ValueError(f"cover {name_c} has no stego twin in the selected stego set")
    dataset = pathlib.Path(fname).parents[len(pathlib.Path(name_c).parents) - 1]
    return dataset / name_c, dataset / name_s


def _check_gray(path) -> None:
    from PIL import Image
    with Image.open(path) as img:
        if img.mode != "L":
            raise ValueError(f"{path}: a {img.mode} image; the correlation is defined on 8-bit grayscale planes "
                             "(the reference broadcasts a colour image's three channels against one prediction plane)")


def _read_gray(path) -> np.ndarray:
    from PIL import Image
    _check_gray(path)
    return np.ascontiguousarray(np.array(Image.open(path)))


def _row(name_c, name_s, cor, p) -> dict:
    return {"name_c": str(name_c), "name_s": str(name_s), "correlation": float(cor), "p-value": float(p)}


def _pair_one(fname, name_c, name_s, predictor, **_kw) -> dict:
    import torch
    from .ws.estimate import unet_model_of
    path_c, path_s = _pair_paths(fname, name_c, name_s)
    x_c, x_s = _read_gray(path_c), _read_gray(path_s)
    if x_c.shape != x_s.shape:
        raise ValueError(f"cover {path_c} is {x_c.shape}, stego {path_s} is {x_s.shape}")
    dev = unet_run.model_device(unet_model_of(predictor))
    cor, p = correlation_u8_batch(torch.from_numpy(x_c)[None].to(dev), torch.from_numpy(x_s)[None].to(dev), predictor)
    return _row(name_c, name_s, cor[0], p[0])


_pairs_python = fabrika.cover_stego_spatial(iterator="python", convert_to="pandas", ignore_missing=True)(_pair_one)


def _chunk_planes(fnames, kws):
    """Cover and stego planes of a chunk as two (N,H,W) uint8 host tensors (native batched decode into pinned buffers), or None
    when the chunk's images differ in shape."""
    paths = [_pair_paths(f, kw["name_c"], kw["name_s"]) for f, kw in zip(fnames, kws)]
    for pc, ps in paths:
        _check_gray(pc)
        _check_gray(ps)
    xc = load_planes_u8([p[0] for p in paths])
    xs = load_planes_u8([p[1] for p in paths]) if xc is not None else None
    if xc is None or xs is None or xc.shape != xs.shape:
        return None
    return xc, xs


def _pair_chunk(fnames, kws, prefetched=None) -> typing.List[dict]:
    """_pair_one for a chunk of pairs (fabrika iterator='batched'): one upload and one K15 launch chain for the whole chunk."""
    from .ws.estimate import unet_model_of
    planes = prefetched if prefetched is not None else _chunk_planes(fnames, kws)
    if planes is None:                                              # ragged chunk
        return [_pair_one(f, **kw) for f, kw in zip(fnames, kws)]
    predictor = kws[0]["predictor"]
    xc, xs = upload_planes(planes, unet_run.model_device(unet_model_of(predictor)))
    cor, p = correlation_u8_batch(xc, xs, predictor)
    return [_row(kw["name_c"], kw["name_s"], cor[i], p[i]) for i, kw in enumerate(kws)]


_pair_chunk.prefetch = _chunk_planes
_pairs_batched = fabrika.cover_stego_spatial(iterator="batched", convert_to="pandas", ignore_missing=True)(_pair_chunk)


def run(input_dir: pathlib.Path, stego_method: str = None, alpha: float = None, predictor: typing.Callable = None,
        iterator: str = "batched", progress_on: bool = False, **kw):
    """Per-pair rows {name_c, name_s, correlation, p-value} of src/correlation.py:22-59 over the cover/stego pairs of a data set,
    in fabrika's order (sorted by stem, then name_c).  `predictor`: see correlation_u8_batch.  iterator='batched' runs chunks of
    pairs through one upload and one launch chain, decoding the next chunk meanwhile; 'python' runs pair by pair.  Both give the
    same table bit for bit."""
    if predictor is None:
        raise ValueError("a predictor is needed (filters.get_filter_estimator, get_unet_estimator or a callable)")
    fn = {"python": _pairs_python, "batched": _pairs_batched}[iterator]
    sel = {k: v for k, v in (("stego_method", stego_method), ("alpha", alpha)) if v is not None}
    return fn(input_dir, predictor=predictor, progress_on=progress_on, **sel, **kw)


def table(frames):
    """The published layout (src/correlation.py:108-118) from per-model frames, each carrying a `model_name` column: median
    correlation and p-value per model (NaN skipped, as pandas' median does), one column per model in order of first appearance,
    rows `correlation` and `p-value`.  `table(frames).to_csv(path)` writes the reference's file."""
    import pandas as pd
    res = pd.concat(frames).reset_index(drop=True)
    model_names = res.model_name.unique().tolist()
    res = res.groupby("model_name").agg({"correlation": "median", "p-value": "median"})
    return res.T[model_names]


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="the predictor / stego-change correlation table (results/estimation/correlation.csv)")
    ap.add_argument("--data", required=True, help="dataset root with images*/ and stego*/ files.csv (the reference's ../data)")
    ap.add_argument("--out", required=True, help="output CSV (the reference writes results/estimation/correlation.csv)")
    ap.add_argument("--filters", nargs="*", default=list(MODEL_NAMES), help="named filters of filters.NAMED_FILTERS_2D")
    ap.add_argument("--model-dir", default=None, help="trained UNets in the reference's layout <dir>/<stego method>/<run>/"
                                                      "{config.json,model/best_model.pt.tar}; UNet columns are omitted without it")
    ap.add_argument("--unet-stego-methods", nargs="*", default=list(UNET_STEGO_METHODS))
    ap.add_argument("--stego-method", default="LSBR")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--mode", default=None, help="UNet inference mode (default: the package default)")
    ap.add_argument("--per-image", action="store_true", help="one launch chain per pair instead of one per chunk of 32")
    ap.add_argument("--per-pair-out", default=None, help="also write the un-aggregated rows with their model_name")
    ap.add_argument("--progress", action="store_true")
    from .ols import add_kernels_argument
    add_kernels_argument(ap)
    return ap.parse_args(argv)


def main(argv=None) -> None:
    a = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    from .ols import register_from_args
    register_from_args(a)

    import pandas as pd
    iterator = "python" if a.per_image else "batched"
    frames = []

    def add(model_name, predictor):
        logging.info(f"running {model_name} ...")
        res = run(a.data, stego_method=a.stego_method, alpha=a.alpha, predictor=predictor, iterator=iterator, progress_on=a.progress)
        res["model_name"] = model_name
        frames.append(res)

    for name in a.filters:
        add(name, filters.get_filter_estimator(filter_name=name, flatten=False))
    if a.model_dir:
        from .evaluate import trained_runs
        from .ws.estimate import as_unet_estimator
        for method, model_name, config in trained_runs(a.model_dir, a.unet_stego_methods):
            predictor = as_unet_estimator((pathlib.Path(a.model_dir) / method, model_name), a.mode)
            add(f"UNet_{method}_{config['loss']}", predictor)
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    table(frames).to_csv(out)
    if a.per_pair_out:
        pathlib.Path(a.per_pair_out).parent.mkdir(parents=True, exist_ok=True)
        pd.concat(frames).reset_index(drop=True).to_csv(a.per_pair_out, index=False)
    logging.info(f"output saved to {out}")


if __name__ == "__main__":
    main()
