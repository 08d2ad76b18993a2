"""Least-squares 3x3 pixel predictors: the fitted counterpart of the fixed AVG / KB filters, and the predictor of the "improved WS"
estimator of Ker and Boehme (moderated weights and bias correction are in wsu_ws_attack already).

The reference's tooling reads such fits (filters/evaluate.py:129-133 `OLS_*.csv`, predictor_error.py:194-210 'OLS', contour.py
`kernels.json['OLS_0']`) but ships no code that makes them.  Here:

  * the device computes the exact integer moments of an image (ops.ols_moments, K24): per interior pixel the eight neighbours in the
    ring order of the flattened filters (x00 x01 x02 x12 x22 x21 x20 x10, _defs/filters.py:57-67) and the centre y, summed as the 45
    products v_i * v_j, i <= j.  They hold A = X^T X (8x8), b = X^T y and y^T y, and they add over images;
  * the host solves the normal equations A k = b in float64 (`fit`; no intercept), per image or for summed moments;
  * a fitted filter is entered into the name registry of `filters` (`filters.register_filter`), so every driver that looks a filter
    name up accepts it; `save_kernels` / `load_kernels` keep fits in a JSON file {"OLS": [8 taps], ...} (the drivers' --kernels);
  * `AdaptiveOLSEstimator` is the predictor fitted on the image under attack; ws.estimate runs moments -> fit -> the statistic with one
    filter per image (wsu_ws_attack_taps) on the resident planes.  Model names 'OLSa' (8 taps) and 'OLSa2' (symmetric).

A fit is valid iff the matrix of the solved system is positive definite and its condition number is at most 1e12; otherwise (a flat
image, fewer independent interior pixels than parameters) the taps are KB's and ok is False.

    python -m ws_unet_amd.ols --data DIR [--split split_tr.csv] [--take N] [--symmetric] --out kernels.json
"""
from __future__ import annotations

import collections
import json
import logging
import pathlib

import numpy as np

from . import filters
from .planes import load_planes_u8, plane_groups, upload_planes

COND_MAX = 1e12
_IU = np.triu_indices(9)
# edge and corner taps of the ring x00 x01 x02 x12 x22 x21 x20 x10: the two parameters of the symmetric fit
SYMMETRIC = np.zeros((8, 2))
SYMMETRIC[1::2, 0] = 1.
SYMMETRIC[0::2, 1] = 1.
ADAPTIVE_NAMES = {"OLSa": False, "OLSa2": True}              # model name -> symmetric


def _kb() -> np.ndarray:
    return filters.NAMED_FILTERS["KB"][:, 0].copy()


def unpack(moments):
    """(45,) or (N,45) integer moments -> (A (...,8,8), b (...,8), yty (...)) float64.  Float64 holds integers up to 2^53 exactly; a
    larger entry (about 5e5 images of 512^2 summed) raises."""
    m = np.asarray(moments)
    if m.dtype.kind not in "iu" or m.shape[-1] != 45 or m.ndim not in (1, 2):
        raise ValueError(f"expected integer moments of shape (45,) or (N,45), got {m.dtype} {m.shape}")
    if m.size and (m.min() < 0 or m.max() > 2 ** 53):
        raise OverflowError("a moment outside [0, 2^53] is not exact in float64")
    full = np.zeros(m.shape[:-1] + (9, 9))
    full[..., _IU[0], _IU[1]] = m
    full[..., _IU[1], _IU[0]] = m
    return full[..., :8, :8], full[..., :8, 8], full[..., 8, 8]


def _solve(A, b, symmetric):
    S = SYMMETRIC if symmetric else None
    if symmetric:
        A, b = S.T @ A @ S, S.T @ b
    try:
        np.linalg.cholesky(A)
        if not np.linalg.cond(A) <= COND_MAX:
            raise np.linalg.LinAlgError
        k = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return _kb(), False
    if not np.all(np.isfinite(k)):
        return _kb(), False
    return (S @ k if symmetric else k), True


def fit(moments, symmetric: bool = False):
    """Least-squares taps of one row of moments -> (taps8 (8,) float64, ok), or of every row of (N,45) -> ((N,8), ok (N,) bool).
    numpy.linalg.solve on the normal equations, no intercept.  symmetric=True fits two parameters, one for the four edge and one for
    the four corner neighbours (A and b folded with the 8x2 indicator matrix, S^T A S and S^T b) and expands them to 8 taps; validity
    is then judged on the folded 2x2 system, the one that is solved.  An invalid fit returns KB's taps and ok False."""
    A, b, _ = unpack(moments)
    if A.ndim == 2:
        return _solve(A, b, symmetric)
    res = [_solve(Ai, bi, symmetric) for Ai, bi in zip(A, b)]
    return np.array([r[0] for r in res]).reshape(len(res), 8), np.array([r[1] for r in res], dtype=bool)


def residual_mse(moments, taps8, count):
    """Mean squared residual of y - X k over the `count` pixels the moments were summed over: (yty - 2 k.b + k.A.k) / count, exact
    algebra on the moments (the pixel count is no moment of a fit without intercept, so the caller passes it)."""
    A, b, yty = unpack(moments)
    k = np.asarray(taps8, dtype=np.float64).reshape(8)
    return (yty - 2. * (b @ k) + k @ A @ k) / count


# ---- files and registry -----------------------------------------------------------------------------------------------------------

def save_kernels(path, kernels) -> None:
    """{name: taps8} -> JSON {"OLS": [8 floats], ...}; Python's float repr round-trips exactly."""
    out = {str(name): [float(t) for t in np.asarray(taps, dtype=np.float64).reshape(8)] for name, taps in kernels.items()}
    path = pathlib.Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")


def load_kernels(path, register: bool = False) -> dict:
    """The {name: taps8 float64} of a save_kernels file; register=True enters every one into the filter registry."""
    raw = json.loads(pathlib.Path(path).read_text())
    if not isinstance(raw, dict):
        raise ValueError(f"{path}: expected a JSON object of name -> 8 taps")
    kernels = {}
    for name, taps in raw.items():
        k = np.asarray(taps, dtype=np.float64)
        if k.shape != (8,):
            raise ValueError(f"{path}: {name!r} has shape {k.shape}, expected 8 taps")
        kernels[name] = k
    if register:
        for name, k in kernels.items():
            filters.register_filter(name, k)
    return kernels


def add_kernels_argument(ap) -> None:
    """The drivers' `--kernels kernels.json`."""
    ap.add_argument("--kernels", default=None, metavar="kernels.json",
                    help="fitted filters written by `python -m ws_unet_amd.ols`; their names become valid filter names")


def register_from_args(a) -> None:
    if getattr(a, "kernels", None):
        load_kernels(a.kernels, register=True)


# ---- the predictor fitted on the image under attack ----------------------------------------------------------------------------------

class AdaptiveOLSEstimator:
    """The least-squares predictor of each image, fitted on that image (the stego image under attack: no cover is needed).
    ws.estimate._stat recognises it and keeps everything on the device's planes; called on a host (H,W,C) array like the reference's
    estimators it fits and predicts that one image through filters.infere_single.  Images whose fit is invalid get KB's taps;
    `fallbacks` counts them and the first one is logged (once per estimator, i.e. per run)."""

    def __init__(self, symmetric: bool = False):
        self.symmetric = bool(symmetric)
        self.fallbacks = 0

    def note(self, ok) -> None:
        bad = int(np.size(ok) - np.count_nonzero(ok))
        if bad and not self.fallbacks:
            logging.warning("OLS fit: singular or ill-conditioned normal equations; such images are predicted with KB")
        self.fallbacks += bad

    def kernels(self, x_u8):
        """(N,H,W) uint8 device planes -> (N,3,3,1) float32 kernels in the layout of filters.NAMED_FILTERS_2D."""
        from . import ops
        taps, ok = fit(ops.ols_moments(x_u8).cpu().numpy(), self.symmetric)
        self.note(ok)
        return np.stack([filters.kernel_2d(t) for t in taps])

    def __call__(self, x: np.ndarray) -> np.ndarray:
        import torch
        from .imread import u8_plane
        plane = u8_plane(np.asarray(x)[..., 0], "the OLS fit needs integer pixel values in 0..255")
        kernel = self.kernels(torch.from_numpy(np.ascontiguousarray(plane))[None].cuda())[0]
        return filters.infere_single(x, kernel)


def adaptive_estimator(model_name: str):
    """'OLSa' / 'OLSa2' -> a fresh AdaptiveOLSEstimator, any other name -> None."""
    return AdaptiveOLSEstimator(ADAPTIVE_NAMES[model_name]) if model_name in ADAPTIVE_NAMES else None


# ---- one fit for a data set ----------------------------------------------------------------------------------------------------------

DatasetFit = collections.namedtuple("DatasetFit", "taps ok moments count")


def fit_dataset(data_dir, split: str = None, take_num_images: int = None, symmetric: bool = False, batch_size: int = 32) -> DatasetFit:
    """One fit over the cover images of a data set (fabrika's precovers; `split`, `take_num_images` as everywhere): the batched
    iterator with the native PNG decode one chunk ahead, one ols_moments launch per chunk, the rows summed as int64 on the device and
    read back once.  -> DatasetFit(taps (8,) float64, ok, moments (45,) int64, count = interior pixels summed).  Single process."""
    import torch
    from . import fabrika, ops
    total, count = [None], [0]

    def chunk(fnames, kws, prefetched=None):
        for g, _ in plane_groups(fnames, prefetched):             # (a ragged chunk: image by image)
            m = ops.ols_moments(upload_planes(g, "cuda")).sum(dim=0)
            total[0] = m if total[0] is None else total[0] + m
            count[0] += g.shape[0] * (g.shape[1] - 2) * (g.shape[2] - 2)
        return [None] * len(fnames)

    chunk.prefetch = lambda fnames, kws: (load_planes_u8(fnames),)
    fabrika.precovers(iterator="batched", convert_to=None, ignore_missing=True, batch_size=batch_size)(chunk)(
        data_dir, split=split, take_num_images=take_num_images)
    moments = total[0].cpu().numpy()
    taps, ok = fit(moments, symmetric)
    return DatasetFit(taps, ok, moments, count[0])


def main(argv=None) -> None:
    import argparse
    ap = argparse.ArgumentParser(description="fit a least-squares 3x3 pixel predictor on the cover images of a data set")
    ap.add_argument("--data", required=True, help="dataset root with images*/files.csv (the reference's ../data)")
    ap.add_argument("--split", default=None, help="split file under --data, e.g. split_tr.csv (default: every cover)")
    ap.add_argument("--take", type=int, default=None, help="the first N images")
    ap.add_argument("--symmetric", action="store_true", help="two parameters (edge, corner); the entry is named OLS2")
    ap.add_argument("--out", required=True, help="kernels.json; an existing file keeps its other entries")
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    res = fit_dataset(a.data, split=a.split, take_num_images=a.take, symmetric=a.symmetric)
    name = "OLS2" if a.symmetric else "OLS"
    if not res.ok:
        logging.warning(f"{name}: singular or ill-conditioned normal equations; writing KB's taps")
    out = pathlib.Path(a.out)
    kernels = load_kernels(out) if out.exists() else {}
    kernels[name] = res.taps
    save_kernels(out, kernels)
    with np.printoptions(precision=6, suppress=True):
        print(f"{name} taps (x00 x01 x02 x12 x22 x21 x20 x10): {res.taps}")
    print(f"{name} residual mse {residual_mse(res.moments, res.taps, res.count):.6f}   "
          f"KB residual mse {residual_mse(res.moments, _kb(), res.count):.6f}   over {res.count} pixels")
    print(f"output saved to {out}")


if __name__ == "__main__":
    main()
