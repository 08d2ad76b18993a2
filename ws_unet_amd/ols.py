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

import numpy as np

from . import filters, lsq
from .lsq import COND_MAX, DatasetFit                        # (also names of this module)

# edge and corner taps of the ring x00 x01 x02 x12 x22 x21 x20 x10: the two parameters of the symmetric fit
SYMMETRIC = np.zeros((8, 2))
SYMMETRIC[1::2, 0] = 1.
SYMMETRIC[0::2, 1] = 1.
ADAPTIVE_NAMES = {"OLSa": False, "OLSa2": True}              # model name -> symmetric


def _kb() -> np.ndarray:
    return filters.NAMED_FILTERS["KB"][:, 0].copy()


def _show(name, taps) -> str:
    with np.printoptions(precision=6, suppress=True):
        return f"{name} taps (x00 x01 x02 x12 x22 x21 x20 x10): {taps}"


# the 3x3 window: 8 neighbours and the centre, 45 moments.  lsq.Window has the fit; `fit` returns (taps8 (8,) float64, ok) and with
# symmetric=True fits the two parameters of SYMMETRIC, judged on the folded 2x2 system; load_kernels(register=True) enters a kernel
# file's {"OLS": [8 taps], ...} into the filter registry
WINDOW = lsq.Window(vars=9, symmetric=SYMMETRIC, kb=_kb, moments_op="ols_moments", margin=1, register=filters.register_filter,
                    size="3x3", label="OLS", entries=("OLS", "OLS2"), file="kernels.json", symmetric_help="two parameters (edge, corner)",
                    show=_show)
unpack, fit, residual_mse = WINDOW.unpack, WINDOW.fit, WINDOW.residual_mse
save_kernels, load_kernels = WINDOW.save_kernels, WINDOW.load_kernels
fit_dataset, main = WINDOW.fit_dataset, WINDOW.main


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

    def kernels(self, x_u8):
        """(N,H,W) uint8 device planes -> (N,3,3,1) float32 kernels in the layout of filters.NAMED_FILTERS_2D."""
        from . import ops
        taps, ok = fit(ops.ols_moments(x_u8).cpu().numpy(), self.symmetric)
        WINDOW.note(self, ok)
        return np.stack([filters.kernel_2d(t) for t in taps])

    def device_arguments(self, x_u8, correct_bias: bool = False) -> dict:
        """The statistic kernels' keywords (ws.estimate.predictor_arguments): one filter per image, evaluated in the kernel."""
        return dict(pixel_filter=self.kernels(x_u8)[..., ::-1])

    def __call__(self, x: np.ndarray) -> np.ndarray:
        import torch
        from .imread import u8_plane
        plane = u8_plane(np.asarray(x)[..., 0], "the OLS fit needs integer pixel values in 0..255")
        kernel = self.kernels(torch.from_numpy(np.ascontiguousarray(plane))[None].cuda())[0]
        return filters.infere_single(x, kernel)


def adaptive_estimator(model_name: str):
    """'OLSa' / 'OLSa2' -> a fresh AdaptiveOLSEstimator, any other name -> None."""
    return AdaptiveOLSEstimator(ADAPTIVE_NAMES[model_name]) if model_name in ADAPTIVE_NAMES else None


if __name__ == "__main__":
    main()
