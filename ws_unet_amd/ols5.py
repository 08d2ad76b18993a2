"""Least-squares 5x5 pixel predictors: the predictor of Ker and Boehme's "improved WS" ("Revisiting weighted stego-image steganalysis",
2008) in its full form (24 taps) and a symmetry-constrained form (5 parameters), fitted on the image under attack or on a data set.
The 3x3 counterparts and their 8-tap file format are ws_unet_amd.ols; moderated weights and bias correction are in wsu_ws_attack.

  * the device computes the exact integer moments of an image (ops.ols_moments5, K56): at every pixel with a full 5x5 window the 24
    neighbours x[r-2+a][c-2+b] in raster order of (a,b), the centre skipped, and the centre y, summed as the 325 products v_p * v_q,
    p <= q.  They hold A = X^T X (24x24), b = X^T y and y^T y, and they add over images;
  * the host solves the normal equations A k = b in float64 (`fit`; no intercept), per image or for summed moments; symmetric=True
    fits one parameter per class of neighbours at the same unordered (|dr|,|dc|): (0,1), (1,1), (0,2), (1,2), (2,2) -- 4, 4, 4, 8, 4 taps;
  * the device evaluates 24 float32 taps as full-frame planes (ops.predict5x5, K57): 0 on the frame border, KB on the ring inside it
    (where the 5x5 window leaves the image), the taps elsewhere, in K11's float32 operation sequence; the WS statistics take the planes
    as x_hat / x_bias with hat_scale = 1 (ws.estimate.predictor_arguments), so random, sequential and adaptive placement, ws.locate
    and ws.keysearch work with them unchanged;
  * `Predictor5x5` is that path as a pixel predictor: fixed taps, or fitted per image.  Model names 'OLSa5x5' (24 taps, fitted on each
    image under attack), 'OLSa5x5s' (5 parameters), and every name loaded from a 5x5 kernels file (`load_kernels`, the drivers'
    --kernels5), which `python -m ws_unet_amd.ols5` writes as {"OLS5x5": [24 floats]} / "OLS5x5s".

A fit is valid iff the matrix of the solved system is positive definite and its condition number is at most 1e12 (lsq.COND_MAX);
otherwise the taps are KB's, embedded in the 24, and ok is False.

NOT checked: the symmetric pattern is Ker and Boehme's as remembered, and nothing here was compared with their implementation.

    python -m ws_unet_amd.ols5 --data DIR [--split split_tr.csv] [--take N] [--symmetric] --out kernels5.json
"""
from __future__ import annotations

import numpy as np

from . import filters, lsq
from .lsq import DatasetFit                                  # (also a name of this module)
from .ols import ADAPTIVE_NAMES as _OLS3_NAMES

TAPS, VARS, MOMENTS = 24, 25, 325
# (dr, dc) of tap k: the 5x5 raster without its centre
OFFSETS = [(a - 2, b - 2) for a in range(5) for b in range(5) if (a, b) != (2, 2)]
CLASSES = ((0, 1), (1, 1), (0, 2), (1, 2), (2, 2))           # unordered (|dr|,|dc|): the five parameters of the symmetric fit
SYMMETRIC = np.zeros((TAPS, len(CLASSES)))
for _k, (_dr, _dc) in enumerate(OFFSETS):
    SYMMETRIC[_k, CLASSES.index(tuple(sorted((abs(_dr), abs(_dc)))))] = 1.
ADAPTIVE_NAMES = {"OLSa5x5": False, "OLSa5x5s": True}        # model name -> symmetric
KERNELS = {}                                                 # name -> (24,) float64 taps of the loaded 5x5 kernels files


def embed3x3(weights3x3) -> np.ndarray:
    """(3,3) weights of x[r-1+a][c-1+b] -> the 24 taps with those on the inner ring and zeros on the outer one (the centre's is dropped)."""
    full = np.zeros((5, 5))
    full[1:4, 1:4] = np.asarray(weights3x3, dtype=np.float64).reshape(3, 3)
    return np.delete(full.reshape(25), 12)


def _kb() -> np.ndarray:
    return embed3x3(filters.NAMED_FILTERS_2D["KB"][::-1, ::-1, 0])


# ---- files and registry -----------------------------------------------------------------------------------------------------------

def register_kernel(name: str, taps) -> None:
    """Enter fixed 5x5 taps under `name` as a model name of the WS drivers.  Registering a name again replaces it; the names of the 3x3
    filters and of the adaptive predictors are refused."""
    k = np.array(taps, dtype=np.float64)
    if k.shape != (TAPS,) or not np.all(np.isfinite(k)):
        raise ValueError(f"5x5 kernel {name!r}: {TAPS} finite taps expected, got shape {k.shape}")
    if not isinstance(name, str) or not name or name in filters.NAMED_FILTERS_2D or name in _OLS3_NAMES or name in ADAPTIVE_NAMES:
        raise ValueError(f"5x5 kernel name {name!r} is empty, a 3x3 filter's or an adaptive predictor's")
    KERNELS[name] = k


def _show(name, taps) -> str:
    with np.printoptions(precision=6, suppress=True, linewidth=140):
        return f"{name} taps (5x5 raster, the centre left out):\n{np.insert(taps, 12, np.nan).reshape(5, 5)}"


# the 5x5 window: 24 neighbours and the centre, 325 moments.  lsq.Window has the fit; `fit` returns (taps (24,) float64, ok) and with
# symmetric=True fits the five class parameters of SYMMETRIC, judged on the folded 5x5 system; an invalid fit returns KB's taps embedded
# in the 24; load_kernels(register=True) enters a kernel file's {"OLS5x5": [24 taps], ...} as model names (`register_kernel`)
WINDOW = lsq.Window(vars=VARS, symmetric=SYMMETRIC, kb=_kb, moments_op="ols_moments5", margin=2, register=register_kernel,
                    size="5x5", label="OLS 5x5", entries=("OLS5x5", "OLS5x5s"), file="kernels5.json",
                    symmetric_help="five parameters, one per (|dr|,|dc|) class", show=_show)
unpack, fit, residual_mse = WINDOW.unpack, WINDOW.fit, WINDOW.residual_mse
save_kernels, load_kernels = WINDOW.save_kernels, WINDOW.load_kernels
fit_dataset, main = WINDOW.fit_dataset, WINDOW.main


def add_kernels_argument(ap) -> None:
    """The drivers' `--kernels5 kernels5.json`."""
    ap.add_argument("--kernels5", default=None, metavar="kernels5.json",
                    help="fitted 5x5 predictors written by `python -m ws_unet_amd.ols5`; their names become valid filter names")


def register_from_args(a) -> None:
    if getattr(a, "kernels5", None):
        load_kernels(a.kernels5, register=True)


def names() -> list:
    """Every model name `estimator` answers: the adaptive ones and the registered fixed ones."""
    return sorted(ADAPTIVE_NAMES) + sorted(KERNELS)


# ---- the predictor ---------------------------------------------------------------------------------------------------------------------

class Predictor5x5:
    """A 5x5 linear pixel predictor: fixed `taps` (24, K56's variable order), or with adaptive=True the least-squares taps of each
    image, fitted on that image (the stego image under attack: no cover is needed; symmetric=True: the five-parameter form).
    `planes` keeps everything on the device: moments -> float64 fit on the host -> float32 taps -> K57's full frames, which
    ws.estimate.predictor_arguments hands to the statistic kernels.  Called on a host (H,W,C) array like the reference's estimators it
    predicts that one image and returns (H-2,W-2,1).  Images whose fit is invalid get KB's taps; `fallbacks` counts them and the first one
    is logged (once per predictor, i.e. per run)."""

    def __init__(self, taps=None, adaptive: bool = False, symmetric: bool = False):
        if (taps is None) != bool(adaptive):
            raise ValueError("Predictor5x5: give fixed taps or adaptive=True")
        if symmetric and not adaptive:
            raise ValueError("Predictor5x5: symmetric=True belongs to the adaptive fit; fixed taps are used as they are")
        self.adaptive, self.symmetric = bool(adaptive), bool(symmetric)
        self.taps = None
        if taps is not None:
            self.taps = np.array(taps, dtype=np.float64)
            if self.taps.shape != (TAPS,) or not np.all(np.isfinite(self.taps)):
                raise ValueError(f"Predictor5x5: {TAPS} finite taps expected, got shape {self.taps.shape}")
        self.fallbacks = 0

    def image_taps(self, x_u8):
        """(N,H,W) uint8 device planes -> float32 device taps: (24,) fixed, (N,24) fitted per image."""
        import torch
        from . import ops
        if not self.adaptive:
            return torch.from_numpy(self.taps.astype(np.float32)).to(x_u8.device)
        taps, ok = fit(ops.ols_moments5(x_u8).cpu().numpy(), self.symmetric)
        WINDOW.note(self, ok)
        return torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float32)).to(x_u8.device)

    def planes(self, x_u8, want_bias: bool = False):
        """(N,H,W) uint8 device planes -> x_hat float32 (N,H,W) in pixel units (hat_scale = 1), with want_bias (x_hat, x_bias)."""
        if x_u8.dim() != 3 or x_u8.shape[1] < 5 or x_u8.shape[2] < 5:
            raise ValueError(f"the 5x5 predictor needs (N,H,W) planes of at least 5 x 5 pixels, got {tuple(x_u8.shape)}")
        from . import ops
        return ops.predict5x5(x_u8, self.image_taps(x_u8), want_bias)

    def device_arguments(self, x_u8, correct_bias: bool = False) -> dict:
        """The statistic kernels' keywords (ws.estimate.predictor_arguments): K57's full frames in pixel units, with their own x_bias."""
        if not correct_bias:
            return dict(x_hat=self.planes(x_u8), hat_scale=1.0)
        x_hat, x_bias = self.planes(x_u8, want_bias=True)
        return dict(x_hat=x_hat, x_bias=x_bias, hat_scale=1.0)

    def __call__(self, x: np.ndarray) -> np.ndarray:
        import torch
        from .imread import u8_plane
        plane = u8_plane(np.asarray(x)[..., 0], "the 5x5 predictor needs integer pixel values in 0..255")
        hat = self.planes(torch.from_numpy(np.ascontiguousarray(plane))[None].cuda())[0]
        return hat[1:-1, 1:-1].cpu().numpy()[..., None]


def estimator(model_name: str):
    """'OLSa5x5' / 'OLSa5x5s' or a name loaded from a 5x5 kernels file -> a fresh Predictor5x5, any other name -> None."""
    if model_name in ADAPTIVE_NAMES:
        return Predictor5x5(adaptive=True, symmetric=ADAPTIVE_NAMES[model_name])
    return Predictor5x5(KERNELS[model_name]) if model_name in KERNELS else None


if __name__ == "__main__":
    main()
