"""HILL embedding cost and the numpy quantile index the wMAE threshold uses.

The reference's prediction evaluation rates a predictor by its MAE and its wMAE: the MAE over the 10 % of interior pixels with the
lowest HILL cost (src/filters/evaluate.py:79-115, src/predictor_error.py:19-76).  The two reference callers take HILL from
`conseal.hill._costmap.compute_cost` and `stegolab2.hill.compute_rho`; both are treated here as the textbook cost, the one pinned
by the published results/prediction/filters.csv:

    R = x (*) [[-1,2,-1],[2,-4,2],[-1,2,-1]];  rho0 = 1 / (box3x3(|R|) / 9);  cost = box15x15(rho0) / 225
    ('same' convolutions, boundary 'symm'), then cost[isinf | isnan | cost > 1e10] = 1e10.

`compute_cost` runs on the GPU (wsu_hill_cost); the maps are fp32, which ranks the pixels of the reference's covers exactly as the
float64 original does.
"""
from __future__ import annotations

import math
import typing

import numpy as np

CLAMP = 1e10


def quantile_index(count: int, quantile: float) -> typing.Tuple[int, float]:
    """(k, g) of numpy.quantile(..., method='linear') over `count` values: virtual index v = (count-1)*quantile in float64,
    k = floor(v), g = v - k; the result is a + (b-a)*g (b - (b-a)*(1-g) when g >= 0.5) with a = c_(k), b = c_(min(k+1, count-1)).
    At v >= count-1 numpy takes the last value: k = count-1, g = 0."""
    count = int(count)
    quantile = float(quantile)
    if count < 1:
        raise ValueError(f"quantile of {count} values")
    if not 0.0 <= quantile <= 1.0:
        raise ValueError(f"quantile {quantile} outside [0, 1]")
    v = float(count - 1) * quantile
    if v >= count - 1:
        return count - 1, 0.0
    k = int(math.floor(v))
    return k, v - k


def compute_cost(x, clamp: float = CLAMP):
    """HILL cost of one (H,W) or a batch (N,H,W) of uint8 planes, with the reference's clamp applied.  Takes a numpy array (the
    result is a numpy fp32 array) or a device tensor (the result stays on the device)."""
    import torch
    from . import ops
    is_np = isinstance(x, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda() if is_np else x
    if t.dtype != torch.uint8:
        raise TypeError(f"uint8 planes expected, got {t.dtype}")
    if t.dim() not in (2, 3):
        raise ValueError(f"(H,W) or (N,H,W) expected, got shape {tuple(t.shape)}")
    single = t.dim() == 2
    c = ops.hill_cost((t[None] if single else t).contiguous(), clamp)
    c = c[0] if single else c
    return c.cpu().numpy() if is_np else c
