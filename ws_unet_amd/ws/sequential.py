"""The WS estimator for sequentially placed payloads (Ker, "A weighted stego image detector for sequential LSB replacement", SPIE 2007)
beside the uniform-placement one of ws.estimate.  Not part of the reference.

Most LSB-replacement tools write the message into the first pixels in file order: row by row from the top, or from the bottom row for
BMP-style tools.  The WS statistic of ws.estimate assumes a payload spread uniformly over the image; on a sequential payload its
local-variance weights pick up whatever region the message happens to lie in, and the estimate is badly off.

Derivation.  Let the used pixels be the path positions 1..k.  A used pixel of the stego image s is its cover value or that value with
the LSB flipped, so its cover estimate is (s + s_bar) / 2 with s_bar = s ^ 1; an unused pixel's is s itself.  Against the prediction
s_hat the weighted squared error is

    E(k) = sum_{i <= k} w_i ((s_i + s_bar_i) / 2 - s_hat_i)^2  +  sum_{i > k} w_i (s_i - s_hat_i)^2 .

With (s + s_bar) / 2 = s - (s - s_bar) / 2 and (s - s_bar)^2 = 1, a used pixel's term is w ((s - s_hat)^2 - (s - s_bar)(s - s_hat) + 1/4),
so E(k) = sum_i w_i (s_i - s_hat_i)^2 - T(k) with

    T(k) = sum_{i <= k} w_i (r_i - 1/4),     r_i = (s_i - s_bar_i)(s_i - s_hat_i),     T(0) = 0,

and the estimate is the k that maximises T: a changepoint of the cumulative sum of the very per-pixel terms the WS statistic averages
(E[r] = 1/2 on a used pixel, 0 on an unused one).  ops.ws_sequential (K27) forms the terms in float32 as wsu_ws_attack does, adds them
as fixed-point integers (2^24 units, so the maximum-prefix reduction is exact and order-independent) and returns the first maximiser k
over the path of INTERIOR pixels, row by row, left to right, rows from the top ('rows') or from the bottom ('rows_up').

`payload` turns k into the payload in bits per pixel of the whole plane, written once for numpy arrays and torch tensors (the device
batch never waits for the GPU).  The message's own path runs over the whole plane, border included: p_hat = 0 for k = 0; otherwise the
k-th interior pixel of the path sits at plane position (r, c), and p_hat = (its 1-based position on the whole-plane path) / (H W).  For
'rows' that is (r W + c + 1) / (H W), for 'rows_up' ((H - 1 - r) W + c + 1) / (H W).  `beta` = p_hat / 2 is the change rate, which is what
`beta_hat` means in every table of ws.estimate and ws.roc."""
from __future__ import annotations

import numpy as np
import torch

PLACEMENTS = ("random", "sequential", "adaptive")      # 'adaptive': along a recomputed cost order, ws/adaptive.py
ORDERS = ("rows", "rows_up")


def check_placement(placement, order) -> None:
    if placement not in PLACEMENTS:
        raise ValueError(f"unknown placement {placement!r}; choose from {PLACEMENTS}")
    if order not in ORDERS:
        raise ValueError(f"unknown order {order!r}; choose from {ORDERS}")


def payload(k, h: int, w: int, order: str = "rows"):
    """k: changepoints in 0..(H-2)(W-2) (int, numpy array or torch tensor) -> p_hat in float64 of the same kind."""
    if order not in ORDERS:
        raise ValueError(f"unknown order {order!r}; choose from {ORDERS}")
    h, w = int(h), int(w)
    if h < 3 or w < 3:
        raise ValueError(f"payload: a plane of at least 3 x 3 pixels expected, got {h} x {w}")
    xp = torch if isinstance(k, torch.Tensor) else np
    k = k.to(torch.int64) if xp is torch else np.asarray(k).astype(np.int64)
    j = xp.where(k > 0, k - 1, k * 0)                        # 0-based index of the last used interior pixel on the interior path
    pr = j // (w - 2) + 1                                    # rows of the plane the path has fully passed or is in, border row included
    c = j % (w - 2) + 1
    pos = (pr * w + c + 1)                                   # 'rows': pr = r; 'rows_up': pr = H - 1 - r
    p = (pos.to(torch.float64) if xp is torch else pos.astype(np.float64)) / float(h * w)
    return xp.where(k > 0, p, p * 0.)


def beta(k, h: int, w: int, order: str = "rows"):
    """The change rate p_hat / 2 (float64)."""
    return payload(k, h, w, order) / 2.
