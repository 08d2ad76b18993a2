"""The WS estimator for payloads placed in the order of an adaptivity criterion: the informed WS attack on naive content-adaptive
embedding (Schoettle, Korff, Boehme, "Weighted stego-image steganalysis for naive content-adaptive embedding", WIFS 2012) beside the
uniform-placement statistic of ws.estimate and the file-order changepoint of ws/sequential.py.  Not part of the reference.

The reference's HILLR puts every change into the pixels of lowest HILL cost.  The WS statistic with its weights 1 / (5 + var) looks
away from exactly those textured pixels, and its estimate of a HILLR payload is a fraction of the truth.  But the attacker can
recompute the criterion: the cost depends on the image through smoothed high-pass residuals, which LSB flips barely move, so the cost
of the STEGO image orders the pixels almost as the cover's did.  Along that order the payload is "sequential", and Ker's changepoint
argument applies with one more parameter.

Derivation.  Let the path visit the interior pixels in ascending order of the key, ties to the smaller raster index, and let the used
pixels be the path positions 1..k.  A used pixel was flipped with probability pi (`flip_rate`): pi = 1 for HILLR, which flips every
pixel up to its threshold, pi = 1/2 for a real message.  Its cover estimate is s - pi (s - s_bar) with s_bar = s ^ 1, an unused pixel's
is s itself.  Against the prediction s_hat, with (s - s_bar)^2 = 1, a used pixel's weighted squared error is

    w ((s - s_hat) - pi (s - s_bar))^2 = w ((s - s_hat)^2 - 2 pi ((s - s_bar)(s - s_hat) - pi / 2)),

so the error of the whole path is E(k) = sum_i w_i (s_i - s_hat_i)^2 - 2 pi T(k) with

    T(k) = sum_{i <= k} w_i (r_i - pi / 2),     r_i = (s_i - s_bar_i)(s_i - s_hat_i),     T(0) = 0,

and the estimate k_hat is the first maximiser of T over 0..M, M = (H-2)(W-2): E[r] = pi on a used pixel and 0 on an unused one, so the
terms drift upwards by pi / 2 per used pixel and downwards by as much after it.  pi = 1/2 gives the term r - 1/4 of ws/sequential.py.
The change rate is beta_hat = pi k_hat / M.  ops.ws_ordered (K33) forms the terms in float32 as wsu_ws_attack does, with
tau = (float32)(pi / 2), adds them as fixed-point integers (2^24 units) along the path and returns k_hat exactly.

What is NOT a kernel of this library: the order itself.  `path_for` computes the key with ops.hill_cost (K12) and sorts it with
torch.sort(stable=True) on the device (ops.interior_order).  The key is float32 and computed from the image under attack, not from
its cover, so the path differs from the embedder's on near-ties and wherever the embedding moved the cost; the estimator absorbs that
(tests/test_gpu_ws_adaptive.py holds the accuracy measured on the five fixture images, the only ones it was checked on)."""
from __future__ import annotations

import numpy as np
import torch

CRITERIA = ("hill",)


def check_options(criterion, flip_rate) -> None:
    if criterion not in CRITERIA:
        raise ValueError(f"unknown criterion {criterion!r}; choose from {CRITERIA}")
    try:
        ok = 0.0 < float(flip_rate) <= 1.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"flip_rate must lie in (0, 1] (1: every used pixel flipped, as HILLR does; 0.5: a real message), got {flip_rate!r}")


def path_for(x_u8: torch.Tensor, criterion: str = "hill") -> torch.Tensor:
    """x_u8: (N,H,W) uint8 on the device, the images under attack -> int32 (N,(H-2)(W-2)): the interior pixels in ascending order of the
    criterion recomputed from these very images ('hill': ops.hill_cost), ties to the smaller raster index."""
    from .. import ops
    if criterion not in CRITERIA:
        raise ValueError(f"unknown criterion {criterion!r}; choose from {CRITERIA}")
    return ops.interior_order(ops.hill_cost(x_u8))


def beta(k, h: int, w: int, flip_rate: float = 1.0):
    """k: changepoints in 0..(H-2)(W-2) (int, numpy array or torch tensor) -> the change rate flip_rate * k / M in float64 of the same kind."""
    check_options(CRITERIA[0], flip_rate)
    h, w = int(h), int(w)
    if h < 3 or w < 3:
        raise ValueError(f"beta: a plane of at least 3 x 3 pixels expected, got {h} x {w}")
    k = k.to(torch.float64) if isinstance(k, torch.Tensor) else np.asarray(k).astype(np.float64)
    return k * float(flip_rate) / float((h - 2) * (w - 2))
