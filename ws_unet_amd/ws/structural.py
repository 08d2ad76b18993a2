"""Structural LSB-replacement payload estimators beside the weighted-stego ones of ws.estimate / ws.roc: Sample Pairs Analysis
(Dumitrescu, Wu, Wang 2003) and RS analysis (Fridrich, Goljan, Du 2001).  Neither is part of the reference; they are the estimators
the WS literature measures itself against.

Both follow the package's pattern for per-image statistics: the device counts exact integers over every pixel (ops.spa_tables, K25;
ops.rs_counts, K26) and a few float64 operations per image solve a quadratic.  `spa` and `rs` are that solve, written once for numpy
arrays (the host API) and torch tensors (the device batch of `StructuralEstimator.beta`, which never waits for the GPU).

SPA.  Pairs are all horizontally and vertically adjacent pixels (u,v); d = |u-v|, m = d >> 1.  tables[...,0,m] = E[m] (d even),
[...,1,m] = X[m] (d odd, max(u,v) even: the halves u >> 1, v >> 1 differ by m + 1), [...,2,m] = Y[m] (d odd, max odd: the halves differ
by m).  C_m = E[m] + Y[m] + X[m-1] pairs have halves that differ by m (X[-1] = 0, C_128 = E[128] = 0).  LSB replacement of a fraction p
leaves sum_{m<=j} (Y[m] - X[m]) = 0 in expectation on the cover, which gives, with s = sum_{m=0..j} (Y[m] - X[m]) on the image at hand,

    (2 C_0 - C_{j+1}) / 4 * p^2  -  (2 E[0] - E[j+1] + 2 s) / 2 * p  +  s  =  0,        p = the root of smaller absolute value.

RS.  counts[...,0:4] = R_M, S_M, R_-M, S_-M of the plane (groups of 4 pixels of a row, mask (0,1,1,0)), [...,4:8] the same of the plane
with every LSB flipped.  With d0 = R_M - S_M, d-0 = R_-M - S_-M and d1, d-1 on the flipped plane,

    2 (d1 + d0) z^2  +  (d-0 - d-1 - d1 - 3 d0) z  +  (d0 - d-0)  =  0,        z = the root of smaller absolute value,  p = z / (z - 1/2).

Both return NaN where the leading coefficient is 0, where the discriminant is negative and (RS) where z = 1/2.  The coefficients are
sums of a few counts, exact in float64 below 2^53; the root's error is a few eps * |b / a| (~1e-14 near p = 0, where it cancels).

p is the payload in bits per pixel.  `StructuralEstimator.beta` returns p / 2, the change rate, which is what `beta_hat` means in every
table of ws.estimate and ws.roc."""
from __future__ import annotations

import numpy as np
import torch

NAMES = ("SPA", "RS")


def _f64(a):
    """(array or tensor of counts as float64, its namespace: torch or numpy)"""
    if isinstance(a, torch.Tensor):
        return a.to(torch.float64), torch
    return np.asarray(a).astype(np.float64), np


def _smaller_root(a, b, c, xp):
    """The root of a x^2 + b x + c of smaller absolute value; NaN where a = 0 or the discriminant is negative."""
    disc = b * b - 4. * a * c
    sq = xp.sqrt(xp.where(disc < 0., disc * 0., disc))
    r1, r2 = (-b + sq) / (2. * a), (-b - sq) / (2. * a)
    r = xp.where(abs(r1) <= abs(r2), r1, r2)
    return xp.where((a == 0.) | (disc < 0.), r * 0. + float("nan"), r)


def spa(tables, j: int = 30):
    """tables (...,3,128) counts (numpy array or torch tensor) -> p (...) float64 of the same kind.  j: the largest m whose pairs enter
    (30 is the usual choice, 127 uses every pair)."""
    if not 0 <= int(j) <= 127:
        raise ValueError(f"spa: j must be in 0..127, got {j}")
    if tuple(tables.shape[-2:]) != (3, 128):
        raise ValueError(f"spa: tables of shape (...,3,128) expected, got {tuple(tables.shape)}")
    t, xp = _f64(tables)
    j = int(j)
    E, X, Y = t[..., 0, :], t[..., 1, :], t[..., 2, :]
    s = (Y - X)[..., :j + 1].sum(-1)
    c0 = E[..., 0] + Y[..., 0]
    e_next = E[..., j + 1] if j < 127 else s * 0.
    c_next = e_next + Y[..., j + 1] + X[..., j] if j < 127 else s * 0.
    with np.errstate(divide="ignore", invalid="ignore"):
        return _smaller_root((2. * c0 - c_next) / 4., -(2. * E[..., 0] - e_next + 2. * s) / 2., s, xp)


def rs(counts):
    """counts (...,8) (numpy array or torch tensor) -> p (...) float64 of the same kind."""
    if tuple(counts.shape[-1:]) != (8,):
        raise ValueError(f"rs: counts of shape (...,8) expected, got {tuple(counts.shape)}")
    t, xp = _f64(counts)
    d0, dm0 = t[..., 0] - t[..., 1], t[..., 2] - t[..., 3]
    d1, dm1 = t[..., 4] - t[..., 5], t[..., 6] - t[..., 7]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = _smaller_root(2. * (d1 + d0), dm0 - dm1 - d1 - 3. * d0, d0 - dm0, xp)
        return xp.where(z == .5, z * 0. + float("nan"), z / (z - .5))


def require_unweighted(weighted, correct_bias) -> None:
    """Local-variance weights and the bias term are notions of the WS statistic; a structural estimator has neither."""
    if int(weighted) != 0 or correct_bias:
        raise ValueError(f"structural estimators {NAMES} take weighted=0 and correct_bias=False, got weighted={weighted} "
                         f"correct_bias={correct_bias}")


class StructuralEstimator:
    """'SPA' (with its j) or 'RS' as an estimator of ws.estimate / ws.roc: `.beta` is the whole statistic (no pixel predictor)."""

    def __init__(self, name: str, j: int = 30):
        if name not in NAMES:
            raise ValueError(f"unknown structural estimator {name!r}; choose from {NAMES}")
        if not 0 <= int(j) <= 127:
            raise ValueError(f"spa: j must be in 0..127, got {j}")
        self.name, self.j = name, int(j)

    def beta(self, x_u8: torch.Tensor) -> torch.Tensor:
        """x_u8: device (N,H,W) uint8 -> device float64 (N,): p / 2, the estimated change rate (NaN where the estimator has no answer).
        Kernel and solve are queued on the current stream; nothing waits for them."""
        from .. import ops
        if self.name == "SPA":
            return spa(ops.spa_tables(x_u8), self.j) / 2.
        return rs(ops.rs_counts(x_u8)) / 2.
