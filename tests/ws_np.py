"""numpy-only restatement of the WS payload estimate K11 (include/wsu.h, ws_unet_amd/csrc/ws_attack.hip), one image at a time, with its
three sums taken exactly.

terms: the per-pixel float32 sequence of ws_pixel_terms (csrc/wsu_metric.h), every operation a separate float32 rounding: mu, mu2 by a true
convolution summed K00 .. K22 from 0, var = mu2 - mu * mu, t = 5 + var, wgt = 1 / t (weighted 1) | t (-1) | 1 (0), s = x - (x ^ 1), the
prediction x_hat = conv(x / 255, K) * 255 from a filter or y * hat_scale from a tensor (full frame or interior), the bias
conv(-+(1 / 255), K) * 255 or x_bias * hat_scale, res = x - x_hat, ws = wgt * s, and the terms wgt, ws * res, ws * bias.
sums: math.fsum of the terms widened to float64 -- the exact sums, rounded once -- and the sums of their absolute values.
finish: the kernel's few float64 operations: b = sb / sw, NaN stays NaN, negative -> 0, b -= b * (sc / sw) with correct_bias, float32(b)."""
import math

import numpy as np

from sequential_np import _conv9


def terms(x, x_hat=None, x_bias=None, hat_scale=255., pixel_kernel=None, mean_kernel=None, weighted=1, correct_bias=False):
    """x: (H,W) uint8.  x_hat (and x_bias with it): (H,W) full frames or (H-2,W-2) interiors, float32, multiplied by hat_scale; or
    pixel_kernel (3,3) K[a][b].  -> float32 (H-2,W-2) arrays (wgt, ws * res, ws * bias); the last is ws * 0 without correct_bias."""
    x = np.asarray(x, dtype=np.uint8)
    h, w = x.shape
    assert (x_hat is None) != (pixel_kernel is None) and int(weighted) in (-1, 0, 1)
    f255 = np.float32(255.0)
    u = [[x[i:h - 2 + i, j:w - 2 + j] for j in range(3)] for i in range(3)]
    v = [[p.astype(np.float32) for p in row] for row in u]
    with np.errstate(all="ignore"):
        wgt = np.ones((h - 2, w - 2), dtype=np.float32)
        if weighted:
            v2 = [[p * p for p in row] for row in v]
            mu, mu2 = _conv9(mean_kernel, v), _conv9(mean_kernel, v2)
            var = mu2 - mu * mu
            t = np.float32(5.0) + var
            wgt = np.float32(1.0) / t if weighted > 0 else t
        xc = v[1][1]
        s = xc - (u[1][1] ^ 1).astype(np.float32)
        bias = np.zeros((h - 2, w - 2), dtype=np.float32)
        if pixel_kernel is not None:
            hat = _conv9(pixel_kernel, [[p / f255 for p in row] for row in v]) * f255
            if correct_bias:
                one = np.float32(1.0) / f255                                  # (x_bar - x) / 255 = -1/255 at an odd pixel, +1/255 at an even one
                bias = _conv9(pixel_kernel, [[np.where(p & 1, -one, one).astype(np.float32) for p in row] for row in u]) * f255
        else:
            def inner(a):
                a = np.asarray(a, dtype=np.float32)
                a = a[1:-1, 1:-1] if a.shape == (h, w) else a
                assert a.shape == (h - 2, w - 2), a.shape
                return a
            hat = inner(x_hat) * np.float32(hat_scale)
            if correct_bias:
                bias = inner(x_bias) * np.float32(hat_scale)
        res = xc - hat
        ws = wgt * s
        out = wgt, ws * res, ws * bias
    assert all(a.dtype == np.float32 for a in out)
    return out


def _fsum(a):
    try:
        return math.fsum(a)
    except (ValueError, OverflowError):                     # +inf and -inf among the terms
        return float("nan")


def sums(term_arrays):
    """(wgt, ws * res, ws * bias) -> float64 (3,) exact sums (sw, sb, sc) and float64 (3,) sums of the absolute terms."""
    wide = [np.asarray(a, dtype=np.float64).reshape(-1) for a in term_arrays]
    return np.array([_fsum(a) for a in wide]), np.array([_fsum(np.abs(a)) for a in wide])


def finish(sw, sb, sc, correct_bias):
    """float64 sums -> float32 beta_hat"""
    sw, sb, sc = np.float64(sw), np.float64(sb), np.float64(sc)
    with np.errstate(all="ignore"):
        b = sb / sw
        if b < 0.0:                                         # a NaN fails the comparison and stays
            b = np.float64(0.0)
        if correct_bias:
            b = b - b * (sc / sw)
        return np.float32(b)


def attack(x, correct_bias=False, **kw):
    """One image -> (beta_hat float32, sums float64 (3,), sums of absolute terms float64 (3,)); keywords as `terms`."""
    s, a = sums(terms(x, correct_bias=correct_bias, **kw))
    return finish(s[0], s[1], s[2], correct_bias), s, a
