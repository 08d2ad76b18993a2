"""numpy-only restatement of the weighted sums of the linear SRM submodels (include/wsu.h K52) and of the 16-bit change weights (K51),
written from the header: K49's residuals, digits and tables (srm_np); the weight plane cut to the residual's centres; per run the largest
weight of its four positions by a running np.maximum; a weighted np.bincount into int64 (its float64 sums of integers stay below 2^53
for any plane of fewer than 2^37 pixels, so they are exact).  The weight of a pixel is
floor((p+ + p-) * 65536) of pm1_np.probabilities."""
import numpy as np

import pm1_np
import srm_np
from srm_np import BINS, TABLES


def centres(plane, taps):
    """plane (N,H,W) cut to the positions of the residual with these taps: where srm_np.residual has its values"""
    n, h, w = plane.shape
    up, down = -min(dr for dr, _ in taps), max(dr for dr, _ in taps)
    left, right = -min(dc for _, dc in taps), max(dc for _, dc in taps)
    return plane[:, up:up + max(h - up - down, 0), left:left + max(w - left - right, 0)]


def table(D, Wc, scan):
    """D (N,H',W') digits, Wc (N,H',W') int64 weights at the same positions -> (N,625) int64: every run of four along a row (scan 'h') or
    down a column ('v') adds the largest of its four weights to its bin"""
    n, hh, ww = D.shape
    out = np.zeros((n, BINS), dtype=np.int64)
    if (ww if scan == "h" else hh) < 4 or hh == 0 or ww == 0:
        return out
    cut = (lambda A, k: A[:, :, k:ww - 3 + k]) if scan == "h" else (lambda A, k: A[:, k:hh - 3 + k, :])
    idx = sum((cut(D, k) + 2) * 5 ** (3 - k) for k in range(4)).reshape(n, -1)
    wmax = cut(Wc, 0)
    for k in range(1, 4):
        wmax = np.maximum(wmax, cut(Wc, k))
    wmax = wmax.reshape(n, -1)
    for i in range(n):                                                    # float64 sums of integers below 2^53: exact
        out[i] = np.bincount(idx[i], weights=wmax[i].astype(np.float64), minlength=BINS).astype(np.int64)
    return out


def sums(x_u8, weights):
    """(N,44,625) int64 of (N,H,W) uint8 planes and (N,H,W) integer weights"""
    x, wt = np.asarray(x_u8), np.asarray(weights)
    assert x.dtype == np.uint8 and x.ndim == 3 and wt.shape == x.shape
    x, wt = x.astype(np.int64), wt.astype(np.int64)
    out, cache = [], {}
    for cls, q2, res, scan in TABLES:
        taps = srm_np.CLASSES[cls][1][res]
        if (cls, res) not in cache:
            cache[cls, res] = srm_np.residual(x, taps), centres(wt, taps)
        R, Wc = cache[cls, res]
        out.append(table(srm_np.digit(R, q2), Wc, scan))
    return np.stack(out, axis=1)


def beta_scaled(x, rho, lam):
    """(p+ + p-) * 65536 in float64, per pixel"""
    pp, pm = pm1_np.probabilities(x, rho, lam)
    return (pp + pm) * 65536.0


def change_weights(x, rho, lam):
    """floor((p+ + p-) * 65536) as uint16 (beta <= 2/3: at most 43 690)"""
    return np.floor(beta_scaled(x, rho, lam)).astype(np.uint16)


def near_boundary(x, rho, lam, eps=1e-6):
    """how many pixels have beta * 65536 within eps of a positive integer: where a last-bit difference could move the floor"""
    b = beta_scaled(x, rho, lam)
    near = np.abs(b - np.rint(b)) <= eps
    return int(np.count_nonzero(near & (np.rint(b) >= 1)))


# the inputs of the K51 comparisons on the GPU: (content, shape of pm1_np.case, lambda, whether some costs are set to +inf).  The host test
# asserts that none of them has a pixel within 1e-6 of a positive integer boundary, so the GPU test may ask for equality.
K51_CASES = (("photo", (8, 8), 0.5, False), ("photo", (65, 130), 0.02, True), ("photo", (70, 90), 3.0, False), ("photo", (70, 90), np.inf, False),
             ("flat", (8, 8), 1e-10, False), ("flat", (70, 90), 1.0, True), ("ends", (65, 130), 0.1, False), ("ends", (70, 90), 0.7, True),
             ("ends", (8, 8), 2.0, False))


def k51_case(content, shape, lam, wet):
    """(x, rho, lam) of a K51 comparison: pm1_np.case's plane and HILL cost, every 15th pixel wet (rho = +inf) when asked"""
    x, rho = pm1_np.case(content, shape)
    if wet:
        rho = rho.copy()
        rho.reshape(-1)[::15] = np.inf
    return x, rho, float(lam)
