"""numpy-only restatement of the counts of the linear SRM submodels (include/wsu.h K49) and of the features made from them
(ws_unet_amd/srm.py; Fridrich, Kodovsky 2012), written from the definition: every residual is a sum of shifted slices over the centres
whose taps all lie in the image, a table counts four digits in a row of that plane, the orbits are found by enumeration.  Vectorised over
the batch.  The discriminant and the AUC are spam_np's."""
import itertools

import numpy as np

from spam_np import auc, fld_fit, fld_output  # noqa: F401  (the same discriminant)

KB = ((-1, 2, -1), (2, -4, 2), (-1, 2, -1))
KV = ((-1, 2, -2, 2, -1), (2, -6, 8, -6, 2), (-2, 8, -12, 8, -2), (2, -6, 8, -6, 2), (-1, 2, -2, 2, -1))
# class -> (its q2 = 2q ascending, its residuals: name -> the taps {(dr, dc): weight} around the centre)
CLASSES = {
    "S1": ((2, 4), {"h": {(0, 0): -1, (0, 1): 1}, "v": {(0, 0): -1, (1, 0): 1}}),
    "S2": ((4, 6, 8), {"h": {(0, -1): 1, (0, 0): -2, (0, 1): 1}, "v": {(-1, 0): 1, (0, 0): -2, (1, 0): 1}}),
    "S3": ((6, 9, 12), {"h": {(0, -1): 1, (0, 0): -3, (0, 1): 3, (0, 2): -1}, "v": {(-1, 0): 1, (0, 0): -3, (1, 0): 3, (2, 0): -1}}),
    "S3x3": ((8, 12, 16), {"n": {(i - 1, j - 1): KB[i][j] for i in range(3) for j in range(3)}}),
    "S5x5": ((24, 36, 48), {"n": {(i - 2, j - 2): KV[i][j] for i in range(5) for j in range(5)}}),
}
# the 44 tables in order: (class, q2, residual, scan)
TABLES = [(cls, q2, res, scan) for cls, (steps, ress) in CLASSES.items() for q2 in steps for res in ress for scan in "hv"]
# the (a, b) of a table's total max(h - a, 0) max(w - b, 0), as the issue's table states them
REACH = {"S1": {"hh": (0, 4), "hv": (3, 1), "vh": (1, 3), "vv": (4, 0)}, "S2": {"hh": (0, 5), "hv": (3, 2), "vh": (2, 3), "vv": (5, 0)},
         "S3": {"hh": (0, 6), "hv": (3, 3), "vh": (3, 3), "vv": (6, 0)}, "S3x3": {"nh": (2, 5), "nv": (5, 2)}, "S5x5": {"nh": (4, 7), "nv": (7, 4)}}
BINS, CENTRE, DIM = 625, 312, 3718


def totals(h, w):
    """the 44 totals of an h x w image"""
    return [max(h - a, 0) * max(w - b, 0) for cls, _, res, scan in TABLES for a, b in [REACH[cls][res + scan]]]


def residual(x, taps):
    """x (N,H,W) int64 -> the residual at every centre whose taps all lie in the image, (N, H', W') (an empty array where there is none)"""
    n, h, w = x.shape
    up, down = -min(dr for dr, _ in taps), max(dr for dr, _ in taps)
    left, right = -min(dc for _, dc in taps), max(dc for _, dc in taps)
    hh, ww = max(h - up - down, 0), max(w - left - right, 0)
    R = np.zeros((n, hh, ww), dtype=np.int64)
    if hh and ww:
        for (dr, dc), wt in taps.items():
            R += wt * x[:, up + dr:up + dr + hh, left + dc:left + dc + ww]
    return R


def digit(R, q2):
    """sign(R) min((4|R| + q2) / (2 q2), 2) in integers: R / q rounded half away from zero, cut to -2..2"""
    return np.sign(R) * np.minimum((4 * np.abs(R) + q2) // (2 * q2), 2)


def table(D, scan):
    """D (N,H',W') digits -> (N,625): the runs of four along a row (scan 'h') or down a column ('v'), first digit most significant"""
    n, hh, ww = D.shape
    if scan == "h":
        runs = [D[:, :, k:ww - 3 + k] for k in range(4)] if ww >= 4 else None
    else:
        runs = [D[:, k:hh - 3 + k, :] for k in range(4)] if hh >= 4 else None
    out = np.zeros((n, BINS), dtype=np.int64)
    if runs is None or runs[0].size == 0:
        return out
    idx = sum((d + 2) * 5 ** (3 - k) for k, d in enumerate(runs)).reshape(n, -1)
    for i in range(n):
        out[i] = np.bincount(idx[i], minlength=BINS)
    return out


def counts(x_u8):
    """(N,44,625) int64 of (N,H,W) uint8 planes"""
    x = np.asarray(x_u8)
    assert x.dtype == np.uint8 and x.ndim == 3
    x = x.astype(np.int64)
    out, cache = [], {}
    for cls, q2, res, scan in TABLES:
        if (cls, res) not in cache:
            cache[cls, res] = residual(x, CLASSES[cls][1][res])
        out.append(table(digit(cache[cls, res], q2), scan))
    return np.stack(out, axis=1)


def orbits():
    """The orbits of the digit tuples under (d0..d3) -> (-d0..-d3) and (d0..d3) -> (d3..d0), by enumeration: a list of lists of bins, the
    orbits in the order of their lexicographically smallest tuple."""
    seen, out = {}, []
    for t in itertools.product(range(-2, 3), repeat=4):                     # lexicographic
        if t in seen:
            continue
        neg, rev = tuple(-d for d in t), t[::-1]
        members = sorted({t, neg, rev, tuple(-d for d in rev)})
        assert members[0] == t
        for m in members:
            seen[m] = len(out)
        out.append([sum((d + 2) * 5 ** (3 - k) for k, d in enumerate(m)) for m in members])
    return out


def fold(T):
    """(.., 625) -> (.., 169): an orbit's value is the sum of its members' counts"""
    return np.stack([T[..., members].sum(axis=-1) for members in orbits()], axis=-1)


def features(c):
    """(N,44,625) counts -> (N,3718) float64: per (class, q) `par` = T[hh] + T[vv] then `perp` = T[hv] + T[vh], or the one T[nh] + T[nv];
    each folded to 169 orbits and divided by its own sum"""
    c = np.asarray(c).astype(np.int64)
    at = {t: i for i, t in enumerate(TABLES)}
    blocks = []
    for cls, (steps, ress) in CLASSES.items():
        for q2 in steps:
            if "n" in ress:
                blocks.append(c[:, at[cls, q2, "n", "h"]] + c[:, at[cls, q2, "n", "v"]])
            else:
                blocks.append(c[:, at[cls, q2, "h", "h"]] + c[:, at[cls, q2, "v", "v"]])
                blocks.append(c[:, at[cls, q2, "h", "v"]] + c[:, at[cls, q2, "v", "h"]])
    out = []
    for b in blocks:
        f = fold(b)
        s = f.sum(axis=1, keepdims=True)
        if (s == 0).any():
            raise ValueError("a block without a run")
        out.append(f.astype(np.float64) / s.astype(np.float64))
    return np.concatenate(out, axis=1)
