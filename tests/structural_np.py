"""numpy-only restatement of the sample-pairs table (K25), of the RS group counts (K26) and of the two payload solves, written from
their definitions (include/wsu.h; Dumitrescu, Wu, Wang 2003; Fridrich, Goljan, Du 2001), one image and one table at a time."""
import math

import numpy as np


def spa_table(x_u8):
    """(H,W) uint8 -> (3,128) int64 {E, X, Y}[m], or (N,H,W) -> (N,3,128).  Pairs: every horizontal and vertical neighbour pair (u,v);
    d = |u-v|, m = d // 2: E if d is even, X if d is odd and max(u,v) even, Y if d is odd and max(u,v) odd."""
    x = np.asarray(x_u8)
    if x.ndim == 3:
        return np.stack([spa_table(p) for p in x])
    x = x.astype(np.int64)
    u = np.concatenate([x[:, :-1].reshape(-1), x[:-1, :].reshape(-1)])
    v = np.concatenate([x[:, 1:].reshape(-1), x[1:, :].reshape(-1)])
    d, hi = np.abs(u - v), np.maximum(u, v)
    kind = np.where(d % 2 == 0, 0, np.where(hi % 2 == 0, 1, 2))
    return np.bincount(kind * 128 + d // 2, minlength=384).astype(np.int64).reshape(3, 128)


def _f(g):
    return np.abs(np.diff(g, axis=-1)).sum(axis=-1)


def _flip_pos(v):
    return v ^ 1


def _flip_neg(v):
    return ((v + 1) ^ 1) - 1                                   # 0 -> -1, 255 -> 256: not clamped


def rs_counts(x_u8):
    """(H,W) uint8 -> (8,) int64, or (N,H,W) -> (N,8): R_M, S_M, R_-M, S_-M over the groups x[r][4g..4g+3] with the mask (0,1,1,0),
    then the same four on x ^ 1."""
    x = np.asarray(x_u8)
    if x.ndim == 3:
        return np.stack([rs_counts(p) for p in x])
    h, w = x.shape
    out = []
    for plane in (x.astype(np.int64), x.astype(np.int64) ^ 1):
        g = plane[:, :w // 4 * 4].reshape(h, w // 4, 4)
        f0 = _f(g)
        for flip in (_flip_pos, _flip_neg):
            gm = g.copy()
            gm[..., 1], gm[..., 2] = flip(g[..., 1]), flip(g[..., 2])
            fm = _f(gm)
            out += [int((fm > f0).sum()), int((fm < f0).sum())]
    return np.array(out, dtype=np.int64)


def smaller_root(a, b, c):
    """root of a x^2 + b x + c of smaller absolute value in float64; NaN if a = 0 or there is no real root"""
    a, b, c = float(a), float(b), float(c)
    disc = b * b - 4. * a * c
    if a == 0. or disc < 0.:
        return math.nan
    roots = ((-b + math.sqrt(disc)) / (2. * a), (-b - math.sqrt(disc)) / (2. * a))
    return min(roots, key=abs)


def spa_p(table, j=30):
    """payload estimate of one (3,128) table"""
    E, X, Y = (np.append(np.asarray(table)[k].astype(np.int64), 0) for k in range(3))        # index 128: no such pair
    C = lambda m: int(E[m] + Y[m] + (X[m - 1] if m > 0 else 0))
    s = int(sum(int(Y[m]) - int(X[m]) for m in range(j + 1)))
    c_next = C(j + 1) if j + 1 < 128 else 0
    return smaller_root((2 * C(0) - c_next) / 4., -(2 * int(E[0]) - int(E[j + 1]) + 2 * s) / 2., s)


def rs_p(counts):
    """payload estimate of one (8,) vector of counts"""
    rm, sm, rn, sn, rm1, sm1, rn1, sn1 = (int(v) for v in np.asarray(counts))
    d0, dn0, d1, dn1 = rm - sm, rn - sn, rm1 - sm1, rn1 - sn1
    z = smaller_root(2 * (d1 + d0), dn0 - dn1 - d1 - 3 * d0, d0 - dn0)
    if math.isnan(z) or z == .5:
        return math.nan
    return z / (z - .5)
