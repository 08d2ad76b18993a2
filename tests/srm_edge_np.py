"""numpy-only restatement of the counts of the SRM EDGE classes (include/wsu.h K55) and of the features made from them
(ws_unet_amd/srm.py `features_edge`), written from the definition in srm_minmax_np's shape: four edge residuals per pixel and class
(the half of the 3x3 or 5x5 kernel on one side of its centre row or column), eleven sets of them, a table counts the runs of four lo
digits and, negated, of four hi digits; a singleton set has lo = hi.  Vectorised over the batch."""
import numpy as np

import srm_minmax_np as mm_np
import srm_np


def _edges(kernel):
    """U: the kernel's rows from its top to its centre row, around the centre; D: U flipped top to bottom; L: U transposed; R: L mirrored"""
    k = len(kernel) // 2
    U = {(i - k, j - k): kernel[i][j] for i in range(k + 1) for j in range(2 * k + 1)}
    return {"U": U, "D": {(-dr, dc): wt for (dr, dc), wt in U.items()}, "L": {(dc, dr): wt for (dr, dc), wt in U.items()},
            "R": {(dc, -dr): wt for (dr, dc), wt in U.items()}}


# the eleven sets in order: name -> members
SETS = {"U": "U", "D": "D", "L": "L", "R": "R", "UL": "UL", "UR": "UR", "DL": "DL", "DR": "DR", "UD": "UD", "LR": "LR", "UDLR": "UDLR"}
# class -> (its q2 ascending: the steps of S3x3 / S5x5, its residuals: name -> taps {(dr, dc): weight} around the pixel)
CLASSES = {"E3": ((8, 12, 16), _edges(srm_np.KB)), "E5": ((24, 36, 48), _edges(srm_np.KV))}
assert CLASSES["E3"][1]["U"] == {(-1, -1): -1, (-1, 0): 2, (-1, 1): -1, (0, -1): 2, (0, 0): -4, (0, 1): 2}
# the 132 tables in order: (class, q2, set, scan)
TABLES = [(cls, q2, name, scan) for cls, (steps, _) in CLASSES.items() for q2 in steps for name in SETS for scan in "hv"]
# the reach (up, down, left, right) of every set as the definition states it (reach() below derives it from the taps)
REACH = {cls: {"U": (k, 0, k, k), "D": (0, k, k, k), "L": (k, k, k, 0), "R": (k, k, 0, k), "UL": (k, k, k, k), "UR": (k, k, k, k),
               "DL": (k, k, k, k), "DR": (k, k, k, k), "UD": (k, k, k, k), "LR": (k, k, k, k), "UDLR": (k, k, k, k)}
         for cls, k in (("E3", 1), ("E5", 2))}
# the submodels of a (class, q2) in order: name -> (the (set, scan) tables it sums, the fold: 169 sign-and-reversal orbits or 325 reversal orbits)
SUBMODELS = {
    "spam14h": ((("U", "h"), ("D", "h"), ("L", "v"), ("R", "v")), 169),
    "spam14v": ((("U", "v"), ("D", "v"), ("L", "h"), ("R", "h")), 169),
    "24": (tuple((s, scan) for s in ("UL", "UR", "DL", "DR") for scan in "hv"), 325),
    "22h": ((("UD", "h"), ("LR", "v")), 325),
    "22v": ((("UD", "v"), ("LR", "h")), 325),
    "41": ((("UDLR", "h"), ("UDLR", "v")), 325),
}
BINS, CENTRE, DIM = 625, 312, 9828


def reach(cls, name):
    """(up, down, left, right) of the union of the taps of the set's members"""
    taps = [t for member in SETS[name] for t in CLASSES[cls][1][member]]
    return (-min(dr for dr, _ in taps), max(dr for dr, _ in taps), -min(dc for _, dc in taps), max(dc for _, dc in taps))


def ab(cls, name, scan):
    """the (a, b) of the table's total 2 max(h - a, 0) max(w - b, 0)"""
    u, dn, l, rt = REACH[cls][name]
    return (u + dn, l + rt + 3) if scan == "h" else (u + dn + 3, l + rt)


def totals(h, w):
    """the 132 totals of an h x w image"""
    return [2 * max(h - a, 0) * max(w - b, 0) for cls, _, name, scan in TABLES for a, b in [ab(cls, name, scan)]]


def members(x, cls, name):
    """x (N,H,W) int64 -> the member residuals of the set at every pixel at which all the set's taps lie in the image, (M, N, H', W')"""
    n, h, w = x.shape
    u, dn, l, rt = reach(cls, name)
    hh, ww = max(h - u - dn, 0), max(w - l - rt, 0)
    out = np.zeros((len(SETS[name]), n, hh, ww), dtype=np.int64)
    if hh and ww:
        for k, member in enumerate(SETS[name]):
            for (dr, dc), wt in CLASSES[cls][1][member].items():
                out[k] += wt * x[:, u + dr:u + dr + hh, l + dc:l + dc + ww]
    return out


def counts(x_u8, plain=False):
    """(N,132,625) int64 of (N,H,W) uint8 planes.  plain=True: ONE update per run, the run of the lo digits alone (what a linear residual's
    table is; of a singleton set its min/max table is this one plus this one with every digit negated)"""
    x = np.asarray(x_u8)
    assert x.dtype == np.uint8 and x.ndim == 3
    x = x.astype(np.int64)
    out, cache = [], {}
    for cls, q2, name, scan in TABLES:
        if (cls, name) not in cache:
            cache[cls, name] = members(x, cls, name)
        D = srm_np.digit(cache[cls, name], q2)
        lo, hi = np.minimum.reduce(D), np.maximum.reduce(D)
        out.append(srm_np.table(lo, scan) + (0 if plain else srm_np.table(-hi, scan)))
    return np.stack(out, axis=1)


def features(c):
    """(N,132,625) counts -> (N,9828) float64: per (class, q2) its six submodels, each the sum of its tables, folded to 169 or 325 orbits
    and divided by its own sum"""
    c = np.asarray(c).astype(np.int64)
    at = {t: i for i, t in enumerate(TABLES)}
    orb = {169: srm_np.orbits(), 325: mm_np.orbits()}
    out = []
    for cls, (steps, _) in CLASSES.items():
        for q2 in steps:
            for tables, fold in SUBMODELS.values():
                b = sum(c[:, at[cls, q2, name, scan]] for name, scan in tables)
                f = np.stack([b[:, o].sum(axis=1) for o in orb[fold]], axis=1)
                s = f.sum(axis=1, keepdims=True)
                if (s == 0).any():
                    raise ValueError("a submodel without a run")
                out.append(f.astype(np.float64) / s.astype(np.float64))
    return np.concatenate(out, axis=1)
