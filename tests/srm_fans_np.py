"""numpy-only restatement of the counts of the SRM fan submodels (include/wsu.h K54) and of the features made from them
(ws_unet_amd/srm.py `features_fans`), written from the definition in srm_minmax_np's shape: eight directional residuals per pixel and
class, a set is a perpendicular pair or a run of adjacent directions, its digits are the minimum and the maximum over its members'
digits, a table counts the runs of four lo digits and, negated, of four hi digits.  Vectorised over the batch."""
import numpy as np

import srm_minmax_np as mm_np
import srm_np

# the eight directions counter-clockwise and their steps (dr, dc)
DIRECTIONS = {"E": (0, 1), "NE": (-1, 1), "N": (-1, 0), "NW": (-1, -1), "W": (0, -1), "SW": (1, -1), "S": (1, 0), "SE": (1, 1)}
# the 20 sets in order, named by their members: four perpendicular pairs, the four 3-fans centred on a diagonal, the eight 4-fans (the
# four "vertical" ones, which hold N or S with both its neighbours, then the four "horizontal" ones), the four 5-fans centred on a diagonal
PAIRS = ("E+N", "N+W", "W+S", "S+E")
FAN3 = ("E+NE+N", "N+NW+W", "W+SW+S", "S+SE+E")
FAN4_VERTICAL = ("E+NE+N+NW", "NE+N+NW+W", "W+SW+S+SE", "SW+S+SE+E")
FAN4_HORIZONTAL = ("N+NW+W+SW", "NW+W+SW+S", "S+SE+E+NE", "SE+E+NE+N")
FAN5 = ("SE+E+NE+N+NW", "NE+N+NW+W+SW", "NW+W+SW+S+SE", "SW+S+SE+E+NE")
SETS = {name: tuple(name.split("+")) for name in PAIRS + FAN3 + FAN4_VERTICAL + FAN4_HORIZONTAL + FAN5}
# class -> (its q2 ascending, its residuals: name -> taps {(dr, dc): weight} around the pixel)
CLASSES = {
    "S1": ((2, 4), {k: {(dr, dc): 1, (0, 0): -1} for k, (dr, dc) in DIRECTIONS.items()}),
    "S3": ((6, 9, 12), {k: {(-dr, -dc): 1, (0, 0): -3, (dr, dc): 3, (2 * dr, 2 * dc): -1} for k, (dr, dc) in DIRECTIONS.items()}),
}
# the 200 tables in order: (class, q2, set, scan)
TABLES = [(cls, q2, name, scan) for cls, (steps, _) in CLASSES.items() for q2 in steps for name in SETS for scan in "hv"]


def _stated(order):
    """the reach (up, down, left, right) of every set as the definition states it: a first-order residual reaches 1 along its direction; a
    third-order one 2 along it and 1 against it"""
    def side(members, axis, sign):
        along = [DIRECTIONS[m][axis] * sign for m in members]
        return max([0] + [(1 if order == 1 else 2) if a > 0 else (0 if order == 1 else 1) if a < 0 else 0 for a in along])
    return {name: (side(m, 0, -1), side(m, 0, 1), side(m, 1, -1), side(m, 1, 1)) for name, m in SETS.items()}


REACH = {"S1": _stated(1), "S3": _stated(3)}
assert REACH["S1"]["E+N"] == (1, 0, 0, 1) and REACH["S3"]["E+N"] == (2, 1, 1, 2) and REACH["S3"]["W+SW+S"] == (1, 2, 2, 1)
assert REACH["S1"]["E+NE+N+NW"] == (1, 0, 1, 1) and REACH["S3"]["SE+E+NE+N+NW"] == (2, 2, 2, 2) and REACH["S1"]["SW+S+SE+E+NE"] == (1, 1, 1, 1)
# the submodels of a (class, q2) in order: name -> the (set, scan) tables it sums
SUBMODELS = {
    "pair": tuple((s, scan) for s in PAIRS for scan in "hv"),
    "fan3": tuple((s, scan) for s in FAN3 for scan in "hv"),
    "fan4h": tuple((s, "h") for s in FAN4_VERTICAL) + tuple((s, "v") for s in FAN4_HORIZONTAL),
    "fan4v": tuple((s, "v") for s in FAN4_VERTICAL) + tuple((s, "h") for s in FAN4_HORIZONTAL),
    "fan5": tuple((s, scan) for s in FAN5 for scan in "hv"),
}
BINS, CENTRE, ORBITS, DIM = 625, 312, 325, 8125


def reach(cls, name):
    """(up, down, left, right) of the union of the taps of the set's members"""
    taps = [t for member in SETS[name] for t in CLASSES[cls][1][member]]
    return (-min(dr for dr, _ in taps), max(dr for dr, _ in taps), -min(dc for _, dc in taps), max(dc for _, dc in taps))


def ab(cls, name, scan):
    """the (a, b) of the table's total 2 max(h - a, 0) max(w - b, 0)"""
    u, dn, l, rt = REACH[cls][name]
    return (u + dn, l + rt + 3) if scan == "h" else (u + dn + 3, l + rt)


def totals(h, w):
    """the 200 totals of an h x w image"""
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


def counts(x_u8):
    """(N,200,625) int64 of (N,H,W) uint8 planes"""
    x = np.asarray(x_u8)
    assert x.dtype == np.uint8 and x.ndim == 3
    x = x.astype(np.int64)
    out, cache = [], {}
    for cls, q2, name, scan in TABLES:
        if (cls, name) not in cache:
            cache[cls, name] = members(x, cls, name)
        D = srm_np.digit(cache[cls, name], q2)
        lo, hi = np.minimum.reduce(D), np.maximum.reduce(D)
        out.append(srm_np.table(lo, scan) + srm_np.table(-hi, scan))
    return np.stack(out, axis=1)


def features(c):
    """(N,200,625) counts -> (N,8125) float64: per (class, q2) its five submodels, each the sum of its tables, folded to 325 orbits and
    divided by its own sum"""
    c = np.asarray(c).astype(np.int64)
    at = {t: i for i, t in enumerate(TABLES)}
    orb = mm_np.orbits()
    out = []
    for cls, (steps, _) in CLASSES.items():
        for q2 in steps:
            for tables in SUBMODELS.values():
                b = sum(c[:, at[cls, q2, name, scan]] for name, scan in tables)
                f = np.stack([b[:, o].sum(axis=1) for o in orb], axis=1)
                s = f.sum(axis=1, keepdims=True)
                if (s == 0).any():
                    raise ValueError("a submodel without a run")
                out.append(f.astype(np.float64) / s.astype(np.float64))
    return np.concatenate(out, axis=1)
