"""numpy-only restatement of the counts of the SRM min/max submodels (include/wsu.h K50) and of the features made from them
(ws_unet_amd/srm.py `features_minmax`), written from the definition: every member residual of a set is a sum of shifted slices over the
centres at which ALL the set's taps lie in the image, the set's digits are np.minimum.reduce / np.maximum.reduce over its members'
digits, a table counts the runs of four lo digits and, negated, of four hi digits (srm_np.digit, srm_np.table).  Vectorised over the
batch."""
import itertools

import numpy as np

import srm_np

# class -> (its q2 ascending, its residuals: name -> taps {(dr, dc): weight} around the pixel, its sets in order: name -> members)
_S13 = {"WE": "WE", "NS": "NS", "WENS": "WENS", "WNE": "WNE", "ESW": "ESW", "SWN": "SWN", "NES": "NES"}
CLASSES = {
    "S1": ((2, 4), {"E": {(0, 1): 1, (0, 0): -1}, "W": {(0, -1): 1, (0, 0): -1}, "S": {(1, 0): 1, (0, 0): -1}, "N": {(-1, 0): 1, (0, 0): -1}}, _S13),
    "S2": ((4, 6, 8), {"h": {(0, -1): 1, (0, 0): -2, (0, 1): 1}, "v": {(-1, 0): 1, (0, 0): -2, (1, 0): 1},
                       "d": {(-1, -1): 1, (0, 0): -2, (1, 1): 1}, "m": {(-1, 1): 1, (0, 0): -2, (1, -1): 1}},
           {"hv": "hv", "hvdm": "hvdm", "hvd": "hvd", "hvm": "hvm", "hd": "hd", "hm": "hm", "vd": "vd", "vm": "vm"}),
    "S3": ((6, 9, 12), {"E": {(0, -1): 1, (0, 0): -3, (0, 1): 3, (0, 2): -1}, "W": {(0, 1): 1, (0, 0): -3, (0, -1): 3, (0, -2): -1},
                        "S": {(-1, 0): 1, (0, 0): -3, (1, 0): 3, (2, 0): -1}, "N": {(1, 0): 1, (0, 0): -3, (-1, 0): 3, (-2, 0): -1}}, _S13),
}
# the 118 tables in order: (class, q2, set, scan)
TABLES = [(cls, q2, name, scan) for cls, (steps, _, sets) in CLASSES.items() for q2 in steps for name in sets for scan in "hv"]
# the reach (up, down, left, right) of every set as the definition states it (not derived from the taps: reach() below is, and the
# host test compares the two)
REACH = {"S1": {"WE": (0, 0, 1, 1), "NS": (1, 1, 0, 0), "WENS": (1, 1, 1, 1), "WNE": (1, 0, 1, 1), "ESW": (0, 1, 1, 1), "SWN": (1, 1, 1, 0),
                "NES": (1, 1, 0, 1)},
         "S2": {name: (1, 1, 1, 1) for name in CLASSES["S2"][2]},
         "S3": {"WE": (0, 0, 2, 2), "NS": (2, 2, 0, 0), "WENS": (2, 2, 2, 2), "WNE": (2, 1, 2, 2), "ESW": (1, 2, 2, 2), "SWN": (2, 2, 2, 1),
                "NES": (2, 2, 1, 2)}}
# the submodels of a (class, q2) in order: name -> the (set, scan) tables it sums
SUBMODELS = {
    "S1": {"22h": (("WE", "h"), ("NS", "v")), "22v": (("WE", "v"), ("NS", "h")), "24": (("WENS", "h"), ("WENS", "v")),
           "34h": (("WNE", "h"), ("ESW", "h"), ("SWN", "v"), ("NES", "v")), "34v": (("WNE", "v"), ("ESW", "v"), ("SWN", "h"), ("NES", "h"))},
    "S2": {"21": (("hv", "h"), ("hv", "v")), "41": (("hvdm", "h"), ("hvdm", "v")), "32": (("hvd", "h"), ("hvd", "v"), ("hvm", "h"), ("hvm", "v")),
           "24h": (("hd", "h"), ("hm", "h"), ("vd", "v"), ("vm", "v")), "24v": (("hd", "v"), ("hm", "v"), ("vd", "h"), ("vm", "h"))},
}
SUBMODELS["S3"] = SUBMODELS["S1"]
BINS, CENTRE, ORBITS, DIM = 625, 312, 325, 13000


def reach(cls, name):
    """(up, down, left, right) of the union of the taps of the set's members"""
    taps = [t for member in CLASSES[cls][2][name] for t in CLASSES[cls][1][member]]
    return (-min(dr for dr, _ in taps), max(dr for dr, _ in taps), -min(dc for _, dc in taps), max(dc for _, dc in taps))


def ab(cls, name, scan):
    """the (a, b) of the table's total 2 max(h - a, 0) max(w - b, 0)"""
    u, dn, l, rt = REACH[cls][name]
    return (u + dn, l + rt + 3) if scan == "h" else (u + dn + 3, l + rt)


def totals(h, w):
    """the 118 totals of an h x w image"""
    return [2 * max(h - a, 0) * max(w - b, 0) for cls, _, name, scan in TABLES for a, b in [ab(cls, name, scan)]]


def members(x, cls, name):
    """x (N,H,W) int64 -> the member residuals of the set at every pixel at which all the set's taps lie in the image, (M, N, H', W')"""
    n, h, w = x.shape
    u, dn, l, rt = reach(cls, name)
    hh, ww = max(h - u - dn, 0), max(w - l - rt, 0)
    out = np.zeros((len(CLASSES[cls][2][name]), n, hh, ww), dtype=np.int64)
    if hh and ww:
        for k, member in enumerate(CLASSES[cls][2][name]):
            for (dr, dc), wt in CLASSES[cls][1][member].items():
                out[k] += wt * x[:, u + dr:u + dr + hh, l + dc:l + dc + ww]
    return out


def counts(x_u8):
    """(N,118,625) int64 of (N,H,W) uint8 planes"""
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


def orbits():
    """The orbits of the digit tuples under (d0..d3) -> (d3..d0) alone, by enumeration: a list of lists of bins, the orbits in the order of
    their lexicographically smallest tuple."""
    seen, out = {}, []
    for t in itertools.product(range(-2, 3), repeat=4):                     # lexicographic
        if t in seen:
            continue
        group = sorted({t, t[::-1]})
        assert group[0] == t
        for m in group:
            seen[m] = len(out)
        out.append([sum((d + 2) * 5 ** (3 - k) for k, d in enumerate(m)) for m in group])
    return out


def features(c):
    """(N,118,625) counts -> (N,13000) float64: per (class, q2) its five submodels, each the sum of its tables, folded to 325 orbits and
    divided by its own sum"""
    c = np.asarray(c).astype(np.int64)
    at = {t: i for i, t in enumerate(TABLES)}
    orb = orbits()
    out = []
    for cls, (steps, _, _) in CLASSES.items():
        for q2 in steps:
            for tables in SUBMODELS[cls].values():
                b = sum(c[:, at[cls, q2, name, scan]] for name, scan in tables)
                f = np.stack([b[:, o].sum(axis=1) for o in orb], axis=1)
                s = f.sum(axis=1, keepdims=True)
                if (s == 0).any():
                    raise ValueError("a submodel without a run")
                out.append(f.astype(np.float64) / s.astype(np.float64))
    return np.concatenate(out, axis=1)
