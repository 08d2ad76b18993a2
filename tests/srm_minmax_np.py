"""numpy-only restatement of the counts of the SRM min/max submodels (include/wsu.h K50) and of the features made from them
(ws_unet_amd/srm.py `features_minmax`): the data of its three classes; srm_sets_np has the arithmetic, written from the definition."""
import itertools

import srm_sets_np as sets_np

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


_RESIDUALS = {cls: residuals for cls, (_, residuals, _) in CLASSES.items()}
_SETS = {cls: sets for cls, (_, _, sets) in CLASSES.items()}


def reach(cls, name):
    return sets_np.reach(_RESIDUALS, _SETS, cls, name)


def ab(cls, name, scan):
    return sets_np.ab(REACH, cls, name, scan)


def totals(h, w):
    """the 118 totals of an h x w image"""
    return sets_np.totals(REACH, TABLES, h, w)


def members(x, cls, name):
    return sets_np.members(_RESIDUALS, _SETS, x, cls, name)


def counts(x_u8):
    """(N,118,625) int64 of (N,H,W) uint8 planes"""
    return sets_np.counts(_RESIDUALS, _SETS, TABLES, x_u8)


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
    orb = orbits()
    return sets_np.features(TABLES, {cls: steps for cls, (steps, _, _) in CLASSES.items()},
                            {cls: [(summed, orb) for summed in SUBMODELS[cls].values()] for cls in CLASSES}, c)
