"""numpy-only restatement of the counts of the SRM EDGE classes (include/wsu.h K55) and of the features made from them
(ws_unet_amd/srm.py `features_edge`), written from the definition in srm_minmax_np's shape: four edge residuals per pixel and class
(the half of the 3x3 or 5x5 kernel on one side of its centre row or column), eleven sets of them, a table counts the runs of four lo
digits and, negated, of four hi digits; a singleton set has lo = hi.  Vectorised over the batch."""
import srm_minmax_np as mm_np
import srm_np
import srm_sets_np as sets_np


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


_RESIDUALS = {cls: residuals for cls, (_, residuals) in CLASSES.items()}
_SETS = {cls: SETS for cls in CLASSES}


def reach(cls, name):
    return sets_np.reach(_RESIDUALS, _SETS, cls, name)


def ab(cls, name, scan):
    return sets_np.ab(REACH, cls, name, scan)


def totals(h, w):
    """the 132 totals of an h x w image"""
    return sets_np.totals(REACH, TABLES, h, w)


def members(x, cls, name):
    return sets_np.members(_RESIDUALS, _SETS, x, cls, name)


def counts(x_u8, plain=False):
    """(N,132,625) int64 of (N,H,W) uint8 planes; plain=True: one update per run, the run of the lo digits alone"""
    return sets_np.counts(_RESIDUALS, _SETS, TABLES, x_u8, plain)


def features(c):
    """(N,132,625) counts -> (N,9828) float64: per (class, q2) its six submodels, each the sum of its tables, folded to 169 or 325 orbits
    and divided by its own sum"""
    orb = {169: srm_np.orbits(), 325: mm_np.orbits()}
    return sets_np.features(TABLES, {cls: steps for cls, (steps, _) in CLASSES.items()},
                            {cls: [(summed, orb[fold]) for summed, fold in SUBMODELS.values()] for cls in CLASSES}, c)
