"""numpy-only restatement of the counts of the SRM fan submodels (include/wsu.h K54) and of the features made from them
(ws_unet_amd/srm.py `features_fans`), written from the definition in srm_minmax_np's shape: eight directional residuals per pixel and
class, a set is a perpendicular pair or a run of adjacent directions, its digits are the minimum and the maximum over its members'
digits, a table counts the runs of four lo digits and, negated, of four hi digits.  Vectorised over the batch."""
import srm_minmax_np as mm_np
import srm_sets_np as sets_np

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


_RESIDUALS = {cls: residuals for cls, (_, residuals) in CLASSES.items()}
_SETS = {cls: SETS for cls in CLASSES}


def reach(cls, name):
    return sets_np.reach(_RESIDUALS, _SETS, cls, name)


def ab(cls, name, scan):
    return sets_np.ab(REACH, cls, name, scan)


def totals(h, w):
    """the 200 totals of an h x w image"""
    return sets_np.totals(REACH, TABLES, h, w)


def members(x, cls, name):
    return sets_np.members(_RESIDUALS, _SETS, x, cls, name)


def counts(x_u8):
    """(N,200,625) int64 of (N,H,W) uint8 planes"""
    return sets_np.counts(_RESIDUALS, _SETS, TABLES, x_u8)


def features(c):
    """(N,200,625) counts -> (N,8125) float64: per (class, q2) its five submodels, each the sum of its tables, folded to 325 orbits and
    divided by its own sum"""
    orb = mm_np.orbits()
    return sets_np.features(TABLES, {cls: steps for cls, (steps, _) in CLASSES.items()},
                            {cls: [(summed, orb) for summed in SUBMODELS.values()] for cls in CLASSES}, c)
