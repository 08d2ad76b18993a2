"""numpy-only restatement of what the min/max count kernels of the SRM share (include/wsu.h K50, K54, K55), written from the definition:
every member residual of a set is a sum of shifted slices over the centres at which ALL the set's taps lie in the image, the set's digits
are np.minimum.reduce / np.maximum.reduce over its members' digits, a table counts the runs of four lo digits and, negated, of four hi
digits (srm_np.digit, srm_np.table).  Vectorised over the batch.  srm_minmax_np, srm_fans_np and srm_edge_np hold the data of their
classes and call this with it:
  residuals   class -> member -> taps {(dr, dc): weight} around the pixel
  sets        class -> set -> its members
  stated      class -> set -> the reach (up, down, left, right) as the definition states it
  tables      the tables in order, (class, q2, set, scan)"""
import numpy as np

import srm_np


def reach(residuals, sets, cls, name):
    """(up, down, left, right) of the union of the taps of the set's members"""
    taps = [t for member in sets[cls][name] for t in residuals[cls][member]]
    return (-min(dr for dr, _ in taps), max(dr for dr, _ in taps), -min(dc for _, dc in taps), max(dc for _, dc in taps))


def ab(stated, cls, name, scan):
    """the (a, b) of the table's total 2 max(h - a, 0) max(w - b, 0)"""
    u, dn, l, rt = stated[cls][name]
    return (u + dn, l + rt + 3) if scan == "h" else (u + dn + 3, l + rt)


def totals(stated, tables, h, w):
    """the tables' totals of an h x w image"""
    return [2 * max(h - a, 0) * max(w - b, 0) for cls, _, name, scan in tables for a, b in [ab(stated, cls, name, scan)]]


def members(residuals, sets, x, cls, name):
    """x (N,H,W) int64 -> the member residuals of the set at every pixel at which all the set's taps lie in the image, (M, N, H', W')"""
    n, h, w = x.shape
    u, dn, l, rt = reach(residuals, sets, cls, name)
    hh, ww = max(h - u - dn, 0), max(w - l - rt, 0)
    out = np.zeros((len(sets[cls][name]), n, hh, ww), dtype=np.int64)
    if hh and ww:
        for k, member in enumerate(sets[cls][name]):
            for (dr, dc), wt in residuals[cls][member].items():
                out[k] += wt * x[:, u + dr:u + dr + hh, l + dc:l + dc + ww]
    return out


def counts(residuals, sets, tables, x_u8, plain=False):
    """(N,len(tables),625) int64 of (N,H,W) uint8 planes.  plain=True: ONE update per run, the run of the lo digits alone (what a linear
    residual's table is; of a singleton set its min/max table is this one plus this one with every digit negated)"""
    x = np.asarray(x_u8)
    assert x.dtype == np.uint8 and x.ndim == 3
    x = x.astype(np.int64)
    out, cache = [], {}
    for cls, q2, name, scan in tables:
        if (cls, name) not in cache:
            cache[cls, name] = members(residuals, sets, x, cls, name)
        D = srm_np.digit(cache[cls, name], q2)
        lo, hi = np.minimum.reduce(D), np.maximum.reduce(D)
        out.append(srm_np.table(lo, scan) + (0 if plain else srm_np.table(-hi, scan)))
    return np.stack(out, axis=1)


def features(tables, steps, submodels, c):
    """(N,len(tables),625) counts -> (N,DIM) float64: per (class, q2) (steps: class -> its q2 ascending) its submodels (submodels: class
    -> a sequence of (the (set, scan) tables it sums, the orbits it is folded to)), each the sum of its tables, folded and divided by
    its own sum"""
    c = np.asarray(c).astype(np.int64)
    at = {t: i for i, t in enumerate(tables)}
    out = []
    for cls, q2s in steps.items():
        for q2 in q2s:
            for summed, orb in submodels[cls]:
                b = sum(c[:, at[cls, q2, name, scan]] for name, scan in summed)
                f = np.stack([b[:, o].sum(axis=1) for o in orb], axis=1)
                s = f.sum(axis=1, keepdims=True)
                if (s == 0).any():
                    raise ValueError("a submodel without a run")
                out.append(f.astype(np.float64) / s.astype(np.float64))
    return np.concatenate(out, axis=1)
