"""The FLD ensemble of ws_unet_amd.ensemble restated in numpy, step for step of that module's docstring and written without reading its
code paths: the Gram by einsum, the draws, scatter, solve, threshold (a brute force over every candidate), out-of-bag tally and vote."""
import numpy as np


def gram(zt, idx, weights, dtype=np.float64):
    """G[l, a, b] = sum_i weights[l, i] zt[idx[l, a], i] zt[idx[l, b], i] in `dtype` (int64: exact for integer data; longdouble: the
    reference of the real-valued test)"""
    zt, out = np.asarray(zt).astype(dtype), []
    for l in range(len(idx)):
        A = zt[np.asarray(idx[l])]
        out.append(np.einsum("i,ai,bi->ab", np.asarray(weights[l]).astype(dtype), A, A))
    return np.stack(out)


def gram_abs(zt, idx, weights):
    """sum_i w_i |z_a z_b| in longdouble: what the rounding bound of a product sum is taken of"""
    return gram(np.abs(np.asarray(zt, dtype=np.longdouble)), idx, weights, np.longdouble)


def groups(n0, n1, groups0=None, groups1=None):
    if groups0 is None:
        if n1 % n0 == 0:
            groups0, groups1 = np.arange(n0), np.tile(np.arange(n0), n1 // n0)
        else:
            groups0, groups1 = np.arange(n0), np.arange(n0, n0 + n1)
    labels = np.concatenate([groups0, groups1])
    order = sorted(set(int(v) for v in labels))
    return np.array([order.index(int(v)) for v in labels]), len(order)


def draws(seed, d, d_subs, learners, group, n_groups, n0):
    """[(idx (L, d_sub), c (L, n_groups)) per candidate], one Philox stream; a learner's whole draw is repeated while a class is empty"""
    rng = np.random.Generator(np.random.Philox(key=seed))
    out = []
    for ds in d_subs:
        idxs, cs = [], []
        while len(idxs) < learners:
            idx = sorted(rng.permutation(d)[:ds].tolist())
            c = np.bincount(rng.integers(0, n_groups, n_groups), minlength=n_groups)
            w = c[group]
            if w[:n0].sum() == 0 or w[n0:].sum() == 0:
                continue
            idxs.append(idx)
            cs.append(c)
        out.append((np.array(idxs), np.array(cs)))
    return out


def base_learner(Z, y, idx, w, ridge, dtype=np.float64):
    """w_l of one learner: Z (n, d) centred rows, y 0/1, idx (d_sub,), w (n,) row weights"""
    A = np.asarray(Z, dtype=dtype)[:, idx]
    w = np.asarray(w).astype(dtype)
    n0, n1 = w[y == 0].sum(), w[y == 1].sum()
    m0 = (w[y == 0, None] * A[y == 0]).sum(axis=0) / n0
    m1 = (w[y == 1, None] * A[y == 1]).sum(axis=0) / n1
    G = np.einsum("i,ia,ib->ab", w, A, A)
    S = (G - n0 * np.outer(m0, m0) - n1 * np.outer(m1, m1)) / (n0 + n1 - 2)
    lam = ridge * np.trace(S) / len(idx)
    M = S + lam * np.eye(len(idx), dtype=dtype)
    return np.linalg.solve(M.astype(np.float64), (m1 - m0).astype(np.float64)), M


def bag_error(p, y, w, b):
    """the weighted (P_FA + P_MD) / 2 of a bag at threshold b, as an exact fraction's numerator over the common denominator 2 n0 n1"""
    w = np.asarray(w).astype(np.int64)
    n0, n1 = int(w[y == 0].sum()), int(w[y == 1].sum())
    fa = int(w[(y == 0) & (p > b)].sum())
    md = int(w[(y == 1) & ~(p > b)].sum())
    return fa * n1 + md * n0


def threshold(p, y, w):
    """brute force: every midpoint of consecutive distinct projections of the bag, the lowest of the best"""
    inbag = np.asarray(w) > 0
    v = sorted(set(float(x) for x in p[inbag]))
    if len(v) == 1:
        return v[0]
    best, best_b = None, None
    for lo, hi in zip(v[:-1], v[1:]):
        b = (lo + hi) / 2.
        e = bag_error(p, y, w, b)
        if best is None or e < best:
            best, best_b = e, b
    return best_b


def oob_error(stego_votes, in_bag, y):
    tally = {0: [0., 0], 1: [0., 0]}
    for i in range(len(y)):
        judges = [l for l in range(stego_votes.shape[1]) if not in_bag[i, l]]
        if not judges:
            continue
        s = sum(bool(stego_votes[i, l]) for l in judges)
        if 2 * s == len(judges):
            e = 0.5
        else:
            e = float((2 * s > len(judges)) != bool(y[i]))
        tally[int(y[i])][0] += e
        tally[int(y[i])][1] += 1
    rate = [tally[c][0] / tally[c][1] if tally[c][1] else 0.5 for c in (0, 1)]
    return (rate[0] + rate[1]) / 2.


def votes(F, mean, idx, w, b):
    Z = np.asarray(F, dtype=np.float64) - mean
    return np.array([sum(bool(Z[i, idx[l]] @ w[l] > b[l]) for l in range(len(idx))) for i in range(len(Z))])


def fit(X0, X1, learners, d_subs, ridge, seed, groups0=None, groups1=None):
    """the whole fit: dict(idx, w, b, mean, d_sub, oob_error, oob_errors)"""
    X = np.concatenate([X0, X1]).astype(np.float64)
    n0 = len(X0)
    y = np.concatenate([np.zeros(n0, dtype=int), np.ones(len(X1), dtype=int)])
    mean = X.mean(axis=0)
    Z = X - mean
    group, n_groups = groups(n0, len(X1), groups0, groups1)
    best, errs = None, []
    for ds, (idx, c) in zip(d_subs, draws(seed, X.shape[1], d_subs, learners, group, n_groups, n0)):
        wt = c[:, group]
        w = np.stack([base_learner(Z, y, idx[l], wt[l], ridge)[0] for l in range(learners)])
        P = np.stack([Z[:, idx[l]] @ w[l] for l in range(learners)], axis=1)
        b = np.array([threshold(P[:, l], y, wt[l]) for l in range(learners)])
        e = oob_error(P > b[None, :], wt.T > 0, y)
        errs.append(e)
        if best is None or e < best["oob_error"]:
            best = dict(idx=idx, w=w, b=b, mean=mean, d_sub=ds, oob_error=e)
    best["oob_errors"] = errs
    return best
