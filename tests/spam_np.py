"""numpy-only restatement of the SPAM counts (include/wsu.h K36), of the features made from them and of the ridge-regularised Fisher
discriminant (ws_unet_amd/spam.py; Pevny, Bas, Fridrich 2010), written from the definitions: all eight directions are counted by brute
force over shifted slices, one image at a time."""
import numpy as np

STEPS = ((0, 1), (1, 0), (1, 1), (1, -1))                                   # K36's four: right, down, down-right, down-left
STEPS8 = STEPS + tuple((-dr, -dc) for dr, dc in STEPS)                      # ... and their opposites: left, up, up-left, up-right


def bins(order, T):
    return (2 * T + 1) ** (order + 1)


def counts_step(p, dr, dc, order, T):
    """(B^(order+1),) int64 of one (H,W) plane along the step (dr, dc)."""
    h, w = p.shape
    B, k = 2 * T + 1, order + 1
    x = p.astype(np.int64)
    r_lo, r_hi = max(0, -k * dr), h - max(0, k * dr)                         # the positions whose whole run is in the image
    c_lo, c_hi = max(0, -k * dc), w - max(0, k * dc)
    if r_hi <= r_lo or c_hi <= c_lo:
        return np.zeros(bins(order, T), dtype=np.int64)
    at = lambda j: x[r_lo + j * dr:r_hi + j * dr, c_lo + j * dc:c_hi + j * dc]
    idx = np.zeros((r_hi - r_lo, c_hi - c_lo), dtype=np.int64)
    for j in range(order + 1):
        idx = idx * B + np.clip(at(j) - at(j + 1), -T, T) + T
    return np.bincount(idx.ravel(), minlength=bins(order, T)).astype(np.int64)


def counts(x_u8, order=2, T=3, steps=STEPS):
    """(N, len(steps), B^(order+1)) int64 of (N,H,W) planes."""
    x = np.asarray(x_u8)
    assert x.dtype == np.uint8 and x.ndim == 3
    return np.stack([np.stack([counts_step(p, dr, dc, order, T) for dr, dc in steps]) for p in x])


def opposite(c, order=2, T=3):
    """C_opp[d_0, .., d_order] = C[-d_order, .., -d_0] on the last axis, bin by bin."""
    B, k = 2 * T + 1, order + 1
    c = np.asarray(c)
    out = np.empty_like(c)
    for b in range(bins(order, T)):
        digits = [(b // B ** (k - 1 - j)) % B for j in range(k)]             # d_j + T, d_0 first
        src = sum((2 * T - dg) * B ** (k - 1 - j) for j, dg in enumerate(reversed(digits)))
        out[..., b] = c[..., src]
    return out


def features(c, order=2, T=3, normalise="joint"):
    """(N,4,bins) counts -> (N, 2 bins) float64."""
    B, nb = 2 * T + 1, bins(order, T)
    c = np.asarray(c)
    tables = np.concatenate([c, opposite(c, order, T)], axis=1).astype(np.float64)
    totals = tables.sum(axis=2, keepdims=True)
    if (totals == 0).any():
        raise ValueError("a direction without a run")
    if normalise == "joint":
        p = tables / totals
    else:
        rows = tables.reshape(len(c), 8, nb // B, B)
        den = rows.sum(axis=3, keepdims=True)
        p = np.divide(rows, den, out=np.zeros_like(rows), where=den != 0).reshape(tables.shape)
    axis = (p[:, 0] + p[:, 4] + p[:, 1] + p[:, 5]) / 4.
    diag = (p[:, 2] + p[:, 6] + p[:, 3] + p[:, 7]) / 4.
    return np.concatenate([axis, diag], axis=1)


def fld_fit(X0, X1, ridge=0.1):
    """(w, b): w = (S + lambda I)^-1 (mu1 - mu0), S the pooled within-class covariance, lambda = ridge trace(S) / d, b = w.(mu0 + mu1) / 2."""
    X0, X1 = np.asarray(X0, dtype=np.float64), np.asarray(X1, dtype=np.float64)
    d = X0.shape[1]
    mu0, mu1 = X0.mean(axis=0), X1.mean(axis=0)
    A0, A1 = X0 - mu0, X1 - mu1
    S = (A0.T @ A0 + A1.T @ A1) / (len(X0) + len(X1) - 2)
    w = np.linalg.solve(S + ridge * np.trace(S) / d * np.eye(d), mu1 - mu0)
    return w, float(w @ (mu0 + mu1) / 2.)


def fld_output(F, w, b):
    return 1. / (1. + np.exp(-(np.asarray(F, dtype=np.float64) @ w - b)))


def auc(neg, pos):
    """P(score of a positive > score of a negative) + half the ties: the area under the ROC."""
    neg, pos = np.asarray(neg, dtype=np.float64)[:, None], np.asarray(pos, dtype=np.float64)[None, :]
    return float(((pos > neg).sum() + 0.5 * (pos == neg).sum()) / (neg.shape[0] * pos.shape[1]))
