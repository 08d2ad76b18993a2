"""numpy-only restatement of the HILL cost and the wMAE of src/filters/evaluate.py:79-115 (the definition that reproduces the
published results/prediction/filters.csv): x padded once by 9 with numpy.pad(mode='symmetric'), three 'valid' box / high-pass
convolutions in float64, the reference's 1e10 clamp, numpy.quantile and a masked mean."""
import numpy as np

HPF = np.array([[-1, 2, -1], [2, -4, 2], [-1, 2, -1]], dtype=np.float64)


def _valid(x, k):
    kh, kw = k.shape
    h, w = x.shape[0] - kh + 1, x.shape[1] - kw + 1
    out = np.zeros((h, w))
    for a in range(kh):
        for b in range(kw):
            if k[a, b] != 0:
                out += k[a, b] * x[a:a + h, b:b + w]
    return out


def _box(x, m):
    c = np.cumsum(np.cumsum(np.pad(x, ((1, 0), (1, 0))), 0), 1)     # exact for the integer sums S (|R| is integral)
    return c[m:, m:] - c[:-m, m:] - c[m:, :-m] + c[:-m, :-m]


def hill_cost(x_u8, clamp=1e10):
    x = np.pad(np.asarray(x_u8, dtype=np.float64), 9, mode="symmetric")
    s = _box(np.abs(_valid(x, HPF)), 3)                              # integers: exact
    with np.errstate(divide="ignore"):
        rho = 1.0 / (s / 9.0)
    # 15x15 direct sums (inf must not meet a subtraction): separable, row pass then column pass
    hs = sum(rho[:, b:b + rho.shape[1] - 14] for b in range(15))
    cost = sum(hs[a:a + hs.shape[0] - 14] for a in range(15)) / 225.0
    cost[np.isinf(cost) | np.isnan(cost) | (cost > clamp)] = clamp
    return cost


def filter_hat(x_u8, taps8):
    """x @ filter of the reference's get_processor features (neighbour order x00 x01 x02 x12 x22 x21 x20 x10), float64."""
    x = np.asarray(x_u8, dtype=np.float64)
    f = np.asarray(taps8, dtype=np.float64).reshape(8)
    nb = [x[:-2, :-2], x[:-2, 1:-1], x[:-2, 2:], x[1:-1, 2:], x[2:, 2:], x[2:, 1:-1], x[2:, :-2], x[1:-1, :-2]]
    return sum(f[i] * nb[i] for i in range(8))


def wmae(abs_resid, cost_interior, quantile=0.1):
    """(wmae, q, selected count) of |resid| over cost <= numpy.quantile(cost, quantile)."""
    q = np.quantile(cost_interior, quantile)
    sel = cost_interior <= q
    return float(np.mean(abs_resid[sel])), float(q), int(sel.sum())
