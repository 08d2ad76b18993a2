"""numpy-only restatement of the predictor / stego-change correlation of src/correlation.py:22-59, in float64:

    d     = (x_s - x_c)[1:-1, 1:-1]                  xhat = predictor(x_s)              dhat = xhat - x_c[1:-1, 1:-1]
    cor   = (sum((dhat - mean dhat) * (d - mean d)) / (n - 1)) / std(xhat) / std(d)     (std: ddof 0; NB std of xhat, not dhat)

Division by zero follows IEEE (numpy with warnings silenced): x_s == x_c gives NaN, a constant prediction +-inf (NaN if the
covariance is 0 as well)."""
import numpy as np


def filter_hat(x_u8, kernel):
    """scipy.signal.convolve(x, K[..., ::-1], 'valid') of a (3,3[,1]) kernel array, in float64: sum_ab K[a][b] x[r+1-a][c+1-b]."""
    k = np.asarray(kernel, dtype=np.float64)
    k = k[..., 0] if k.ndim == 3 else k
    x = np.asarray(x_u8, dtype=np.float64)
    h, w = x.shape[0] - 2, x.shape[1] - 2
    out = np.zeros((h, w))
    for a in range(3):
        for b in range(3):
            out += k[a, b] * x[2 - a:2 - a + h, 2 - b:2 - b + w]
    return out


def correlation(x_c, x_s, xhat):
    """x_c, x_s: (H,W) uint8; xhat: (H-2,W-2) prediction in grey levels (any float dtype, used in float64)."""
    xc = np.asarray(x_c, dtype=np.float64)[1:-1, 1:-1]
    d = np.asarray(x_s, dtype=np.float64)[1:-1, 1:-1] - xc
    xhat = np.asarray(xhat, dtype=np.float64).reshape(d.shape)
    dhat = xhat - xc
    with np.errstate(divide="ignore", invalid="ignore"):
        cov = np.sum((dhat - dhat.mean()) * (d - d.mean())) / (d.size - 1)
        return float(np.float64(cov) / xhat.std() / d.std())


def p_value(cor, n):
    """scipy.stats.t.sf(|cor| / sqrt(1 - cor^2) * sqrt(n - 2), n - 2), with scipy (test side only)."""
    from scipy import stats
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.abs(np.float64(cor)) / np.sqrt(1 - np.float64(cor) ** 2) * np.sqrt(n - 2)
    return float(stats.t.sf(t, n - 2))
