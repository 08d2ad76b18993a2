"""numpy-only restatement of the least-squares predictor's moments (K24), of the float64 solve, and of the WS statistic with an
in-kernel 3x3 filter in the kernel's float32 operation order (ws_unet_amd/csrc/ws_attack.hip)."""
import numpy as np

RING = ((0, 0), (0, 1), (0, 2), (1, 2), (2, 2), (2, 1), (2, 0), (1, 0))          # x00 x01 x02 x12 x22 x21 x20 x10
IU = np.triu_indices(9)


def design(x_u8):
    """(H,W) uint8 -> int64 (P,9): per interior pixel the eight neighbours in ring order, then the centre."""
    x = np.asarray(x_u8).astype(np.int64)
    h, w = x.shape
    cols = [x[a:a + h - 2, b:b + w - 2] for a, b in RING] + [x[1:-1, 1:-1]]
    return np.stack([c.reshape(-1) for c in cols], axis=1)


def moments(x_u8):
    """(H,W) uint8 -> (45,) int64, or (N,H,W) -> (N,45): the upper triangle of V^T V, row-major, exact integers."""
    x = np.asarray(x_u8)
    if x.ndim == 3:
        return np.stack([moments(p) for p in x])
    v = design(x)
    return (v.T @ v)[IU]


def normal_equations(m):
    full = np.zeros((9, 9))
    full[IU] = np.asarray(m, dtype=np.float64)
    full = full + np.triu(full, 1).T
    return full[:8, :8], full[:8, 8], full[8, 8]


def solve(m):
    A, b, _ = normal_equations(m)
    return np.linalg.solve(A, b)


def _conv9_reverse(wgt, planes):
    """acc = 0; acc = acc + wgt[a][b] * v[a][b] from (2,2) down to (0,0), every operation rounded to float32 (scipy's K00 .. K22)."""
    acc = np.zeros_like(planes[0][0])
    for j in range(8, -1, -1):
        acc = acc + wgt[j // 3, j % 3] * planes[j // 3][j % 3]
    return acc


def ws_beta(x_u8, taps8, weighted=0):
    """beta_hat (float32) of the WS statistic without bias correction for a filter of 8 float64 taps in ring order, mean filter AVG."""
    x = np.asarray(x_u8)
    h, w = x.shape
    wgt = np.zeros((3, 3), dtype=np.float32)
    for t, (a, b) in zip(np.asarray(taps8, dtype=np.float64).reshape(8), RING):
        wgt[a, b] = np.float32(t)
    v = [[x[a:a + h - 2, b:b + w - 2].astype(np.float32) for b in range(3)] for a in range(3)]
    q = [[v[a][b] / np.float32(255.) for b in range(3)] for a in range(3)]
    xc = v[1][1]
    xhat = _conv9_reverse(wgt, q) * np.float32(255.)
    res = xc - xhat
    s = xc - (x[1:-1, 1:-1] ^ 1).astype(np.float32)
    if weighted:
        avg = np.full((3, 3), 1 / 8., dtype=np.float32)
        avg[1, 1] = 0
        mu = _conv9_reverse(avg, v)
        mu2 = _conv9_reverse(avg, [[p * p for p in row] for row in v])
        t = np.float32(5.) + (mu2 - mu * mu)
        wt = np.float32(1.) / t if weighted > 0 else t
    else:
        wt = np.ones_like(xc)
    ws = wt * s
    assert ws.dtype == np.float32 and res.dtype == np.float32
    beta = (ws * res).astype(np.float64).sum() / wt.astype(np.float64).sum()
    return np.float32(max(beta, 0.0))
