"""numpy-only restatement of the 5x5 least-squares predictor: the exact moments (K56), the prediction and bias planes in K57's float32
operation order (ws_unet_amd/csrc/ols5.hip), KB embedded in the 24 taps and the 24x5 indicator matrix of the symmetric fit."""
import numpy as np

OFFSETS = [(a, b) for a in range(5) for b in range(5) if (a, b) != (2, 2)]          # v[0..23]: the 5x5 raster without its centre
IU = np.triu_indices(25)
KB3 = np.array([[-1, 2, -1], [2, 0, 2], [-1, 2, -1]], dtype=np.float32) / np.float32(4.)


def design(x_u8):
    """(H,W) uint8 -> int64 (P,25): per pixel with a full 5x5 window the 24 neighbours in raster order, then the centre."""
    x = np.asarray(x_u8).astype(np.int64)
    h, w = x.shape
    cols = [x[a:a + h - 4, b:b + w - 4] for a, b in OFFSETS] + [x[2:-2, 2:-2]]
    return np.stack([c.reshape(-1) for c in cols], axis=1)


def moments(x_u8):
    """(H,W) uint8 -> (325,) int64, or (N,H,W) -> (N,325): the upper triangle of V^T V, row-major, exact integers."""
    x = np.asarray(x_u8)
    if x.ndim == 3:
        return np.stack([moments(p) for p in x])
    v = design(x)
    if len(v) * 255 * 255 < 2 ** 53:                            # every partial sum is an integer below 2^53: the float64 product is exact
        f = v.astype(np.float64)
        return (f.T @ f).astype(np.int64)[IU]
    return (v.T @ v)[IU]


def kb_taps():
    """KB's 3x3 weights on the inner ring of the 5x5 window, zeros on the outer one -> (24,) float64"""
    full = np.zeros((5, 5))
    full[1:4, 1:4] = KB3
    return np.delete(full.reshape(25), 12)


def symmetric_matrix():
    """S (24,5): tap k belongs to the class of its unordered (|dr|,|dc|), in the order (0,1) (1,1) (0,2) (1,2) (2,2)"""
    classes = [(0, 1), (1, 1), (0, 2), (1, 2), (2, 2)]
    S = np.zeros((24, 5))
    for k, (a, b) in enumerate(OFFSETS):
        S[k, classes.index(tuple(sorted((abs(a - 2), abs(b - 2)))))] = 1.
    return S


def _planes(x):
    """q(u) = (float32)u / 255.f and qb(u) = (u & 1) ? -q(1) : q(1) of a uint8 plane"""
    q = x.astype(np.float32) / np.float32(255.)
    q1 = np.float32(1.) / np.float32(255.)
    return q, np.where(x & 1, -q1, q1).astype(np.float32)


def _predict_one(x, taps32):
    h, w = x.shape
    hat, bias = np.zeros((h, w), dtype=np.float32), np.zeros((h, w), dtype=np.float32)
    for src, out in zip(_planes(x), (hat, bias)):
        # ring 1 and everything inside it: KB, acc = acc + kb[j] * q[j] for j = 8 .. 0 (the centre's tap of 0 takes part, as in K11)
        acc = np.zeros((h - 2, w - 2), dtype=np.float32)
        for j in range(8, -1, -1):
            acc = acc + KB3[j // 3, j % 3] * src[j // 3:j // 3 + h - 2, j % 3:j % 3 + w - 2]
        out[1:-1, 1:-1] = acc * np.float32(255.)
        if h >= 5 and w >= 5:                                   # the pixels with a full 5x5 window: the 24 taps, k = 23 .. 0
            acc = np.zeros((h - 4, w - 4), dtype=np.float32)
            for k in range(23, -1, -1):
                a, b = OFFSETS[k]
                acc = acc + taps32[k] * src[a:a + h - 4, b:b + w - 4]
            out[2:-2, 2:-2] = acc * np.float32(255.)
        assert acc.dtype == np.float32
    return hat, bias


def predict(x_u8, taps32):
    """(N,H,W) uint8, float32 taps (24,) or (N,24) -> (x_hat, x_bias) float32 (N,H,W): K57's planes, every operation rounded to float32."""
    x = np.asarray(x_u8)
    t = np.asarray(taps32)
    assert x.ndim == 3 and x.dtype == np.uint8 and t.dtype == np.float32 and t.shape in ((24,), (len(x), 24))
    res = [_predict_one(p, t if t.ndim == 1 else t[i]) for i, p in enumerate(x)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
