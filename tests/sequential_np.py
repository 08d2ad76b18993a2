"""numpy-only restatements of the sequential-payload WS changepoint (include/wsu.h K27, ws_unet_amd/ws/sequential.py) and of the sequential
simulator LSBRS (K28).

ws_terms: the per-pixel float32 terms t = wgt * (s * res - 1/4) of one plane in K11's operation sequence (every product and sum a separate
float32 rounding, the nine taps of a true convolution added K00 .. K22 from 0), quantised to the fixed-point integers
q = 0 where t is NaN, else rint(clip(t, -4096, 4096) * 2^24).  changepoint: the first maximiser of the cumulative sums along the path.
lsbrs_np: Philox4x32-10 of embed_np; a pixel flips iff its path position is below m and its word is below 2^31."""
import numpy as np

import embed_np

ORDERS = ("rows", "rows_up")


def _conv9(kern, planes):
    """true convolution, 'valid', summed in the order K00 .. K22: out(r,c) = sum_{a,b} K[a][b] * v(r+1-a, c+1-b); planes[i][j] = v(r-1+i, c-1+j)"""
    kern = np.asarray(kern, dtype=np.float32).reshape(3, 3)
    acc = np.zeros_like(planes[0][0])
    for a in range(3):
        for b in range(3):
            acc = acc + kern[a, b] * planes[2 - a][2 - b]
    return acc


def ws_terms(x, x_hat=None, hat_scale=255., pixel_kernel=None, mean_kernel=None, weighted=1):
    """x: (H,W) uint8.  x_hat: (H,W) full frame or (H-2,W-2) interior, float32, multiplied by hat_scale; or pixel_kernel (3,3) K[a][b].
    -> q (H-2,W-2) int64."""
    x = np.asarray(x, dtype=np.uint8)
    h, w = x.shape
    v = [[x[i:h - 2 + i, j:w - 2 + j].astype(np.float32) for j in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        wgt = np.float32(1.0)
        if weighted:
            v2 = [[p * p for p in row] for row in v]
            mu, mu2 = _conv9(mean_kernel, v), _conv9(mean_kernel, v2)
            var = mu2 - mu * mu
            wgt = np.float32(1.0) / (np.float32(5.0) + var)
        xc = v[1][1]
        s = xc - (x[1:-1, 1:-1] ^ 1).astype(np.float32)
        if pixel_kernel is not None:
            unit = [[p / np.float32(255.0) for p in row] for row in v]
            hat = _conv9(pixel_kernel, unit) * np.float32(255.0)
        else:
            y = np.asarray(x_hat, dtype=np.float32)
            y = y[1:-1, 1:-1] if y.shape == (h, w) else y
            assert y.shape == (h - 2, w - 2), y.shape
            hat = y * np.float32(hat_scale)
        res = xc - hat
        r = s * res
        d = r - np.float32(0.25)
        t = (wgt * d).astype(np.float32)
        q = np.rint(np.clip(t, np.float32(-4096.0), np.float32(4096.0)).astype(np.float64) * 2.0 ** 24)
    return np.where(np.isnan(t), 0.0, q).astype(np.int64)


def changepoint(q, order="rows"):
    """q: (H-2,W-2) int64 terms -> (k, t_max, t_all, curve (H-2,)): the smallest k in 0..M with T(k) maximal, T(0) = 0 included."""
    assert order in ORDERS
    q = np.asarray(q, dtype=np.int64)
    path = (q if order == "rows" else q[::-1]).reshape(-1)
    T = np.concatenate([[0], np.cumsum(path, dtype=np.int64)])
    k = int(np.argmax(T))                                     # argmax: the first of equal maxima
    curve = T[q.shape[1]::q.shape[1]].copy()
    return k, int(T[k]), int(T[-1]), curve


def ws_sequential_np(x, order="rows", **kw):
    return changepoint(ws_terms(x, **kw), order)


def payload(k, h, w, order="rows"):
    """k -> p_hat: the 1-based position, on the path over the whole plane, of the k-th interior pixel of the path, over H W (0 for k = 0)."""
    assert order in ORDERS
    if k == 0:
        return 0.0
    p, c = divmod(k - 1, w - 2)                               # interior path row, interior column
    r = p + 1 if order == "rows" else h - 2 - p               # plane row
    pos = (r * w if order == "rows" else (h - 1 - r) * w) + (c + 1) + 1
    return pos / (h * w)


def lsbrs_count(alpha, h, w):
    return int(np.floor(np.float64(alpha) * np.float64(h * w)))


def path_positions(h, w, order="rows"):
    """(H,W) int64: every pixel's 0-based position on the path over the whole plane"""
    assert order in ORDERS
    pos = np.arange(h * w, dtype=np.int64).reshape(h, w)
    return pos if order == "rows" else pos[::-1].copy()


def lsbrs_np(cover, alpha, seed, order="rows", count=None):
    """(H,W) uint8 -> the LSBRS twin: the LSBR twin at alpha = 1 on the first m = floor(alpha H W) path positions (or `count` of them), the
    cover elsewhere."""
    cover = np.asarray(cover, dtype=np.uint8)
    full = embed_np.lsbr_np(cover, 1.0, seed)
    used = path_positions(*cover.shape, order) < (lsbrs_count(alpha, *cover.shape) if count is None else count)
    return np.where(used, full, cover)
