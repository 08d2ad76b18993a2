"""numpy-only restatements of the WS changepoint along a cost order (include/wsu.h K33, ws_unet_amd/ws/adaptive.py) and of the HILLRM
simulator (K34).

ordered_terms: sequential_np.ws_terms with tau = (float32)(flip_rate / 2) in place of 1/4: the per-pixel float32 terms
t = wgt * (s * res - tau) in K11's operation sequence, quantised to q = 0 where t is NaN, else rint(clip(t, -4096, 4096) * 2^24).
changepoint_along: the first maximiser of the cumulative sums of q along a path of interior raster indices; an index outside 0..M-1
adds nothing.  interior_order_np: the stable ascending argsort of a key plane's interior.  hillrm_np: the pixels whose float64 HILL cost
is at most the order statistic of rank floor((H W - 1) alpha) flip as under LSBR at alpha = 1."""
import numpy as np

import embed_np
import hill_np
from sequential_np import _conv9


def tau_of(flip_rate):
    return np.float32(float(flip_rate) / 2.0)


def ordered_terms(x, x_hat=None, hat_scale=255., pixel_kernel=None, mean_kernel=None, weighted=1, tau=np.float32(0.5)):
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
        d = r - np.float32(tau)
        t = (wgt * d).astype(np.float32)
        q = np.rint(np.clip(t, np.float32(-4096.0), np.float32(4096.0)).astype(np.float64) * 2.0 ** 24)
    return np.where(np.isnan(t), 0.0, q).astype(np.int64)


def changepoint_along(q, path):
    """q: (H-2,W-2) or (M,) int64 terms, path: (M,) indices into q's raster -> (k, t_max, t_all): the smallest k in 0..M with
    T(k) = sum_{i < k} q[path[i]] maximal, T(0) = 0 included."""
    q = np.asarray(q, dtype=np.int64).reshape(-1)
    path = np.asarray(path).astype(np.int64).reshape(-1)
    ok = (path >= 0) & (path < q.size)
    along = np.where(ok, q[np.where(ok, path, 0)], 0)
    T = np.concatenate([[0], np.cumsum(along, dtype=np.int64)])
    k = int(np.argmax(T))                                     # argmax: the first of equal maxima
    return k, int(T[k]), int(T[-1])


def interior_order_np(keys):
    """keys: (H,W) -> (M,) int32: the interior raster indices in ascending order of keys[1:-1, 1:-1], ties to the smaller index."""
    return np.argsort(np.asarray(keys)[1:-1, 1:-1].reshape(-1), kind="stable").astype(np.int32)


def ws_ordered_np(x, path, flip_rate=1.0, **kw):
    return changepoint_along(ordered_terms(x, tau=tau_of(flip_rate), **kw), path)


def beta_np(k, h, w, flip_rate=1.0):
    return float(flip_rate) * k / ((h - 2) * (w - 2))


def hillrm_rank(alpha, h, w):
    return int(np.floor((h * w - 1) * float(alpha)))


def hillrm_np(cover, alpha, seed, cost=None):
    """(H,W) uint8 -> the HILLRM twin.  alpha == 0: the cover.  Every pixel whose cost ties with the threshold is used."""
    cover = np.asarray(cover, dtype=np.uint8)
    if alpha == 0:
        return cover.copy()
    cost = hill_np.hill_cost(cover) if cost is None else cost
    k = hillrm_rank(alpha, *cover.shape)
    c_k = np.partition(cost.reshape(-1), k)[k]
    return np.where(cost <= c_k, embed_np.lsbr_np(cover, 1.0, seed), cover)
