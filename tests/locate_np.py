"""numpy-only restatements of the payload locator (include/wsu.h K29, ws_unet_amd/ws/locate.py) and of the keyed simulator LSBRK (K30).

terms: the per-pixel float32 terms t = wgt * (s * res) of one plane in K11's operation sequence (every product and sum a separate float32
rounding, the nine taps of a true convolution added K00 .. K22 from 0) and the two fixed-point integers a pixel adds,
q = rint(clip(t, -4096, 4096) * 2^24) and dq = rint(float64(wgt) * 2^32), both 0 where t is NaN.  accumulate: their sums over images.
residual_mean / decide_threshold / decide_count / confusion: the float64 mean num * 256 / den, the two decisions and their score.
key_mask_np / lsbrk_np: Philox4x32-10 of embed_np; a pixel is used iff its word under the stego key is below floor(alpha * 2^32), and a
used pixel flips iff its word under the image's seed is below 2^31."""
import numpy as np

import embed_np
from sequential_np import _conv9


def terms(x, x_hat=None, hat_scale=255., pixel_kernel=None, mean_kernel=None, weighted=1):
    """x: (H,W) uint8.  x_hat: (H,W) full frame or (H-2,W-2) interior, float32, multiplied by hat_scale; or pixel_kernel (3,3) K[a][b].
    -> (q, dq) int64 (H-2,W-2)."""
    x = np.asarray(x, dtype=np.uint8)
    h, w = x.shape
    v = [[x[i:h - 2 + i, j:w - 2 + j].astype(np.float32) for j in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        wgt = np.ones((h - 2, w - 2), dtype=np.float32)
        if weighted:
            v2 = [[p * p for p in row] for row in v]
            mu, mu2 = _conv9(mean_kernel, v), _conv9(mean_kernel, v2)
            var = mu2 - mu * mu
            wgt = (np.float32(1.0) / (np.float32(5.0) + var)).astype(np.float32)
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
        t = (wgt * r).astype(np.float32)
        nan = np.isnan(t)
        q = np.rint(np.clip(np.where(nan, np.float32(0), t), np.float32(-4096.0), np.float32(4096.0)).astype(np.float64) * 2.0 ** 24)
        dq = np.rint(np.where(nan, 0.0, wgt.astype(np.float64)) * 2.0 ** 32)
    return np.where(nan, 0.0, q).astype(np.int64), np.where(nan, 0.0, dq).astype(np.int64)


def accumulate(planes, x_hats=None, hat_scale=255., pixel_kernels=None, mean_kernel=None, weighted=1, num=None, den=None):
    """planes: (N,H,W) uint8; x_hats: per image, or pixel_kernels: per image -> (num, den) int64 (H-2,W-2), added to the given ones."""
    planes = np.asarray(planes, dtype=np.uint8)
    n, h, w = planes.shape
    num = np.zeros((h - 2, w - 2), dtype=np.int64) if num is None else num.copy()
    den = np.zeros((h - 2, w - 2), dtype=np.int64) if den is None else den.copy()
    for i in range(n):
        q, dq = terms(planes[i], x_hat=None if x_hats is None else x_hats[i], hat_scale=hat_scale,
                      pixel_kernel=None if pixel_kernels is None else pixel_kernels[i], mean_kernel=mean_kernel, weighted=weighted)
        num += q
        den += dq
    return num, den


def residual_mean(num, den):
    """float64 num * 256 / den; NaN where den = 0"""
    n, d = num.astype(np.float64), den.astype(np.float64)
    out = np.full(n.shape, np.nan)
    np.divide(n * 256.0, d, out=out, where=d != 0)
    return out


def decide_threshold(mean, threshold=0.25):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(mean), False, mean > threshold)


def decide_count(mean, count):
    """the `count` largest means; among equal means the smaller row-major index first; a NaN ranks last and is never used"""
    flat = mean.reshape(-1)
    idx = sorted(range(flat.size), key=lambda i: (np.isnan(flat[i]), -flat[i] if not np.isnan(flat[i]) else 0.0, i))
    used = np.zeros(flat.size, dtype=bool)
    for i in idx[:count]:
        used[i] = not np.isnan(flat[i])
    return used.reshape(mean.shape)


def confusion(used, truth):
    used, truth = np.asarray(used).astype(bool), np.asarray(truth).astype(bool)
    tp, fp = int((used & truth).sum()), int((used & ~truth).sum())
    tn, fn = int((~used & ~truth).sum()), int((~used & truth).sum())
    return {"tp": tp, "fp": fp, "tn": tn, "fn": fn, "accuracy": (tp + tn) / used.size}


def key_threshold(alpha):
    return int(np.floor(np.float64(alpha) * 2.0 ** 32))


def _words(n, seed):
    groups = (n + 3) // 4
    counter = np.zeros((groups, 4), dtype=np.uint32)
    counter[:, 0] = np.arange(groups, dtype=np.uint32)
    seed = int(seed) % 2 ** 64
    return embed_np.philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n].astype(np.uint64)


def key_mask_np(key_seed, alpha, h, w):
    """(H,W) uint8: 1 where the stego key uses the pixel"""
    return (_words(h * w, key_seed) < np.uint64(key_threshold(alpha))).reshape(h, w).astype(np.uint8)


def lsbrk_np(cover, alpha, seed, key_seed):
    """(H,W) uint8 -> the LSBRK twin"""
    cover = np.asarray(cover, dtype=np.uint8)
    flip = (_words(cover.size, seed) < np.uint64(1 << 31)).reshape(cover.shape).astype(np.uint8)
    return cover ^ (flip & key_mask_np(key_seed, alpha, *cover.shape))
