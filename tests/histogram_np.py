"""numpy-only restatement of the segment histograms (K58), the adjacency histogram (K59), the 2 x 2 calibration image (K60) and of the
host statistics of ws_unet_amd.histogram (chi-square p-value, message length, HCF centres of mass), written from their definitions
(include/wsu.h; Westfeld, Pfitzmann 1999; Harmsen, Pearlman 2003; Ker 2005), one image at a time.  The incomplete gamma function is its
own series / continued fraction, so that nothing here depends on torch or scipy."""
import math

import numpy as np

ORDERS = ("rows", "rows_up")


def seg_hist(x_u8, segments=1, order="rows"):
    """(H,W) uint8 -> (S,256) int64, or (N,H,W) -> (N,S,256): pixel (r,c) has the path position t = r W + c ('rows') or (H-1-r) W + c
    ('rows_up') and is counted in segment floor(t S / (H W)), in Python integers."""
    x = np.asarray(x_u8)
    if x.ndim == 3:
        return np.stack([seg_hist(p, segments, order) for p in x])
    assert order in ORDERS
    h, w = x.shape
    path = (x if order == "rows" else x[::-1]).reshape(-1).astype(np.int64)
    s = np.array([t * segments // (h * w) for t in range(h * w)], dtype=np.int64) if h * w < 4096 else \
        (np.arange(h * w, dtype=np.int64) * segments) // (h * w)                      # < 2^63 for every shape of the tests
    return np.bincount(s * 256 + path, minlength=segments * 256).astype(np.int64).reshape(segments, 256)


def seg_lengths(h, w, segments):
    """the pixels of every segment: ceil((s+1) H W / S) - ceil(s H W / S)"""
    edge = [-((-s * h * w) // segments) for s in range(segments + 1)]
    return np.diff(np.array(edge, dtype=np.int64))


def adjacency(x_u8):
    """(H,W) uint8 -> (256,256) int64, or (N,H,W) -> (N,256,256): A[u][v] = #{(r,c): c + 1 < W, x[r,c] = u, x[r,c+1] = v}."""
    x = np.asarray(x_u8)
    if x.ndim == 3:
        return np.stack([adjacency(p) for p in x])
    u, v = x[:, :-1].reshape(-1).astype(np.int64), x[:, 1:].reshape(-1).astype(np.int64)
    return np.bincount(u * 256 + v, minlength=65536).astype(np.int64).reshape(256, 256)


def downsample(x_u8):
    """(..., H, W) uint8 -> (..., H//2, W//2) uint8: floor of the 2 x 2 block sum over 4; an odd last row or column is dropped."""
    x = np.asarray(x_u8).astype(np.int64)
    h2, w2 = x.shape[-2] // 2 * 2, x.shape[-1] // 2 * 2
    x = x[..., :h2, :w2]
    return ((x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) // 4).astype(np.uint8)


def gammaincc(a, x):
    """Q(a, x), the regularised upper incomplete gamma function of scalars a > 0, x >= 0: the series of P = 1 - Q for x < a + 1, the
    continued fraction of Q (modified Lentz) beyond, both with the prefactor exp(-x + a ln x - lgamma(a))."""
    if x <= 0.:
        return 1.
    log_pre = -x + a * math.log(x) - math.lgamma(a)
    if x < a + 1.:
        term = total = 1. / a
        n = 0
        while abs(term) > abs(total) * 1e-17:
            n += 1
            term *= x / (a + n)
            total += term
        return 1. - total * math.exp(log_pre)
    tiny = 1e-300
    b = x + 1. - a
    c, d = 1. / tiny, 1. / b
    f = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1. / d
        delta = d * c
        f *= delta
        if abs(delta - 1.) < 1e-15:
            break
    return f * math.exp(log_pre) if log_pre > -745. else 0.


def chi2(hist, min_pair=10):
    """(256,) histogram -> (statistic, dof, p) as Python numbers; (..., 256) -> arrays of the leading shape."""
    hist = np.asarray(hist)
    if hist.ndim > 1:
        out = [chi2(row, min_pair) for row in hist.reshape(-1, 256)]
        lead = hist.shape[:-1]
        return (np.array([o[0] for o in out]).reshape(lead), np.array([o[1] for o in out], dtype=np.int64).reshape(lead),
                np.array([o[2] for o in out]).reshape(lead))
    stat, kept = 0., 0
    for k in range(128):
        e, o = int(hist[2 * k]), int(hist[2 * k + 1])
        if e + o >= min_pair:
            kept += 1
            stat += (e - o) ** 2 / (2. * (e + o))
    dof = kept - 1
    return stat, dof, (gammaincc(dof / 2., stat / 2.) if dof >= 1 else 0.)


def curve(x_u8, segments=100, order="rows", min_pair=10):
    """(H,W) uint8 -> (S,) p-values of the prefixes of the path"""
    return chi2(np.cumsum(seg_hist(x_u8, segments, order), axis=0), min_pair)[2]


def length(p, threshold=0.5):
    """(S,) -> the number of leading entries >= threshold, over S"""
    p = np.asarray(p)
    if p.ndim > 1:
        return np.array([length(row, threshold) for row in p])
    n = 0
    while n < len(p) and p[n] >= threshold:
        n += 1
    return n / len(p)


def com(hist):
    """(256,) -> sum_{k<128} k |F[k]| / sum_{k<128} |F[k]|, F = the DFT of the histogram"""
    mag = np.abs(np.fft.fft(np.asarray(hist, dtype=np.float64)))[:128]
    return float((np.arange(128) * mag).sum() / mag.sum())


def com2(A):
    """(256,256) -> sum_{k,l<128} (k + l) |F2[k,l]| / sum |F2[k,l]|, F2 = the two-dimensional DFT of the adjacency histogram"""
    mag = np.abs(np.fft.fft2(np.asarray(A, dtype=np.float64)))[:128, :128]
    k = np.arange(128)
    return float(((k[:, None] + k[None, :]) * mag).sum() / mag.sum())


def output(x_u8, detector):
    """one (H,W) plane -> the score of ws_unet_amd.histogram.outputs"""
    if detector == "CHI2":
        return chi2(seg_hist(x_u8)[0])[2]
    if detector == "HCF":
        return -com(seg_hist(x_u8)[0])
    if detector == "HCF2":
        return -com2(adjacency(x_u8))
    if detector == "HCFC":
        return com(seg_hist(downsample(x_u8))[0]) / com(seg_hist(x_u8)[0])
    if detector == "HCF2C":
        return com2(adjacency(downsample(x_u8))) / com2(adjacency(x_u8))
    raise ValueError(detector)
