"""numpy-only restatement of the directional wavelet cost map of S-UNIWARD and WOW (ws_unet_amd.costs, include/wsu.h K48) and the
inputs its tests share.  Everything is float64; each of the four filter passes adds its 16 taps in ascending order from +0.0, a product
and its addition being two roundings, which is what K48 does: the kernel's plane must equal `cost` bit for bit.

    X~ = numpy.pad(x, mode='symmetric');  l[j] = p[15 - j],  h[j] = (-1)^(j+1) p[j],  p = costs.DB8;  (a,b) = (l,h), (h,l), (h,h)
    r_b[y,n] = sum_v b[v] X~[y, n+8-v]          W_k[m,n] = sum_u a_k[u] r_bk[m+8-u, n]          n in [-8, W+6], m in [-8, H+6]
    g_k = 1 / (|W_k| + sigma)  or  |W_k|
    t_k[m,j] = sum_v |b_k[v]| g_k[m, j-8+v]     xi_k[i,j] = sum_u |a_k[u]| t_k[i-8+u, j]
    rho = (xi_1 + xi_2) + xi_3  or  (1/xi_1 + 1/xi_2) + 1/xi_3;   rho <= clamp ? rho : clamp
"""
import functools
import pathlib

import numpy as np

from ws_unet_amd.costs import DB8

P = np.array(DB8, dtype=np.float64)
L = P[::-1].copy()
H = np.array([p if j % 2 else -p for j, p in enumerate(DB8)], dtype=np.float64)
BANDS = ((L, H), (H, L), (H, H))                                            # (a_k down the rows, b_k along the columns)
CLAMPS = {"suniward": 1e8, "wow": 1e10}
PAD = 16

SHAPES = ((3, 5), (8, 16), (24, 40), (33, 31), (32, 32), (33, 33), (65, 97))     # 32 = the kernel's tile
CONTENTS = ("noise", "photo", "flat", "ends", "stripes")


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

def hashed(h, w, salt=0):
    """(H,W) uint32 of a multiplicative hash of the pixel index: noise without a generator's state."""
    i = np.arange(h * w, dtype=np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B9)
    v = (i * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(13)
    return v.astype(np.uint32).reshape(h, w)


def golden_cover(k=6):
    from PIL import Image
    img = np.asarray(Image.open(pathlib.Path(__file__).resolve().parent / "golden" / f"cover_{k}.png"))
    assert img.ndim == 2 and img.dtype == np.uint8
    return img


def plane(content, h, w):
    """'noise': hashed bytes; 'photo': the crop of tests/golden/cover_6.png at (100, 200); 'flat': 77 everywhere; 'ends': only 0 and
    255; 'stripes': vertical stripes two pixels wide, 40 and 200 (no variation down the columns)."""
    if content == "noise":
        return (hashed(h, w) >> np.uint32(11)).astype(np.uint8)
    if content == "photo":
        return np.ascontiguousarray(golden_cover()[100:100 + h, 200:200 + w])
    if content == "flat":
        return np.full((h, w), 77, dtype=np.uint8)
    if content == "ends":
        return np.where((hashed(h, w, 1) >> np.uint32(9)) & np.uint32(1), 255, 0).astype(np.uint8)
    if content == "stripes":
        return np.ascontiguousarray(np.broadcast_to(np.where((np.arange(w) // 2) % 2, 200, 40).astype(np.uint8), (h, w)))
    raise ValueError(content)


@functools.lru_cache(maxsize=None)
def case(content, shape, kind):
    """(x, rho) of a test input at the default sigma and clamp, made once and read-only."""
    x = plane(content, *shape)
    rho = cost(x, kind)
    x.setflags(write=False)
    rho.setflags(write=False)
    return x, rho


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def padded(x):
    return np.pad(np.asarray(x).astype(np.float64), PAD, mode="symmetric")


def row_transform(xp, b, h, w):
    """r_b[y, n] for y in [-15, H+14] (index y + 15) and n in [-8, W+6] (index n + 8)"""
    r = np.zeros((h + 30, w + 15))
    for v in range(16):
        r = r + b[v] * xp[1:h + 31, PAD - v:PAD - v + w + 15]
    return r


def forward(x):
    """[W_1, W_2, W_3], each (H+15, W+15): W_k[m, n] at index (m + 8, n + 8)"""
    h, w = np.asarray(x).shape
    xp = padded(x)
    out = []
    for a, b in BANDS:
        r = row_transform(xp, b, h, w)
        wk = np.zeros((h + 15, w + 15))
        for u in range(16):
            wk = wk + a[u] * r[15 - u:15 - u + h + 15, :]
        out.append(wk)
    return out


def weight(wk, kind, sigma=1.0):
    if kind == "suniward":
        return 1.0 / (np.abs(wk) + np.float64(sigma))
    if kind == "wow":
        return np.abs(wk)
    raise ValueError(kind)


def back(g, a, b, h, w, di=0, dj=0):
    """xi[i, j] = sum_u |a[u]| sum_v |b[v]| g[i-8+u, j-8+v], the row pass first.  di, dj shift the two back-projection indices (0 is the
    definition; the alignment test shows that +-1 breaks UNIWARD's identity)."""
    g = np.pad(g, 1)
    t = np.zeros((h + 17, w))
    for v in range(16):
        t = t + np.abs(b[v]) * g[:, 1 + dj + v:1 + dj + v + w]
    xi = np.zeros((h, w))
    for u in range(16):
        xi = xi + np.abs(a[u]) * t[1 + di + u:1 + di + u + h, :]
    return xi


def bands_xi(x, kind, sigma=1.0, di=0, dj=0):
    h, w = np.asarray(x).shape
    return [back(weight(wk, kind, sigma), a, b, h, w, di, dj) for wk, (a, b) in zip(forward(x), BANDS)]


def cost(x, kind, sigma=1.0, clamp=None, di=0, dj=0):
    """The (H,W) float64 cost plane of the uint8 plane x."""
    clamp = np.float64(CLAMPS[kind] if clamp is None else clamp)
    x1, x2, x3 = bands_xi(x, kind, sigma, di, dj)
    with np.errstate(divide="ignore"):
        rho = (x1 + x2) + x3 if kind == "suniward" else (1.0 / x1 + 1.0 / x2) + 1.0 / x3
    return np.where(rho <= clamp, rho, clamp)


# ---- the direct 2-D form (768 terms per pixel), for the separable one to be held against -------------------------------------------

def direct_cost_at(x, i, j, kind, sigma=1.0, clamp=None):
    """rho[i, j] from the full kernels F_k = a_k b_k^T and |F_k|: W_k[m,n] = sum_{u,v} F_k[u,v] X~[m+8-u, n+8-v] at the 256 positions
    (m, n) = (i-8+u, j-8+v), then xi_k = sum_{u,v} |F_k[u,v]| g_k[i-8+u, j-8+v]."""
    xp = padded(x)
    xi = []
    for a, b in BANDS:
        f = np.outer(a, b)
        s = 0.0
        for u in range(16):
            for v in range(16):
                m, n = i - 8 + u, j - 8 + v
                win = xp[m + 8 - 15 + PAD:m + 8 + 1 + PAD, n + 8 - 15 + PAD:n + 8 + 1 + PAD]       # X~[m+8-15 .. m+8, n+8-15 .. n+8]
                wk = float((f[::-1, ::-1] * win).sum())
                s += abs(f[u, v]) * float(weight(np.float64(wk), kind, sigma))
        xi.append(s)
    clamp = CLAMPS[kind] if clamp is None else clamp
    with np.errstate(divide="ignore"):
        rho = (xi[0] + xi[1]) + xi[2] if kind == "suniward" else (np.float64(1.0) / xi[0] + np.float64(1.0) / xi[1]) + np.float64(1.0) / xi[2]
    return float(rho) if rho <= clamp else float(clamp)
