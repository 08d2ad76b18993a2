"""numpy-only int64 restatement of the JPEG-history kernels (include/wsu.h K31 / K32; ws_unet_amd/ws/jpeg.py), written from the arithmetic
of DESIGN.md 4-jpeg: the 8x8 integer DCT at scale 2^13 per pass, quantisation that rounds half away from zero, the residual energy of a
table in 2^-10 units, the round trip's prediction, the IJG tables and the quality rule.  kb_plane: the KB prediction of an image without
JPEG history, in K11's float32 operation sequence."""
import numpy as np

from sequential_np import _conv9

IJG_LUMINANCE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
    [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92], [49, 64, 78, 87, 103, 121, 120, 101],
    [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.int64)
KB = np.array([[-1, 2, -1], [2, 0, 2], [-1, 2, -1]], dtype=np.float32) / np.float32(4)


def dct_matrix():
    """C[k][n] = rint(2^13 c_k cos((2n+1) k pi / 16)), int64"""
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(k == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))
    return np.rint(2.0 ** 13 * c * np.cos((2 * n + 1) * k * np.pi / 16)).astype(np.int64)


def table(q):
    """IJG luminance table of quality q in 1..100, int64 (8,8)"""
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((IJG_LUMINANCE * s + 50) // 100, 1, 255)


def tables(qualities):
    return np.stack([table(int(q)) for q in qualities])


def forward(x):
    """(H,W) uint8 -> Y (H/8, W/8, 8, 8) int64 at scale 2^26"""
    h, w = x.shape
    assert h % 8 == 0 and w % 8 == 0
    b = x.astype(np.int64).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128
    c = dct_matrix()
    return c @ b @ c.T


def quantise(y, q):
    d = np.asarray(q, dtype=np.int64) << 26
    return np.sign(y) * ((np.abs(y) + d // 2) // d)


def energy(y, q):
    """E of one plane's coefficients y = forward(x) against one (8,8) table: int"""
    r = y - quantise(y, q) * (np.asarray(q, dtype=np.int64) << 26)
    rp = (r + (1 << 15)) >> 16
    return int((rp * rp).sum())


def energies(x, tabs):
    """(N,H,W) uint8, (M,8,8) -> (N,M) int64"""
    return np.array([[energy(y, t) for t in tabs] for y in map(forward, x)], dtype=np.int64)


def bound(hw, tau=1.0):
    return int(np.floor(tau * 2.0 ** 20 * hw))


def quality(row, hw, tau=1.0):
    """row[j]: the energy at quality j + 1 -> the lowest quality whose energy is at most tau 2^20 H W (integers), 0 if none"""
    return next((q for q, e in enumerate(row, 1) if int(e) <= bound(hw, tau)), 0)


def estimate_quality(x, max_quality=95, tau=1.0):
    """(N,H,W) uint8 -> int64 (N,); the search stops at the first quality that passes"""
    out = []
    for p in x:
        y = forward(p)
        out.append(next((q for q in range(1, max_quality + 1) if energy(y, table(q)) <= bound(p.size, tau)), 0))
    return np.array(out, dtype=np.int64)


def round_trip(x, q):
    """(H,W) uint8, (8,8) table -> Z (H,W) int64 at scale 2^26, the level shift included"""
    h, w = x.shape
    y = forward(x)
    c = dct_matrix()
    z = c.T @ (quantise(y, q) * np.asarray(q, dtype=np.int64)) @ c + (128 << 26)
    return z.transpose(0, 2, 1, 3).reshape(h, w)


def kb_plane(x):
    """(H,W) uint8 -> float32 (H,W): conv(x / 255.f, KB) * 255.f on the interior (K11's sequence), the pixel itself on the border"""
    h, w = x.shape
    out = x.astype(np.float32)
    if h >= 3 and w >= 3:
        unit = [[x[i:h - 2 + i, j:w - 2 + j].astype(np.float32) / np.float32(255.0) for j in range(3)] for i in range(3)]
        out[1:-1, 1:-1] = _conv9(KB, unit) * np.float32(255.0)
    return out


def predict(x, tabs, use=None):
    """(N,H,W) uint8, one (8,8) table per image, use (N,) -> (x_hat float32 (N,H,W), recompressed uint8 (N,H,W))"""
    hats, outs = [], []
    for i, p in enumerate(x):
        if use is not None and not use[i]:
            hats.append(kb_plane(p))
            outs.append(p.copy())
            continue
        z = round_trip(p, tabs[i])
        hats.append((np.clip(z, 0, 255 << 26).astype(np.float64) / 2.0 ** 26).astype(np.float32))
        outs.append(np.clip((z + (1 << 25)) >> 26, 0, 255).astype(np.uint8))
    return np.stack(hats), np.stack(outs)


def recompress(x, q):
    """(N,H,W) uint8 at IJG quality q -> uint8"""
    return predict(x, [table(q)] * len(x))[1]


def lsbr(x, alpha, rng):
    """LSB replacement at payload alpha with numpy's generator: each pixel is used with probability alpha and takes a random bit"""
    used = rng.random(x.shape) < alpha
    bits = rng.integers(0, 2, x.shape, dtype=np.uint8)
    return np.where(used, (x & 0xFE) | bits, x).astype(np.uint8)


def beta_unweighted(x, x_hat):
    """float64 WS estimate mean((x - x_bar)(x - x_hat)) over the interior"""
    xi = x[1:-1, 1:-1].astype(np.float64)
    s = xi - (x[1:-1, 1:-1] ^ 1).astype(np.float64)
    return float((s * (xi - x_hat[1:-1, 1:-1].astype(np.float64))).mean())
