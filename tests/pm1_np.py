"""numpy-only restatements of the +-1 simulators (ws_unet_amd.embed_pm1, include/wsu.h K37-K39) and the inputs their tests share.

For a multiplier lam > 0 and a cost rho > 0 (+inf: wet), per pixel in float64:
    a = lam * rho;  a+ = inf where x == 255 else a;  a- = inf where x == 0 else a;  e+- = exp(-a+-);  Z = (1 + e+) + e-;  p+- = e+- / Z
    h = log2(Z) + (t+ + t-) / (Z ln 2),  t+- = a e+- where e+- > 0 else 0
    T+- = floor(p+- * 2^32);  u = Philox word of the pixel (embed_np);  u < T+: +1;  T+ <= u < T+ + T-: -1
LSBM: T+ = T- = T = floor(alpha / 4 * 2^32), (2T, 0) at x == 0, (0, 2T) at x == 255.
ternary_lambda is the search of ops.ternary_lambda with the entropy above: the same ladder and the same 17 geometric steps per round.
"""
import functools
import pathlib

import numpy as np

import embed_np
import hill_np

LN2 = np.log(2.0)
LADDER = np.array([2.0 ** e for e in range(-50, 26, 5)])
REFINEMENTS = 8
SEED = 7                                     # the seed of every GPU comparison (test_pm1_host asserts that no draw is near a threshold)
SHAPES = ((8, 8), (64, 64), (70, 90), (65, 130))
CONTENTS = ("noise", "photo", "flat", "ends")
ALPHAS = (0.01, 0.4, 1.0)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

def hashed(h, w, salt=0):
    """(H,W) uint32 of a multiplicative hash of the pixel index: noise without a generator's state."""
    i = np.arange(h * w, dtype=np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B9)
    v = (i * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(13)
    return v.astype(np.uint32).reshape(h, w)


def plane(content, h, w):
    """'noise': hashed bytes; 'photo': the top-left crop of tests/golden/cover_8.png; 'flat': 77 everywhere (every cost is the clamp);
    'ends': only 0 and 255 (every pixel has one wet direction): hashed left of column 80, a saturated band of 255 from there on, whose
    costs are the clamp (the two widest shapes have it)."""
    if content == "noise":
        return (hashed(h, w) >> np.uint32(11)).astype(np.uint8)
    if content == "photo":
        from PIL import Image
        img = np.asarray(Image.open(pathlib.Path(__file__).resolve().parent / "golden" / "cover_8.png"))
        assert img.ndim == 2 and img.shape[0] >= h and img.shape[1] >= w
        return np.ascontiguousarray(img[:h, :w]).astype(np.uint8)
    if content == "flat":
        return np.full((h, w), 77, dtype=np.uint8)
    if content == "ends":
        x = np.where((hashed(h, w, 1) >> np.uint32(9)) & np.uint32(1), 255, 0).astype(np.uint8)
        x[:, 80:] = 255
        return x
    raise ValueError(content)


@functools.lru_cache(maxsize=None)
def case(content, shape):
    """(x, rho) of a test input, made once and read-only: the plane and its float64 HILL cost."""
    x = plane(content, *shape)
    rho = hill_np.hill_cost(x)
    x.setflags(write=False)
    rho.setflags(write=False)
    return x, rho


@functools.lru_cache(maxsize=None)
def case_lambda(content, shape, alpha):
    """ternary_lambda of a test input at alpha bits per pixel."""
    x, rho = case(content, shape)
    return ternary_lambda(x, rho, alpha * x.size)


# ---- the formulas -------------------------------------------------------------------------------------------------------------------

def exps(x, rho, lam):
    """(a, e+, e-) of the pixels of x under the multiplier lam."""
    x = np.asarray(x)
    a = np.float64(lam) * np.asarray(rho, dtype=np.float64)
    with np.errstate(under="ignore"):
        e = np.exp(-a)
    return a, np.where(x == 255, 0.0, e), np.where(x == 0, 0.0, e)


def probabilities(x, rho, lam):
    _, ep, em = exps(x, rho, lam)
    z = (1.0 + ep) + em
    return ep / z, em / z


def entropy(x, rho, lam):
    """The sum of h over the image, in bits (math.fsum: the exact sum of the float64 terms, rounded once)."""
    import math
    a, ep, em = exps(x, rho, lam)
    z = (1.0 + ep) + em
    af = np.where(np.isfinite(a), a, 0.0)                        # where a is inf both e are 0: the product is not formed
    with np.errstate(under="ignore"):
        tp = np.where(ep > 0, af * ep, 0.0)
        tm = np.where(em > 0, af * em, 0.0)
    h = np.log2(z) + (tp + tm) / (z * LN2)
    return math.fsum(h.reshape(-1).tolist())


def ternary_lambda(x, rho, m):
    """(lam_lo, lam_hi, ok) of ops.ternary_lambda for one image and a payload of m bits."""
    ge = np.array([entropy(x, rho, lam) >= m for lam in LADDER])
    if not ge[0]:
        return LADDER[0], LADDER[0], False
    k = int(np.nonzero(ge)[0].max())
    lo, hi = LADDER[k], LADDER[min(k + 1, len(LADDER) - 1)]
    steps = np.arange(1, 17, dtype=np.float64) / 17
    for _ in range(REFINEMENTS):
        inner = np.minimum(np.maximum(lo * np.exp2(np.log2(hi / lo) * steps), lo), hi)
        pts = np.concatenate([[lo], inner, [hi]])
        ge = np.array([True] + [entropy(x, rho, lam) >= m for lam in inner] + [False])
        k = int(np.nonzero(ge)[0].max())
        lo, hi = pts[k], pts[k + 1]
    return lo, hi, True


def words(n, seed):
    """The generator word of each of n pixels under the 64-bit seed (embed_np.lsbr_np's)."""
    groups = (n + 3) // 4
    counter = np.zeros((groups, 4), dtype=np.uint32)
    counter[:, 0] = np.arange(groups, dtype=np.uint32)
    seed = int(seed) % 2 ** 64
    return embed_np.philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n].astype(np.int64)


def ternary_thresholds(x, rho, lam):
    pp, pm = probabilities(x, rho, lam)
    return np.floor(pp * 2.0 ** 32).astype(np.int64), np.floor(pm * 2.0 ** 32).astype(np.int64)


def lsbm_threshold(alpha):
    return int(np.floor(np.float64(alpha) / 4 * 2.0 ** 32))


def lsbm_thresholds(x, alpha):
    x = np.asarray(x)
    t = np.int64(lsbm_threshold(alpha))
    return np.where(x == 255, 0, np.where(x == 0, 2 * t, t)).astype(np.int64), np.where(x == 0, 0, np.where(x == 255, 2 * t, t)).astype(np.int64)


def draw(x, tp, tm, seed):
    """(stego as int64, not clipped; changes) of the cover x under the per-pixel thresholds."""
    x = np.asarray(x)
    u = words(x.size, seed).reshape(x.shape)
    d = np.where(u < tp, 1, np.where(u < tp + tm, -1, 0))
    return x.astype(np.int64) + d, int(np.count_nonzero(d))


def min_gap(x, tp, tm, seed):
    """The smallest distance of a pixel's draw from one of its two thresholds."""
    u = words(np.asarray(x).size, seed).reshape(np.asarray(x).shape)
    return int(min(np.abs(u - tp).min(), np.abs(u - (tp + tm)).min()))


def ternary_np(x, rho, lam, seed):
    stego, changes = draw(x, *ternary_thresholds(x, rho, lam), seed)
    return stego, changes


def lsbm_np(x, alpha, seed):
    return draw(x, *lsbm_thresholds(x, alpha), seed)
