"""numpy-only restatement of the ternary two-layer syndrome-trellis embedder (ws_unet_amd.stc_ml, include/wsu.h K43-K47; Filler, Judas,
Fridrich, IEEE TIFS 6(3), 2011, sections V-VI, for +-1 changes), written from the definition in the header over stc_np's binary code and
pm1_np's exponentials and multiplier search, and the fixture grid the CPU and GPU tests share.

Per image: cover x in 0..255 (n pixels), one cost rho >= 0 per pixel for both directions (+inf: wet), a message m[0..k), k >= 2, the
constraint height h and the seed.  lambda = the lower end of pm1_np.ternary_lambda(x, rho, k).  K37's text, unchanged:
    a = lambda * rho;  a+ = +inf where x == 255 else a;  a- = +inf where x == 0 else a;  e+- = exp(-a+-);  Z = (1 + e+) + e-
d = the direction that changes bit 1 of x: +1 for odd x, -1 for even x; o = the other direction.
  high layer:  u1 = (x >> 1) & 1;  rho1 = a_d + log1p(e_o) (+inf where a_d is);  H1 = the sum of the binary entropy of q1 = e_d / Z in bits,
               each term (r log1p(t)) / ln 2 - q1 log2(q1) where e_d > 0 else 0, r = (1 + e_o) / Z, t = e_d / (1 + e_o);
               k1 = min(floor(H1), k - 1);  k1 == 0: y1 = u1;  else y1 = stc_np.viterbi(u1, rho1, m[0..k1))
  low layer:   k0 = k - k1;  where y1 != u1: u0 = 1 - (x & 1), rho0 = +inf;  elsewhere u0 = x & 1, rho0 = a_o;
               y0 = stc_np.viterbi(u0, rho0, m[k1..k))
  stego:       x + d where y1 != u1;  x + o where bit 1 was kept and y0 != (x & 1);  x otherwise;  ok = ok1 and ok0, else the cover
Both layers run along stc_np.key_path(seed) with stc_np.columns(h, .).  The receiver reads m[0..k1) from bit 1 and m[k1..k) from bit 0."""
import functools
import math

import numpy as np

import pm1_np
import stc_np

LN2 = np.log(2.0)
SEED = stc_np.SEED
CONTENTS = ("noise", "photo", "flat", "ends")
SHAPES = ((8, 16), (24, 40), (33, 31))
ALPHAS = (0.1, 0.4, 1.0)


def heights(shape):
    """6 and 7 everywhere (K41's one-wave and many-waves organisations), 10 at (24, 40)"""
    return (6, 7, 10) if shape == (24, 40) else (6, 7)


FIXTURES = [(c, s, a, h) for c in CONTENTS for s in SHAPES for a in ALPHAS for h in heights(s)]


def bits_of(shape, alpha):
    return int(round(alpha * shape[0] * shape[1]))


# ---- the planes ---------------------------------------------------------------------------------------------------------------------

def directions(x, rho, lam):
    """(a_d, a_o, e_d, e_o, Z) of the pixels"""
    x = np.asarray(x)
    a, ep, em = pm1_np.exps(x, rho, lam)
    ap, am = np.where(x == 255, np.inf, a), np.where(x == 0, np.inf, a)
    odd = (x & 1) == 1
    return np.where(odd, ap, am), np.where(odd, am, ap), np.where(odd, ep, em), np.where(odd, em, ep), (1.0 + ep) + em


def high_planes(x, rho, lam):
    """(u1, rho1, the per-pixel entropies h1)"""
    ad, _, ed, eo, z = directions(x, rho, lam)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        q, r, t = ed / z, (1.0 + eo) / z, ed / (1.0 + eo)
        h1 = np.where(ed > 0, (r * np.log1p(t)) / LN2 - q * np.log2(np.where(ed > 0, q, 1.0)), 0.0)
    return ((np.asarray(x) >> 1) & 1).astype(np.uint8), ad + np.log1p(eo), h1


def high_entropy(h1):
    """math.fsum: the exact sum of the float64 terms, rounded once"""
    return math.fsum(np.asarray(h1).reshape(-1).tolist())


def low_planes(x, rho, lam, y1, k1):
    x = np.asarray(x)
    _, ao, _, _, _ = directions(x, rho, lam)
    decided = (np.asarray(y1) & 1) != ((x >> 1) & 1) if k1 > 0 else np.zeros(x.shape, bool)
    return np.where(decided, 1 - (x & 1), x & 1).astype(np.uint8), np.where(decided, np.inf, ao)


def compose(x, rho, y1, y0, k1, ok):
    """(stego uint8, changes, distortion (math.fsum))"""
    x = np.asarray(x)
    xi = x.astype(np.int64)
    d = np.where(x & 1, 1, -1)
    decided = ((np.asarray(y1) & 1) != ((x >> 1) & 1)) if (ok and k1 > 0) else np.zeros(x.shape, bool)
    low = (~decided & ((np.asarray(y0) & 1) != (x & 1))) if ok else np.zeros(x.shape, bool)
    out = np.where(decided, xi + d, np.where(low, xi - d, xi))
    assert out.min() >= 0 and out.max() <= 255
    changed = decided | low
    return out.astype(np.uint8), int(changed.sum()), math.fsum(np.asarray(rho)[changed].tolist())


# ---- the embedder ---------------------------------------------------------------------------------------------------------------------

def layer(u, r, m, h, path, n, wmax_k):
    """one binary code along the path: (the coded plane, ok); no message bits: the plane itself"""
    if len(m) == 0:
        return u.copy(), True
    cols = stc_np.columns(h, -(-n // wmax_k))
    y, _, ok = stc_np.viterbi(u.reshape(-1)[path], r.reshape(-1)[path], m, cols, h)
    out = np.zeros(n, np.uint8)
    out[path] = y
    return out.reshape(u.shape), ok


def embed(x, rho, m, h, seed=SEED, lam=None, k1=None, permute=True):
    """-> dict(stego, changes, distortion, ok, ok1, ok0, fits, k1, k0, lam, H1, u1, rho1, y1, u0, rho0, y0).  lam and k1 can be given (the GPU
    tests pass the device's, so that one unit in the last place of a library function cannot move a length)."""
    x, rho, m = np.asarray(x, np.uint8), np.asarray(rho, np.float64), np.asarray(m, np.uint8)
    n, k = x.size, len(m)
    assert k >= 2
    fits = True
    if lam is None:
        lam, _, fits = pm1_np.ternary_lambda(x, rho, float(k))
    u1, rho1, h1 = high_planes(x, rho, lam)
    H1 = high_entropy(h1)
    if k1 is None:
        k1 = int(min(math.floor(H1), k - 1))
    k0 = k - k1
    path = stc_np.key_path(seed, n) if permute else np.arange(n)
    shortest = min(v for v in (k1, k0) if v > 0)
    y1, ok1 = layer(u1, rho1, m[:k1], h, path, n, shortest)
    u0, rho0 = low_planes(x, rho, lam, y1, k1)
    y0, ok0 = layer(u0, rho0, m[k1:], h, path, n, shortest)
    ok = bool(fits and ok1 and ok0)
    stego, changes, distortion = compose(x, rho, y1, y0, k1, ok)
    return dict(stego=stego, changes=changes, distortion=distortion, ok=ok, ok1=ok1, ok0=ok0, fits=fits, k1=k1, k0=k0, lam=lam, H1=H1, u1=u1,
                rho1=rho1, y1=y1, u0=u0, rho0=rho0, y0=y0)


def extract(stego, k1, k0, h, seed=SEED, permute=True):
    s = np.asarray(stego, np.uint8).reshape(-1)
    n = s.size
    path = stc_np.key_path(seed, n) if permute else np.arange(n)
    cols = stc_np.columns(h, -(-n // min(v for v in (k1, k0) if v > 0)))
    hi = stc_np.syndrome((s[path] >> 1) & 1, k1, cols, h) if k1 > 0 else np.zeros(0, np.uint8)
    return np.concatenate([hi, stc_np.syndrome(s[path] & 1, k0, cols, h)])


def expected_distortion(x, rho, lam):
    """the ternary sender's expectation: the sum of rho (p+ + p-) over the dry pixels"""
    pp, pm = pm1_np.probabilities(x, rho, lam)
    p = pp + pm
    return math.fsum(np.where(p > 0, np.where(np.isfinite(rho), rho, 0.0) * p, 0.0).reshape(-1).tolist())


# ---- shared inputs --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(content, shape):
    """(x, rho): pm1_np.plane and its float64 HILL cost, read-only"""
    return pm1_np.case(content, shape)


@functools.lru_cache(maxsize=None)
def message(shape, alpha):
    m = stc_np.random_message(SEED, bits_of(shape, alpha))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def reference(content, shape, alpha, h):
    """embed() of a fixture with stc_np.random_message under SEED, computed once"""
    x, rho = case(content, shape)
    return embed(x, rho, message(shape, alpha), h)
