"""The Daubechies-8 orthonormal scaling filter (16 taps, minimum phase) by spectral factorisation: the derivation behind the literals
`ws_unet_amd.costs.DB8` and `DB8` of ws_unet_amd/csrc/wavelet_cost.hip (K48).  `python tools/db8_taps.py` prints them with 17 digits.

|m0(w)|^2 = cos^16(w/2) P(sin^2(w/2)) with P(y) = sum_{k=0..7} C(7+k, k) y^k (I. Daubechies, "Orthonormal bases of compactly supported
wavelets", CPAM 41, 1988).  With y = (2 - z - 1/z) / 4 every root y_k of P gives the pair z, 1/z of z^2 - (2 - 4 y_k) z + 1 = 0; the
minimum-phase factor keeps the one inside the unit circle.  The filter is (1 + z)^8 prod_k (z - z_k), scaled to sum sqrt 2.

`derive` does that: the roots of P come from numpy's companion-matrix eigenvalues and are polished by Newton steps in extended precision
(numpy's longdouble where it is wider than float64).

`taps` then rounds to float64 UNDER THE FILTER'S DESIGN CONDITIONS.  The kernel filters with the float64 values, so what annihilates
polynomials there is the moments sum_j (-1)^j j^q p[j], q = 0..7, of the float64 values themselves.  Rounding every tap to its nearest
float64 leaves the seventh moment at 1.2e-11 (half a unit in the last place of p[7] alone moves it by 1.1e-11; the exact taps have 0).
So each tap may move to a float64 at most MAX_STEPS units in the last place from the nearest one, and the steps are chosen, by a
deterministic descent over single taps and pairs of taps, to make the largest of the eight moments (exact rational arithmetic over the
float64 values) as small as the descent finds: 2.4e-13 with six taps moved by one or two units.  A step is 1e-17 or less, so the sum and the
orthonormality conditions stay at the 1e-16 they had."""
import itertools
import math
from fractions import Fraction

import numpy as np

ORDER = 8
MAX_STEPS = 2


def derive(order: int = ORDER) -> np.ndarray:
    """p[0 .. 2 order - 1] in numpy's longdouble: sum p = sqrt 2, p[0] the first tap of the minimum-phase filter (0.0544158422... for order 8)."""
    ld, cld = np.longdouble, np.clongdouble
    coef = [math.comb(order - 1 + k, k) for k in range(order)]                  # ascending in y
    ys = np.roots(np.array(coef[::-1], dtype=np.float64)).astype(cld)
    c = np.array(coef, dtype=ld)
    for _ in range(4):                                                           # Newton on P, extended precision
        pv = sum(c[k] * ys ** k for k in range(order))
        dv = sum(k * c[k] * ys ** (k - 1) for k in range(1, order))
        ys = ys - pv / dv
    b = ld(2) - ld(4) * ys                                                       # z^2 - b z + 1 = 0
    root = np.sqrt(b * b - ld(4))
    z1, z2 = (b + root) / ld(2), (b - root) / ld(2)
    zs = np.where(np.abs(z1) < 1, z1, z2)
    assert np.all(np.abs(zs) < 1)
    poly = np.array([1], dtype=cld)                                              # descending powers of z
    for _ in range(order):
        poly = np.convolve(poly, np.array([1, 1], dtype=cld))
    for z in zs:
        poly = np.convolve(poly, np.array([1, -z], dtype=cld))
    assert float(np.abs(poly.imag).max()) < 1e-12 * float(np.abs(poly.real).max())
    p = poly.real
    return p * (np.sqrt(ld(2)) / p.sum())


def moments(p) -> np.ndarray:
    """sum_j (-1)^j j^q p[j] for q = 0 .. len(p) / 2 - 1 of the float64 values p, in exact rational arithmetic, rounded once"""
    return np.array([float(sum(Fraction((-1) ** j * j ** q) * Fraction(float(v)) for j, v in enumerate(p))) for q in range(len(p) // 2)])


def taps(order: int = ORDER) -> np.ndarray:
    """The float64 taps: `derive` rounded under the moment conditions (the module's text)."""
    p = np.asarray(derive(order), dtype=np.float64)
    n = p.size
    ulp = np.array([math.ulp(v) for v in p])
    m0 = moments(p)
    lever = np.array([[(-1) ** j * float(j) ** q * ulp[j] for j in range(n)] for q in range(n // 2)])     # moment q per step of tap j
    moves = [((j, d),) for j in range(n) for d in (-1, 1)]
    moves += [((j1, d1), (j2, d2)) for j1, j2 in itertools.combinations(range(n), 2) for d1 in (-1, 1) for d2 in (-1, 1)]
    k = np.zeros(n, dtype=np.int64)
    best = float(np.abs(m0).max())
    while True:
        found = None
        for move in moves:                                                       # in a fixed order; the first of equal candidates is kept
            kk = k.copy()
            for j, d in move:
                kk[j] += d
            if np.abs(kk).max() > MAX_STEPS:
                continue
            worst = float(np.abs(m0 + lever @ kk).max())
            if worst < (best if found is None else found[0]):
                found = (worst, kk)
        if found is None:
            break
        best, k = found
    out = p.copy()
    for j in range(n):
        for _ in range(abs(int(k[j]))):
            out[j] = np.nextafter(out[j], math.inf if k[j] > 0 else -math.inf)
    return out


if __name__ == "__main__":
    for v in taps():
        print(f"{v:.17g}")
