"""CPU: the host side of the wavelet costs (ws_unet_amd.costs, include/wsu.h K48) -- the Daubechies-8 literals and their derivation, the
numpy restatement (costs_np) against the direct 2-D definition, UNIWARD's identity rho[i,j] = D(X, X + e_ij), which pins the alignment of
the two filter passes, flat and photographic planes, the names, and the argument checks of the C entry (no GPU here)."""
import math
from fractions import Fraction
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import costs_np
from ws_unet_amd import costs, embed, embed_pm1, stc, stc_ml

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import db8_taps  # noqa: E402

P = np.array(costs.DB8)


@pytest.fixture(scope="module")
def lib():
    from ws_unet_amd import _lib
    return _lib.load()


# ---- the filter -----------------------------------------------------------------------------------------------------------------------

def test_db8_is_orthonormal_with_eight_vanishing_moments():
    assert len(costs.DB8) == 16 and abs(P.sum() - math.sqrt(2.0)) <= 1e-12
    assert [f"{v:.10f}" for v in P[:5]] == ["0.0544158422", "0.3128715909", "0.6756307363", "0.5853546837", "-0.0158291053"]
    for m in range(8):
        assert abs(float(P[:16 - 2 * m] @ P[2 * m:]) - (1.0 if m == 0 else 0.0)) <= 1e-12, m


def _moment(q):
    """sum_j (-1)^j j^q p[j] of the literals, in exact rational arithmetic: only the literals are judged, no summation error"""
    return float(sum(Fraction((-1) ** j * j ** q) * Fraction(p) for j, p in enumerate(costs.DB8)))


@pytest.mark.parametrize("q", range(8))
def test_db8_moment_vanishes_to_1e_12(q):
    """The bound is absolute, 1e-12 for every q.  Taps rounded to their nearest float64 miss it at q = 7 (1.185e-11: half a unit in the last
    place of p[7] alone moves that moment by 1.1e-11), so tools/db8_taps.py rounds under the moment conditions; the literals give at most
    2.4e-13."""
    print(f"moment {q}: {_moment(q):.3e}")
    assert abs(_moment(q)) <= 1e-12


def test_db8_literals_stay_beside_the_derivation():
    """every literal is a float64 at most db8_taps.MAX_STEPS units in the last place from the nearest one to the derived tap; the nearest
    ones themselves miss the seventh moment's bound, which is why the tool moves any"""
    nearest = np.asarray(db8_taps.derive(), dtype=np.float64)
    steps = (P - nearest) / np.array([math.ulp(v) for v in nearest])
    assert np.array_equal(steps, np.round(steps)) and np.abs(steps).max() <= db8_taps.MAX_STEPS == 2
    assert np.abs(db8_taps.moments(nearest)).max() > 1e-12 >= 4 * np.abs(db8_taps.moments(P)).max()
    assert np.array_equal(db8_taps.moments(P), [_moment(q) for q in range(8)])


def test_db8_is_minimum_phase():
    roots = np.roots(P)
    near = np.abs(roots + 1.0) < 0.2                                        # the eightfold zero at -1 spreads into a small circle
    assert near.sum() == 8 and (np.abs(roots[~near]) < 1.0).all() and (~near).sum() == 7


def test_db8_is_what_the_tool_derives_and_what_the_kernel_holds():
    assert np.abs(db8_taps.taps() - P).max() <= 1e-13
    src = (ROOT / "ws_unet_amd" / "csrc" / "wavelet_cost.hip").read_text()
    body = re.search(r"constexpr double DB8\[16\] = \{(.*?)\};", src, flags=re.S).group(1)
    kernel = [t.strip() for t in body.split(",")]
    module = re.search(r"^DB8 = \((.*?)\)", (ROOT / "ws_unet_amd" / "costs.py").read_text(), flags=re.S | re.M).group(1)
    assert kernel == [t.strip() for t in module.split(",")] and [float(t) for t in kernel] == list(costs.DB8)
    assert all(len(t.lstrip("-").replace(".", "").lstrip("0")) == 17 for t in kernel)          # 17 significant digits
    assert np.array_equal(costs_np.L, P[::-1]) and costs_np.H[0] == -P[0] and costs_np.H[1] == P[1] and costs_np.H[15] == P[15]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("suniward", "wow"))
def test_the_separable_form_is_the_direct_definition(kind):
    shape = (33, 31)
    x = costs_np.plane("noise", *shape)
    rho = costs_np.cost(x, kind)
    rng = np.random.default_rng(48)
    pixels = [(0, 0), (0, 30), (32, 0), (32, 30), (16, 0), (0, 15)] + [(int(rng.integers(33)), int(rng.integers(31))) for _ in range(14)]
    for i, j in pixels:
        want = costs_np.direct_cost_at(x, i, j, kind)
        assert abs(rho[i, j] - want) <= 1e-12 * abs(want), (i, j, rho[i, j], want)


def _uniward_distortion(x, i, j, sigma):
    """D(X, X + e_ij) = sum_k sum_{m,n} |W_k(Y) - W_k(X)| / (sigma + |W_k(X)|) over the whole range of the restatement's transform"""
    y = x.copy()
    assert y[i, j] < 255
    y[i, j] += 1
    return sum(float((np.abs(wy - wx) / (np.float64(sigma) + np.abs(wx))).sum()) for wx, wy in zip(costs_np.forward(x), costs_np.forward(y)))


def test_the_cost_is_uniwards_distortion_of_one_change():
    """48 x 48 and 16 <= i, j < 32: nearer than 16 to a border a pixel meets its own mirror image in the padding.  A back-projection
    index shifted by one in either direction breaks the identity."""
    x = np.minimum(costs_np.plane("noise", 48, 48), 254)
    for sigma in (1.0, 0.25):
        rho = costs_np.cost(x, "suniward", sigma=sigma)
        shifted = [costs_np.cost(x, "suniward", sigma=sigma, di=di, dj=dj) for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1))]
        worst = 0.0
        for i, j in [(16, 16), (16, 31), (31, 16), (31, 31), (23, 24), (20, 29), (27, 17)]:
            d = _uniward_distortion(x, i, j, sigma)
            worst = max(worst, abs(rho[i, j] - d) / d)
            assert abs(rho[i, j] - d) <= 1e-12 * d, (sigma, i, j, rho[i, j], d)
            for s in shifted:
                assert abs(s[i, j] - d) > 1e-6 * d, (sigma, i, j)
        print(f"sigma {sigma}: largest relative difference between rho and D(X, X + e) {worst:.3e} (bound 1e-12)")


def test_a_flat_plane():
    x = costs_np.plane("flat", 24, 40)
    wow = costs_np.cost(x, "wow")
    assert (wow == 1e10).all()                                              # every W is 0: xi = 0, 1 / 0 = inf, clamped
    assert (costs_np.cost(x, "wow", clamp=5.0) == 5.0).all()
    su = costs_np.cost(x, "suniward")
    a1 = np.abs(P).sum()
    assert np.abs(su - 3 * a1 * a1).max() <= 1e-12 * 3 * a1 * a1            # g = 1 / sigma everywhere: xi_k = (sum |p|)^2
    assert abs(su[0, 0] - 13.8362623173) < 1e-9 and np.ptp(su) <= 1e-13
    assert np.abs(costs_np.cost(x, "suniward", sigma=4.0) - su / 4).max() <= 1e-13


def test_photo_costs_are_inside_the_clamp():
    x = costs_np.golden_cover(6)
    su = costs_np.cost(x, "suniward")
    assert su.shape == x.shape and su.dtype == np.float64 and (su > 0).all() and (su < 1e8).all()
    assert 0.1 < su.min() and su.max() < 3 * np.abs(P).sum() ** 2 + 1e-9     # g <= 1 / sigma
    wow = costs_np.cost(x, "wow")
    assert (wow > 0).all() and np.isfinite(wow).all()
    print(f"cover 6: S-UNIWARD {su.min():.3g} .. {su.max():.3g}, median {np.median(su):.3g}; "
          f"WOW {wow.min():.3g} .. {wow.max():.3g}, {(wow == 1e10).sum()} clamped")
    # the small shapes that fold several times are defined and finite
    for shape in ((3, 5), (8, 16), (1, 1)):
        r = costs_np.cost(costs_np.plane("noise", *shape), "suniward")
        assert r.shape == shape and np.isfinite(r).all() and (r > 0).all()


# ---- names ------------------------------------------------------------------------------------------------------------------------------

def test_methods_names_and_folders():
    assert costs.COSTS == ("HILL", "SUNIWARD", "WOW") and costs.METHODS == ("SUNIWARD", "WOW", "SUNIWARDT", "WOWT")
    assert [costs.method_name(m) for m in ("suniward", "Wow", "suniwardt", "WOWT")] == list(costs.METHODS)
    assert [costs.method_cost(m) for m in costs.METHODS] == ["SUNIWARD", "WOW", "SUNIWARD", "WOW"]
    assert costs.cost_name("hill") == "HILL"
    for bad in ("HILL", "STCT", "UNIWARD", ""):
        with pytest.raises(NotImplementedError, match="SUNIWARD / WOW / SUNIWARDT / WOWT"):
            costs.method_name(bad)
    with pytest.raises(NotImplementedError, match="HILL / SUNIWARD / WOW"):
        costs.cost_name("MiPOD")
    assert costs.folder_name("wowt", 0.4) == "stego_WOWT_alpha_0.4_independent_images"
    assert costs.folder_name("SUNIWARD", 0.2) == "stego_SUNIWARD_alpha_0.2_independent_images"
    # the older modules keep their methods and refuse the new names
    assert embed.METHODS == ("LSBR", "HILLR", "LSBRS", "LSBRK", "HILLRM") and embed_pm1.METHODS == ("LSBM", "HILL")
    assert stc.METHODS == ("STCR", "STCM") and stc_ml.METHODS == ("STCT",)
    for mod in (embed, embed_pm1, stc, stc_ml):
        for m in costs.METHODS:
            with pytest.raises(NotImplementedError):
                mod.method_name(m)
    with pytest.raises(ValueError, match="takes no message"):
        costs.write_dataset("nowhere", "WOW", message=b"abc")
    with pytest.raises(NotImplementedError, match="hold no message"):
        costs.extract_dataset("nowhere", "SUNIWARD", 0.4, "out")
    with pytest.raises(ValueError, match=r"alpha outside \(0, log2 3\)"):
        costs.write_dataset("nowhere", "WOWT", 0.0)
    with pytest.raises(ValueError, match=r"alpha outside \[0, log2 3\) for 'WOW'"):
        costs.write_dataset("nowhere", "WOW", 1.6)


def test_the_entry_validates_before_any_gpu_call(lib):
    """errno-style code + message naming the argument, with no GPU present"""
    f = lib.wsu_wavelet_cost_f64
    assert f(None, 16, 0, 1.0, 1e8, 1, 8, 8, None) == -1 and b"wavelet_cost_f64: null" in lib.wsu_last_error()
    assert f(16, None, 0, 1.0, 1e8, 1, 8, 8, None) == -1 and b"wavelet_cost_f64: null" in lib.wsu_last_error()
    for kind in (-1, 2):
        assert f(16, 16, kind, 1.0, 1e8, 1, 8, 8, None) == -1 and b"kind=%d" % kind in lib.wsu_last_error()
    for sigma in (0.0, -1.0, math.inf, math.nan):
        assert f(16, 16, 0, sigma, 1e8, 1, 8, 8, None) == -1 and b"sigma" in lib.wsu_last_error()
    for clamp in (0.0, -1.0, math.inf, math.nan):
        for kind in (0, 1):
            assert f(16, 16, kind, 1.0, clamp, 1, 8, 8, None) == -1 and b"clamp" in lib.wsu_last_error()
    assert f(16, 16, 1, 0.0, 0.0, 1, 8, 8, None) == -1 and b"clamp" in lib.wsu_last_error()       # WOW ignores sigma: the clamp is named
    assert f(16, 16, 0, 1.0, 1e8, 0, 8, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert f(16, 16, 0, 1.0, 1e8, 70000, 8, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert f(16, 16, 1, 1.0, 1e10, 1, 8, 0, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert f(16, 16, 1, 1.0, 1e10, 1, 65536, 65536, None) == -1 and b"32-bit" in lib.wsu_last_error()
