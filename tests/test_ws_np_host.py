"""CPU: tests/ws_np.py, the exact-sum restatement of K11 that tests/test_gpu_ws_attack_edges.py compares the kernel with, against the two
older checkers of the WS estimate: oracle/ws_ref.attack_array (float32 sums) at rel 2e-6 / abs 2e-7, and the reference's own `attack` in
tests/golden/ws_attack.npz at that file's rel 2e-4 / abs 2e-5.  Also ws_np.finish at the values where the clip and a NaN matter."""
import math

import numpy as np
import pytest

import ws_np
from oracle import ws_ref
from ws_unet_amd import filters, formula

K2D = {name: np.asarray(filters.NAMED_FILTERS_2D[name])[..., 0] for name in ("KB", "AVG", "AVG9")}
AVG3 = filters.NAMED_FILTERS_2D["AVG"]


def _planes64():
    cov = formula.synthetic_images(3, 64, 64, seed=51)
    return [cov[0], formula.lsbr_embed(cov[1], 0.4, seed=3), formula.lsbr_embed(cov[2], 1.0, seed=4)]


def cross_mean(x):
    return ((x[:-2, 1:-1] + x[2:, 1:-1] + x[1:-1, :-2] + x[1:-1, 2:]) * np.float32(0.25))[..., :1]


def _close(a, b, rel, abs_):
    return math.isclose(float(a), float(b), rel_tol=rel, abs_tol=abs_)


def _beta(plane, name, weighted, correct_bias, mean="AVG"):
    kw = dict(mean_kernel=K2D[mean], weighted=weighted, correct_bias=correct_bias)
    if name != "cross":
        return ws_np.attack(plane, pixel_kernel=K2D[name], **kw)[0]
    x = plane.astype(np.float32)[..., None]
    xbar = (plane ^ 1).astype(np.float32)[..., None]
    return ws_np.attack(plane, x_hat=cross_mean(x)[..., 0], x_bias=cross_mean(xbar - x)[..., 0], hat_scale=1.0, **kw)[0]


@pytest.mark.parametrize("name", ["KB", "AVG", "cross"])
def test_ws_np_vs_oracle_and_reference_golden(golden, name):
    g = golden["ws_attack"]
    oracle_est = cross_mean if name == "cross" else (lambda x: ws_ref.filter_infere_single(x, filters.NAMED_FILTERS_2D[name]))
    clipped = 0
    for j, (w, cb) in enumerate(g["cfgs"]):
        for i, p in enumerate(_planes64()):
            beta = _beta(p, name, int(w), bool(cb))
            assert beta.dtype == np.float32
            ref = ws_ref.attack_array(p, oracle_est, AVG3, correct_bias=bool(cb), weighted=int(w))
            assert _close(beta, ref, 2e-6, 2e-7), (name, i, w, cb, beta, ref)
            assert _close(beta, g[f"beta64_{name}"][i, j], 2e-4, 2e-5), (name, i, w, cb, beta)
            clipped += beta == 0
    assert 0 < clipped < 18                                      # both sides of the clip occur


def test_ws_np_general_mean_filter(golden):
    g = golden["ws_attack"]
    for i, p in enumerate(_planes64()):
        beta = _beta(p, "KB", 1, False, mean="AVG9")
        ref = ws_ref.attack_array(p, lambda x: ws_ref.filter_infere_single(x, filters.NAMED_FILTERS_2D["KB"]), filters.NAMED_FILTERS_2D["AVG9"])
        assert _close(beta, ref, 2e-6, 2e-7), (i, beta, ref)
        assert _close(beta, g["beta64_KB_meanAVG9"][i], 2e-4, 2e-5), (i, beta)


def test_sums_are_exact_and_terms_float32():
    x = np.random.default_rng(5).integers(0, 256, (9, 11), dtype=np.uint8)
    t = ws_np.terms(x, pixel_kernel=K2D["KB"], mean_kernel=K2D["AVG9"], weighted=1, correct_bias=True)
    s, a = ws_np.sums(t)
    for k in range(3):
        assert t[k].dtype == np.float32 and t[k].shape == (7, 9)
        assert s[k] == math.fsum(float(v) for v in t[k].reshape(-1)) and a[k] == math.fsum(abs(float(v)) for v in t[k].reshape(-1))
        assert abs(s[k]) <= a[k]
    # uniform weights: sw is the number of interior pixels; no bias correction: the bias terms are zeros
    s0, _ = ws_np.sums(ws_np.terms(x, pixel_kernel=K2D["KB"], weighted=0))
    assert s0[0] == 63.0 and s0[2] == 0.0
    # full-frame and interior predictions name the same pixels
    y = np.random.default_rng(6).random((9, 11), dtype=np.float32)
    for ta, tb in zip(ws_np.terms(x, x_hat=y, weighted=0), ws_np.terms(x, x_hat=y[1:-1, 1:-1].copy(), weighted=0)):
        np.testing.assert_array_equal(ta, tb)


def test_finish_clip_and_nan():
    nan, inf = float("nan"), float("inf")
    assert ws_np.finish(4.0, 1.0, 0.0, False) == np.float32(0.25)
    assert ws_np.finish(4.0, -1.0, 0.0, False) == 0.0                         # negative -> 0
    assert ws_np.finish(4.0, -1.0, 8.0, True) == 0.0                          # 0 - 0 * 2
    assert ws_np.finish(4.0, 1.0, 8.0, True) == np.float32(-0.25)             # after the correction a result may be negative: 1/4 - 1/4 * 2
    assert np.isnan(ws_np.finish(4.0, nan, 0.0, False))                        # np.clip(nan, 0, None) is nan
    assert np.isnan(ws_np.finish(4.0, -1.0, nan, True))                        # 0 - 0 * nan
    assert np.isnan(ws_np.finish(4.0, 1.0, nan, True))
    assert ws_np.finish(4.0, inf, 0.0, False) == inf and ws_np.finish(4.0, -inf, 0.0, False) == 0.0
    assert ws_np.finish(4.0, 1.0, nan, False) == np.float32(0.25)              # sc is not read without correct_bias
    for sb in (1.0, -1.0, nan):
        want = np.clip(np.float64(sb) / 4.0, 0, None)
        np.testing.assert_array_equal(ws_np.finish(4.0, sb, 0.0, False), np.float32(want))
