"""CPU: the payload solves of the structural estimators (ws_unet_amd.ws.structural.spa / rs) against the numpy restatement
(structural_np), on hand-checkable tables, random tables, every NaN rule, and the fixture covers with their LSBR twins."""
import math

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import structural_np
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import structural

COVERS = (6, 7, 8, 9, 10)
ALPHAS = ("0.01", "0.05", "0.1")


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


# ---- tables one can check by hand -----------------------------------------------------------------------------------------------

def test_one_pair():
    t = structural_np.spa_table(np.array([[3, 4]], dtype=np.uint8))
    want = np.zeros((3, 128), dtype=np.int64)
    want[1, 0] = 1                                              # d = 1, the larger value 4 is even: X[0]
    np.testing.assert_array_equal(t, want)
    assert math.isnan(structural.spa(t)) and math.isnan(structural_np.spa_p(t))


def test_constant_plane():
    t = structural_np.spa_table(np.full((8, 8), 77, dtype=np.uint8))
    want = np.zeros((3, 128), dtype=np.int64)
    want[0, 0] = 8 * 7 + 7 * 8
    np.testing.assert_array_equal(t, want)
    assert structural.spa(t) == 0. and structural_np.spa_p(t) == 0.


def test_checkerboard():
    x = (np.indices((6, 6)).sum(axis=0) % 2 * 255).astype(np.uint8)
    t = structural_np.spa_table(x)
    want = np.zeros((3, 128), dtype=np.int64)
    want[2, 127] = 6 * 5 + 5 * 6                                 # d = 255, the larger value 255 is odd: Y[127]
    np.testing.assert_array_equal(t, want)
    assert math.isnan(structural.spa(t)) and math.isnan(structural.spa(t, j=127))


def test_rs_counts_of_one_group_by_hand():
    # F1 swaps 2k <-> 2k+1, F-1 swaps 2k-1 <-> 2k.  The fifth column belongs to no group.
    # G = (10, 11, 13, 13): f = 1 + 2 + 0 = 3.  F1 on g1, g2: (10, 10, 12, 13): f = 0 + 2 + 1 = 3.  F-1: (10, 12, 14, 13): f = 2 + 2 + 1 = 5 -> R_-M.
    # G ^ 1 = (11, 10, 12, 12): f = 1 + 2 + 0 = 3.  F1: (11, 11, 13, 12): f = 0 + 2 + 1 = 3.  F-1: (11, 9, 11, 12): f = 2 + 2 + 1 = 5 -> R_-M.
    np.testing.assert_array_equal(structural_np.rs_counts(np.array([[10, 11, 13, 13, 200]], dtype=np.uint8)), [0, 0, 1, 0, 0, 0, 1, 0])
    # F-1 leaves 0..255: G = (0, 0, 255, 255): f = 255; F-1: (0, -1, 256, 255): f = 1 + 257 + 1 = 259 -> R_-M; F1: (0, 1, 254, 255): f = 255.
    np.testing.assert_array_equal(structural_np.rs_counts(np.array([[0, 0, 255, 255]], dtype=np.uint8))[:4], [0, 0, 1, 0])
    np.testing.assert_array_equal(structural_np.rs_counts(np.zeros((2, 3), dtype=np.uint8)), np.zeros(8, dtype=np.int64))


# ---- the solves against the restatement ---------------------------------------------------------------------------------------------

def _random_tables(rng, n):
    """tables shaped like an image's: counts falling off with m, X and Y close to each other"""
    scale = 2e5 * np.exp(-np.arange(128) / rng.uniform(2., 20., (n, 1, 1)))
    return rng.poisson(scale * rng.uniform(.5, 1.5, (n, 3, 1))).astype(np.int64)


def _assert_close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 1e-9), np.abs(got[ok] - want[ok]).max()


@pytest.mark.parametrize("j", [0, 30, 126, 127])
def test_spa_equals_the_restatement_on_random_tables(j):
    t = _random_tables(np.random.default_rng(j), 200)
    want = [structural_np.spa_p(ti, j) for ti in t]
    assert np.isfinite(want).sum() > 100
    got = structural.spa(t, j)
    assert got.dtype == np.float64 and got.shape == (200,)
    _assert_close(got, want)
    dev = structural.spa(torch.from_numpy(t), j)                 # the same function on tensors
    assert dev.dtype == torch.float64
    _assert_close(dev.numpy(), want)


def test_rs_equals_the_restatement_on_random_counts():
    rng = np.random.default_rng(5)
    c = rng.integers(0, 30000, (300, 8)).astype(np.int64)
    c[:100] = rng.integers(20000, 21000, (100, 8))              # near-equal counts: small coefficients, negative discriminants
    want = [structural_np.rs_p(ci) for ci in c]
    assert 50 < np.isfinite(want).sum() and np.isnan(want).sum() > 0
    got = structural.rs(c)
    assert got.dtype == np.float64 and got.shape == (300,)
    _assert_close(got, want)
    _assert_close(structural.rs(torch.from_numpy(c)).numpy(), want)


def test_nan_rules():
    """with j = 30: a = (2 (E0 + Y0) - (E31 + Y31 + X30)) / 4, b = -(2 E0 - E31 + 2 s) / 2, c = s = sum_{m <= 30} (Y[m] - X[m])"""
    t = np.zeros((3, 128), dtype=np.int64)
    t[0, 0], t[0, 31], t[2, 5] = 10, 20, 3                      # 2 C_0 = C_31 = 20: the leading coefficient is 0
    assert math.isnan(structural.spa(t)) and math.isnan(structural_np.spa_p(t))
    assert np.isfinite(structural.spa(t, j=29))                  # a = 5, b = -13, c = 3
    t = np.zeros((3, 128), dtype=np.int64)
    t[2, 0], t[1, 0] = 4000, 3990                                # a = 2000, b = -10, c = 10: discriminant 100 - 80 000
    assert math.isnan(structural.spa(t)) and math.isnan(structural_np.spa_p(t))
    t[0, 0] = 100000                                             # a = 52 000, b = -100 010, c = 10: two real roots
    assert 0 < structural.spa(t) < 1e-3 and structural.spa(t) == pytest.approx(structural_np.spa_p(t), abs=1e-9)
    np.testing.assert_array_equal(np.isnan(structural.spa(np.stack([t, 0 * t]))), [False, True])        # per table, not per batch
    # RS: a = 2 (d1 + d0), b = d-0 - d-1 - d1 - 3 d0, c = d0 - d-0
    assert math.isnan(structural.rs(np.array([5, 5, 9, 1, 7, 7, 3, 2])))                                # d0 = d1 = 0: a = 0
    c = np.array([2, 0, 0, 0, 2, 0, 0, 8])                       # d0 = 2, d-0 = 0, d1 = 2, d-1 = -8: 8 z^2 + 0 z + 2
    assert math.isnan(structural.rs(c)) and math.isnan(structural_np.rs_p(c))
    c = np.array([1, 0, 0, 0, 0, 0, 0, 0])                       # d0 = 1: 2 z^2 - 3 z + 1, roots 1/2 and 1: z = 1/2 has no p
    assert math.isnan(structural.rs(c)) and math.isnan(structural_np.rs_p(c))
    c = np.array([0, 0, 0, 0, 2, 0, 0, 1])                       # d1 = 2, d-1 = -1: 4 z^2 - z, roots 0 and 1/4: p = 0
    assert structural.rs(c) == 0. and structural_np.rs_p(c) == 0.
    np.testing.assert_array_equal(np.isnan(structural.rs(torch.tensor([[1, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 2, 0, 0, 1]])).numpy()), [True, False])


def test_j_bounds_and_shapes():
    t = _random_tables(np.random.default_rng(9), 6)
    for bad in (-1, 128):
        with pytest.raises(ValueError, match="0..127"):
            structural.spa(t, j=bad)
        with pytest.raises(ValueError, match="0..127"):
            structural.StructuralEstimator("SPA", j=bad)
    with pytest.raises(ValueError, match="3,128"):
        structural.spa(t[:, :2])
    with pytest.raises(ValueError, match="8"):
        structural.rs(np.zeros((4, 7), dtype=np.int64))
    with pytest.raises(ValueError, match="unknown structural"):
        structural.StructuralEstimator("WS")
    flat = structural.spa(t)
    np.testing.assert_array_equal(structural.spa(t.reshape(2, 3, 3, 128)), flat.reshape(2, 3))
    assert np.shape(structural.spa(t[0])) == () and structural.spa(t[0]) == flat[0]
    c = np.random.default_rng(1).integers(0, 1000, (2, 3, 8))
    np.testing.assert_array_equal(structural.rs(c), structural.rs(c.reshape(6, 8)).reshape(2, 3))
    assert structural.NAMES == ("SPA", "RS")
    with pytest.raises(ValueError, match="weighted=0"):
        structural.require_unweighted(1, False)
    with pytest.raises(ValueError, match="weighted=0"):
        structural.require_unweighted(0, True)


def test_entry_points_reject_bad_arguments_before_any_device_call():
    from ws_unet_amd import _lib
    lib = _lib.load()
    for entry in (lib.wsu_spa_tables, lib.wsu_rs_counts):
        assert entry(None, 1, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
        assert entry(1, None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
        for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
            assert entry(1, 1, n, h, w, None) == -1 and b"bad shape" in lib.wsu_last_error()


# ---- the formulas on images --------------------------------------------------------------------------------------------------

def test_estimates_on_the_fixture_covers_and_their_lsbr_twins():
    """A sanity bound on the formulas, not a claim about the estimators: |p - alpha| <= 0.03 for the five covers and their LSBR twins at
    0.01, 0.05 and 0.1, SPA with j = 30 and j = 127 and RS, 60 estimates.  Measured with numpy: worst 0.0181 (SPA), 0.0207 (RS); the
    bound is that plus half again.  (The alpha = 1.0 twins are outside the methods' range: SPA is NaN for four of the five.)"""
    worst = {}
    for k in COVERS:
        for alpha in (None,) + ALPHAS:
            x = _plane(f"cover_{k}.png" if alpha is None else f"stego_LSBR_{alpha}_{k}.png")
            t, c = structural_np.spa_table(x), structural_np.rs_counts(x)
            for name, p in (("SPA j=30", structural.spa(t, 30)), ("SPA j=127", structural.spa(t, 127)), ("RS", structural.rs(c))):
                err = abs(float(p) - float(alpha or 0.))
                print(f"cover {k} alpha {alpha or 0} {name}: p = {float(p):.4f}")
                assert not math.isnan(float(p)) and err <= 0.03, (k, alpha, name, float(p))
                worst[name] = max(worst.get(name, 0.), err)
    print("worst |p - alpha|:", worst)
    assert len(worst) == 3


def test_trace_set_identity_on_a_cover():
    """C_m = E[m] + Y[m] + X[m-1] against a direct count of the pairs whose halves differ by m"""
    x = _plane("cover_6.png").astype(np.int64)
    t = structural_np.spa_table(x)
    u = np.concatenate([x[:, :-1].reshape(-1), x[:-1, :].reshape(-1)]) >> 1
    v = np.concatenate([x[:, 1:].reshape(-1), x[1:, :].reshape(-1)]) >> 1
    direct = np.bincount(np.abs(u - v), minlength=129)[:128]
    np.testing.assert_array_equal(t[0] + t[2] + np.concatenate([[0], t[1][:-1]]), direct)
    assert t.sum() == 2 * 512 * 511
