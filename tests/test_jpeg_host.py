"""CPU: the host half of the JPEG-history predictor (ws_unet_amd/ws/jpeg.py, ops.jpeg_tables), the argument checks of its two C entry
points (no GPU is touched: they fail before any HIP call), and the properties of the arithmetic itself on the five golden covers, through
the numpy restatement jpeg_np that the GPU tests compare the kernels with bit for bit."""
import numpy as np
import pytest

from conftest import GOLDEN
import jpeg_np
from ws_unet_amd import ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import estimate, jpeg

COVERS = (6, 7, 8, 9, 10)
QUALITIES = (30, 50, 75, 85)


@pytest.fixture(scope="module")
def lib():
    return ops._lib.load()


# ---- tables and the rule ------------------------------------------------------------------------------------------------------------

def test_tables_against_hand_checked_entries():
    """T[0][0] = 16, T[0][1] = 11, T[0][2] = 10, T[7][7] = 99, T[4][5] = 109.  q = 1: s = 5000, every entry clips to 255.  q = 49:
    s = 102: (16*102+50)//100 = 16, (11*102+50)//100 = 11, (99*102+50)//100 = 101, (109*102+50)//100 = 111.  q = 50: s = 100, the base
    table.  q = 75: s = 50: 850//100 = 8, 600//100 = 6, 550//100 = 5, 5000//100 = 50, 5500//100 = 55.  q = 100: s = 0, every entry clips to 1."""
    t = ops.jpeg_tables([1, 49, 50, 75, 100])
    assert t.dtype == np.int32 and t.shape == (5, 8, 8)
    assert (t[0] == 255).all() and (t[4] == 1).all()
    pick = lambda k: [int(t[k][0][0]), int(t[k][0][1]), int(t[k][0][2]), int(t[k][7][7]), int(t[k][4][5])]
    assert pick(1) == [16, 11, 10, 101, 111]
    assert pick(2) == [16, 11, 10, 99, 109]
    assert pick(3) == [8, 6, 5, 50, 55]
    np.testing.assert_array_equal(ops.jpeg_tables(np.arange(1, 101)), jpeg_np.tables(range(1, 101)))
    assert ops.jpeg_tables(75).shape == (1, 8, 8)
    for bad in ([0], [101], [50.0], [[50]]):
        with pytest.raises(ValueError, match="1..100"):
            ops.jpeg_tables(bad)


def test_dct_matrix_is_the_kernels_table_and_nearly_orthogonal():
    c = jpeg_np.dct_matrix()
    assert c.dtype == np.int64 and c[0].tolist() == [2896] * 8 and c[1].tolist() == [4017, 3406, 2276, 799, -799, -2276, -3406, -4017]
    # C C^T = 2^26 I up to the rounding of C: every entry is off by at most 1/2, in 8 products with a factor of at most 2^12, on either side
    assert np.abs(c @ c.T - (np.eye(8) * 2 ** 26).astype(np.int64)).max() < 2 * 8 * 2 ** 12 // 2


def test_quality_rule_on_synthetic_rows():
    import torch
    rows = np.array([[9, 9, 3, 9, 1], [9, 9, 9, 9, 9], [4, 0, 0, 0, 0], [5, 5, 5, 5, 4], [2 ** 62, 2 ** 40, 5, 4, 3]], dtype=np.int64)
    want = [3, 0, 1, 5, 4]                               # the LOWEST passing candidate, not the best; none passes -> 0; the bound itself passes
    np.testing.assert_array_equal(jpeg.quality_rule(rows, 4), want)
    got = jpeg.quality_rule(torch.from_numpy(rows), 4)
    assert got.dtype == torch.int64 and got.tolist() == want
    assert [jpeg_np.quality(r, 1, tau=4 / 2 ** 20) for r in rows] == want
    assert jpeg.energy_bound(512, 512) == 2 ** 38 and jpeg.energy_bound(8, 16, 0.5) == 2 ** 26 == jpeg_np.bound(128, 0.5)


def test_the_float_quotient_of_the_energy_kernel_is_exact():
    """K31 divides t = (2 ah + hb + Q) >> 1 by Q as int(float32(t) * (1.f / Q) + 0.002f).  t < 2^11 + 2^7 (|Y| < 2^37); every t below 2^12
    and every Q, in float32 with one rounding per operation."""
    t = np.arange(0, 4096, dtype=np.int64)
    for q in range(1, 256):
        rq = np.float32(1.0) / np.float32(q)
        k = ((t.astype(np.float32) * rq).astype(np.float32) + np.float32(0.002)).astype(np.float32).astype(np.int64)
        np.testing.assert_array_equal(k, t // q, err_msg=f"Q = {q}")


def test_the_32_bit_form_of_the_residual_is_the_definition():
    """(ah, al, hb, lo, S) of jpeg_history.hip against r' = (Y - k D + 2^15) >> 16 on random and edge coefficients"""
    rng = np.random.default_rng(31)
    y = rng.integers(-(1 << 37) + 1, 1 << 37, 400000)
    q = rng.integers(1, 256, y.shape)
    y[:8] = [0, 1, -1, 1 << 25, -(1 << 25), (1 << 25) - 1, -(1 << 25) + 1, (1 << 37) - 1]
    q[:8] = [1, 1, 1, 1, 1, 1, 1, 255]
    d = q << 26
    r = y - jpeg_np.quantise(y, q) * d
    want = (r + (1 << 15)) >> 16
    a = np.abs(y)
    ah, al = a >> 26, a & ((1 << 26) - 1)
    lo = np.where(y >= 0, (al + (1 << 15)) >> 16, ((1 << 15) - al) >> 16)
    s = np.where(y < 0, -1024, 1024)
    k = ((2 * ah + (al >> 25) + q) >> 1) // q
    np.testing.assert_array_equal(s * ah + lo - s * k * q, want)
    assert np.abs(want).max() < 2 ** 18 and (2 * ah + (al >> 25) + q).max() < 2 ** 13


# ---- argument errors of the C entry points -----------------------------------------------------------------------------------------

def test_argument_errors_without_a_gpu(lib):
    ok = np.ones((2, 64), dtype=np.int32)
    tp = ok.ctypes.data
    use = np.ones(2, dtype=np.uint8).ctypes.data
    P = 4096                                             # a well-aligned stand-in for a device pointer: nothing dereferences it
    E, R = lib.wsu_jpeg_energies, lib.wsu_jpeg_predict
    err = lambda: lib.wsu_last_error().decode()
    for args in ((None, tp, 2, P, 1, 8, 8, None), (P, None, 2, P, 1, 8, 8, None), (P, tp, 2, None, 1, 8, 8, None)):
        assert E(*args) == -1 and "null" in err()
    for args in ((None, tp, use, P, P, 2, 8, 8, None), (P, None, use, P, P, 2, 8, 8, None), (P, tp, None, P, P, 2, 8, 8, None),
                 (P, tp, use, None, None, 2, 8, 8, None)):
        assert R(*args) == -1 and "null" in err()
    assert E(P, tp, 2, P, 1, 12, 16, None) == -1 and "h=12" in err() and "w=16" in err()
    assert R(P, tp, use, P, P, 2, 12, 16, None) == -1 and "h=12" in err() and "w=16" in err()
    assert E(P, tp, 2, P, 1, 16, 20, None) == -1 and "w=20" in err()
    assert E(P, tp, 2, P, 1, 0, 8, None) == -1 and "h=0" in err()
    assert E(P, tp, 0, P, 1, 8, 8, None) == -1 and "m=0" in err()
    assert E(P, tp, 2, P, 0, 8, 8, None) == -1 and "n=0" in err()
    assert R(P, tp, use, P, P, 0, 8, 8, None) == -1 and "n=0" in err()
    assert E(P, tp, 2, P, 1, 8192, 8192, None) == -1 and "2^24" in err()       # 2^26 pixels
    assert E(P, tp, 2, P, 1, 4096, 4104, None) == -1 and "2^24" in err()       # one block column past 2^24
    assert R(P, tp, use, P, P, 2, 8192, 8192, None) == -1 and "2^24" in err()
    for value in (0, 256, -3):
        bad = ok.copy()
        bad[1, 63] = value
        assert E(P, bad.ctypes.data, 2, P, 1, 8, 8, None) == -1 and f"is {value}" in err() and "1..255" in err() and "table 1 entry 63" in err()
        assert R(P, bad.ctypes.data, use, P, P, 2, 8, 8, None) == -1 and f"is {value}" in err() and "1..255" in err()
    assert E(P + 4, tp, 2, P, 1, 8, 8, None) == -1 and "aligned" in err()
    assert R(P, tp, use, P + 8, P, 2, 8, 8, None) == -1 and "aligned" in err()


def test_python_argument_errors_without_a_gpu():
    import torch
    with pytest.raises(Exception, match="CPU tensor"):
        ops.jpeg_energies(torch.zeros((1, 8, 8), dtype=torch.uint8), ops.jpeg_tables([50]))
    for est_args in (dict(quality=0), dict(quality=50.0), dict(max_quality=101), dict(fallback="AVG"), dict(tau=0.)):
        with pytest.raises(ValueError):
            jpeg.JPEGEstimator(**est_args)
    est = jpeg.JPEGEstimator()
    assert est.fallbacks == 0 and est.quality is None and est.max_quality == 95 and est.fallback == "KB"
    est.note(np.array([True, False, False]))
    est.note(np.array([False]))
    assert est.fallbacks == 3
    assert isinstance(jpeg.estimator("JPEG"), jpeg.JPEGEstimator) and jpeg.estimator("KB") is None
    with pytest.raises(ValueError, match="correct_bias"):
        estimate._check_options(est, 0, True)
    with pytest.raises(ValueError, match="correct_bias"):
        estimate._check_options(est, 1, True, "sequential", "rows")
    estimate._check_options(est, -1, False)
    estimate._check_options(est, 1, False, "sequential", "rows_up")
    assert estimate._native_planes_ok((3,), est, imread4_u8, None)


# ---- the arithmetic on the golden covers ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def covers():
    return np.stack([np.ascontiguousarray(imread4_u8(GOLDEN / f"cover_{k}.png")[..., 3]) for k in COVERS])


def test_history_and_estimate_of_precompressed_covers(covers):
    """The five golden covers precompressed by the oracle at IJG quality 30 / 50 / 75 / 85, then LSBR at alpha = 0 and 0.4 from numpy's
    generator seeded with 2008: the quality found is within 2 of the truth, and the unweighted WS estimate with the recompression
    predictor at the quality FOUND is within 0.05 of alpha / 2.  Measured with the clamp of the prediction in place: worst |q_hat - q0| = 2
    (q_hat is 30 at 30, 48-49 at 50, 73-74 at 75, 83-84 at 85: the lowest quality that passes, and neighbouring tables differ in few
    entries); worst |beta_hat - alpha / 2| = 0.0158 (cover_9 at quality 85, alpha 0.4), mean 0.0036."""
    rng = np.random.default_rng(2008)
    errs = []
    for q0 in QUALITIES:
        pre = jpeg_np.recompress(covers, q0)
        for alpha in (0, 0.4):
            x = jpeg_np.lsbr(pre, alpha, rng) if alpha else pre
            q_hat = jpeg_np.estimate_quality(x)
            print(f"q0 {q0} alpha {alpha}: q_hat {q_hat.tolist()}")
            assert (q_hat > 0).all() and np.abs(q_hat - q0).max() <= 2, (q0, alpha, q_hat)
            hat, _ = jpeg_np.predict(x, [jpeg_np.table(int(q)) for q in q_hat])
            beta = np.array([jpeg_np.beta_unweighted(x[i], hat[i]) for i in range(len(x))])
            print(f"    beta_hat - alpha / 2 {np.round(beta - alpha / 2, 4).tolist()}")
            assert np.abs(beta - alpha / 2).max() <= 0.05, (q0, alpha, beta)
            errs += np.abs(beta - alpha / 2).tolist()
    print(f"worst |beta_hat - alpha / 2| {max(errs):.4f}, mean {np.mean(errs):.4f}")


def test_raw_covers_show_no_history(covers):
    """never-compressed covers and their alpha = 0.4 twins: no quality up to 95 passes"""
    rng = np.random.default_rng(2008)
    assert jpeg_np.estimate_quality(covers).tolist() == [0] * 5
    assert jpeg_np.estimate_quality(jpeg_np.lsbr(covers, 0.4, rng)).tolist() == [0] * 5
