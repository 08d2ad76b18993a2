"""CPU: the host side of the cost-ordered WS estimator (ws/adaptive.py, K33) and of the HILLRM simulator (K34): adaptive.beta on numpy
and torch inputs, the option errors of ws.estimate / ws.roc raised up front, the names and ranks of ws_unet_amd.embed, the argument
errors of ops and of the C entries (no GPU call is made), and the numpy restatement's own edge cases."""
import ctypes

import numpy as np
import pytest
import torch

import adaptive_np
import embed_np
import sequential_np
from ws_unet_amd import _lib, embed, filters, ops
from ws_unet_amd.ws import adaptive, estimate, roc, sequential, structural


# ---- beta() -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flip_rate", [1.0, 0.5, 0.3])
@pytest.mark.parametrize("h,w", [(3, 3), (5, 7), (512, 512), (70, 300)])
def test_beta_of_numpy_and_torch_changepoints(h, w, flip_rate):
    m = (h - 2) * (w - 2)
    ks = np.unique(np.concatenate([[0, m], np.random.default_rng(h * w).integers(0, m + 1, 50)])).astype(np.int64)
    want = np.array([adaptive_np.beta_np(int(k), h, w, flip_rate) for k in ks])
    got = adaptive.beta(ks, h, w, flip_rate)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    got_t = adaptive.beta(torch.from_numpy(ks), h, w, flip_rate)
    assert isinstance(got_t, torch.Tensor) and got_t.dtype == torch.float64
    np.testing.assert_array_equal(got_t.numpy(), want)
    assert got[0] == 0.0 and got[-1] == flip_rate and float(adaptive.beta(m, h, w, flip_rate)) == flip_rate
    assert float(adaptive.beta(1, h, w)) == 1.0 / m                                          # flip_rate defaults to 1


def test_beta_rejects_bad_arguments():
    with pytest.raises(ValueError, match="flip_rate"):
        adaptive.beta(np.arange(3), 5, 5, 0.0)
    with pytest.raises(ValueError, match="flip_rate"):
        adaptive.beta(np.arange(3), 5, 5, 1.5)
    with pytest.raises(ValueError, match="3 x 3"):
        adaptive.beta(np.arange(3), 2, 5)
    assert adaptive.CRITERIA == ("hill",)
    with pytest.raises(ValueError, match="unknown criterion"):
        adaptive.path_for(torch.zeros((1, 8, 8), dtype=torch.uint8), "wow")


# ---- names ------------------------------------------------------------------------------------------------------------------

def test_placements_and_methods_are_appended():
    assert sequential.PLACEMENTS[-1] == "adaptive" and sequential.PLACEMENTS[:2] == ("random", "sequential")
    assert embed.METHODS[-1] == "HILLRM" and embed.METHODS[:4] == ("LSBR", "HILLR", "LSBRS", "LSBRK")
    assert embed.method_name("hillrm") == "HILLRM" and embed.method_name("HILLrm") == "HILLRM"
    assert embed.method_name("hillr") == "HILLR"
    assert embed.folder_name("hillrm", 0.4) == "stego_HILLRM_alpha_0.4_independent_images" == embed.folder_name("HILLRM", 0.4, "rows_up")
    for h, w in ((512, 512), (67, 259), (1, 1), (3, 5)):
        for alpha in (1e-9, 0.1, 0.3, 1.0):
            assert embed.hillrm_rank(alpha, h, w) == adaptive_np.hillrm_rank(alpha, h, w) == int(np.floor((h * w - 1) * alpha))
        assert embed.hillrm_rank(0.0, h, w) == -1 and embed.hillrm_rank(1.0, h, w) == h * w - 1
    assert embed.hillrm_rank(0.4, 512, 512) == 2 * embed.hillr_rank(0.4, 512, 512) + 1 == 104857
    with pytest.raises(ValueError, match="seed"):
        embed.simulate(torch.zeros((1, 4, 4), dtype=torch.uint8), "HILLRM", 0.5)
    with pytest.raises(ValueError, match="alpha"):
        embed.simulate(torch.zeros((1, 4, 4), dtype=torch.uint8), "HILLRM", 1.5, [1])


def test_pair_loader_rejects_hillrm_twins(tmp_path):
    from ws_unet_amd.data.pairs import PairLoader
    with pytest.raises(ValueError, match="HILLRM"):
        PairLoader(tmp_path, None, "HILLRM", 0.4, batch_size=2, simulate=True, device="cuda")


# ---- the restatement --------------------------------------------------------------------------------------------------------

def test_restated_terms_at_a_quarter_are_the_sequential_ones_and_shift_with_tau():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (9, 12), dtype=np.uint8)
    kb = np.asarray(filters.NAMED_FILTERS_2D["KB"])[..., 0]
    avg = np.asarray(filters.NAMED_FILTERS_2D["AVG"])[..., 0]
    for weighted in (0, 1):
        a = adaptive_np.ordered_terms(x, pixel_kernel=kb, mean_kernel=avg, weighted=weighted, tau=adaptive_np.tau_of(0.5))
        np.testing.assert_array_equal(a, sequential_np.ws_terms(x, pixel_kernel=kb, mean_kernel=avg, weighted=weighted))
    # unweighted, a prediction that makes s * res a multiple of 1/4: the term is exactly r - tau
    xi = x[1:-1, 1:-1]
    s = xi.astype(np.float32) - (xi ^ 1).astype(np.float32)
    hat = (xi.astype(np.float32) - s * np.float32(1.5)).astype(np.float32)
    assert (adaptive_np.ordered_terms(x, x_hat=hat, hat_scale=1., weighted=0, tau=adaptive_np.tau_of(1.0)) == 1 << 24).all()
    assert (adaptive_np.ordered_terms(x, x_hat=hat, hat_scale=1., weighted=0, tau=adaptive_np.tau_of(0.5)) == 5 << 22).all()
    assert adaptive_np.tau_of(1.0) == np.float32(0.5) and adaptive_np.tau_of(0.3) == np.float32(0.15)


def test_restated_changepoint_follows_the_path():
    one = 1 << 24
    q = np.array([[one, -one, one], [-one, one, one]], dtype=np.int64)
    assert adaptive_np.changepoint_along(q, np.arange(6)) == sequential_np.changepoint(q)[:3] == (6, 2 * one, 2 * one)
    assert adaptive_np.changepoint_along(q, [0, 2, 4, 5, 1, 3]) == (4, 4 * one, 2 * one)
    assert adaptive_np.changepoint_along(q, [1, 3, 0, 2, 4, 5]) == (6, 2 * one, 2 * one)
    assert adaptive_np.changepoint_along(q, [0, 1, 2, 3, -1, 6]) == (1, one, 0)             # entries outside 0..M-1 add nothing; first maximum
    assert adaptive_np.changepoint_along(-np.abs(q), np.arange(6)) == (0, 0, -6 * one)
    keys = np.zeros((4, 5), dtype=np.float32)
    keys[1:-1, 1:-1] = [[2, 1, 2], [1, 0, 1]]
    assert adaptive_np.interior_order_np(keys).tolist() == [4, 1, 3, 5, 0, 2] and adaptive_np.interior_order_np(keys).dtype == np.int32


def test_restated_hillrm_is_a_subset_of_hillr_at_twice_the_change_rate():
    cover = np.random.default_rng(8).integers(0, 256, (40, 44), dtype=np.uint8)
    seed = (3 << 32) | 12345
    assert (adaptive_np.hillrm_np(cover, 0.0, seed) == cover).all()
    twin = adaptive_np.hillrm_np(cover, 0.25, seed)
    full = embed_np.lsbr_np(cover, 1.0, seed)
    used = embed_np.hillr_np(cover, 0.5) != cover                                            # HILLR at alpha / 2 = 0.25 flips exactly the used pixels
    assert adaptive_np.hillrm_rank(0.25, 40, 44) == embed_np.hillr_rank(0.5, 40, 44)
    np.testing.assert_array_equal(twin[used], full[used])
    np.testing.assert_array_equal(twin[~used], cover[~used])
    assert ((twin ^ cover) <= 1).all() and 0 < (twin != cover).sum() < used.sum()
    np.testing.assert_array_equal(adaptive_np.hillrm_np(cover, 1.0, seed), full)


# ---- option errors, raised up front -----------------------------------------------------------------------------------------

def test_estimate_rejects_what_the_adaptive_statistic_does_not_have(tmp_path):
    kb = filters.get_filter_estimator(filter_name="KB", flatten=False)
    for name in structural.NAMES:
        with pytest.raises(ValueError, match="structural"):
            estimate.attack("missing.png", (3,), structural.StructuralEstimator(name), weighted=0, placement="adaptive")
        with pytest.raises(ValueError, match="structural"):
            estimate.run(tmp_path, "HILLR", 0.4, name, None, (3,), weighted=0, correct_bias=False, placement="adaptive")
        with pytest.raises(ValueError, match="structural"):
            roc.collect_ws_scores(tmp_path, ["HILLR"], [0.4], ("KB", name), placement="adaptive")
    for bad in (dict(weighted=-1), dict(weighted=1, correct_bias=True)):
        with pytest.raises(ValueError, match="weighted 0 or 1 and correct_bias=False"):
            estimate.attack("missing.png", (3,), kb, placement="adaptive", **bad)
        with pytest.raises(ValueError, match="weighted 0 or 1 and correct_bias=False"):
            estimate.attack_batch(["missing.png"], [{}], channels=(3,), pixel_estimator=kb, placement="adaptive", **bad)
        with pytest.raises(ValueError, match="weighted 0 or 1 and correct_bias=False"):
            estimate.run(tmp_path, "HILLR", 0.4, "KB", None, (3,), placement="adaptive", batched=True, **bad)
    for bad, what in ((dict(criterion="wow"), "unknown criterion"), (dict(flip_rate=0.0), "flip_rate"), (dict(flip_rate=1.01), "flip_rate"),
                      (dict(flip_rate=None), "flip_rate")):
        with pytest.raises(ValueError, match=what):
            estimate.attack("missing.png", (3,), kb, placement="adaptive", **bad)
        with pytest.raises(ValueError, match=what):
            estimate.attack_batch(["missing.png"], [{}], channels=(3,), pixel_estimator=kb, placement="adaptive", **bad)
        with pytest.raises(ValueError, match=what):
            estimate.run(tmp_path, "HILLR", 0.4, "KB", None, (3,), placement="adaptive", **bad)
        with pytest.raises(ValueError, match=what):
            roc.collect_ws_scores(tmp_path, ["HILLR"], [0.4], ("KB",), placement="adaptive", **bad)
    with pytest.raises(ValueError, match="unknown placement"):
        estimate.attack("missing.png", (3,), kb, placement="clustered")
    with pytest.raises(ValueError, match="unknown placement"):
        estimate.run(tmp_path, "HILLR", 0.4, "KB", None, (3,), placement="clustered", criterion="hill")
    with pytest.raises(ValueError, match="unknown placement"):
        roc.collect_ws_scores(tmp_path, ["HILLR"], [0.4], ("KB",), placement="clustered")
    with pytest.raises(ValueError, match="unknown placement"):
        sequential.check_placement("Adaptive", "rows")
    sequential.check_placement("adaptive", "rows")
    assert estimate._placement_tail("random", "rows", "hill", 0.5) == {}
    assert estimate._placement_tail("sequential", "rows_up", "hill", 0.5) == {"placement": "sequential", "order": "rows_up"}
    assert estimate._placement_tail("adaptive", "rows", "hill", 0.5) == {"placement": "adaptive", "criterion": "hill", "flip_rate": 0.5}
    assert list(estimate._placement_tail("adaptive", "rows")) == ["placement", "criterion", "flip_rate"]
    assert {"criterion", "flip_rate"} <= set(estimate._ATTACK_KEYS)


def test_cli_flags():
    a = estimate.parse_args(["--placement", "adaptive", "--flip-rate", "0.5", "--criterion", "hill"])
    assert (a.placement, a.criterion, a.flip_rate) == ("adaptive", "hill", 0.5)
    a = estimate.parse_args(["--placement", "adaptive"])
    assert (a.placement, a.criterion, a.flip_rate, a.order) == ("adaptive", "hill", 1.0, "rows")
    a = estimate.parse_args([])
    assert (a.placement, a.criterion, a.flip_rate) == ("random", "hill", 1.0)
    a = roc.parse_args(["--data", "d", "--out-dir", "o", "--placement", "adaptive", "--flip-rate", "0.5"])
    assert (a.placement, a.criterion, a.flip_rate) == ("adaptive", "hill", 0.5)
    with pytest.raises(SystemExit):
        estimate.parse_args(["--placement", "adaptive", "--criterion", "wow"])
    with pytest.raises(SystemExit):
        roc.parse_args(["--data", "d", "--out-dir", "o", "--placement", "clustered"])


def test_ops_argument_errors_before_any_device_work():
    x = torch.zeros((1, 8, 8), dtype=torch.uint8)
    path = torch.zeros((1, 36), dtype=torch.int32)
    kb = filters.NAMED_FILTERS_2D["KB"]
    with pytest.raises(ValueError, match="weighted=-1 is not defined"):
        ops.ws_ordered(x, path, pixel_filter=kb, weighted=-1)
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_ordered(x, path, weighted=0)
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_ordered(x, path, torch.zeros((1, 8, 8)), pixel_filter=kb, weighted=0)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="flip_rate"):
            ops.ws_ordered(x, path, pixel_filter=kb, weighted=0, flip_rate=bad)
    with pytest.raises(_lib.WsuError, match="CPU tensor"):
        ops.ws_ordered(x, path, pixel_filter=kb, weighted=0)
    with pytest.raises(ValueError, match="float32"):
        ops.interior_order(torch.zeros((1, 8, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        ops.interior_order(torch.zeros((1, 2, 8), dtype=torch.float32))
    with pytest.raises(_lib.WsuError, match="CPU tensor"):
        ops.interior_order(torch.zeros((1, 8, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="terms must be"):
        ops.ws_ordered_fold(torch.zeros((1, 35), dtype=torch.int64), path, 8, 8)


# ---- the C entries' argument errors: errno-style code + message before any HIP call ------------------------------------------

def _ord(lib, *, x=1, x_hat=1, pf=None, pfs=None, mean=None, weighted=0, tau=0.5, path=4, k=1, t_max=1, t_all=1, ws=8, ws_bytes=1 << 40,
         n=1, h=8, w=8):
    return lib.wsu_ws_ordered(x, x_hat, pf, pfs, mean, 1, 255.0, weighted, tau, path, k, t_max, t_all, ws, ws_bytes, n, h, w, None)


def test_c_entries_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    m = 510 * 510
    chunks = (m + 2047) // 2048
    assert lib.wsu_ws_ordered_fold_workspace_bytes(3, 512, 512) == 3 * chunks * 24
    assert lib.wsu_ws_ordered_workspace_bytes(3, 512, 512) == 3 * m * 8 + 3 * chunks * 24
    assert lib.wsu_ws_ordered_workspace_bytes(1, 3, 3) == 8 + 24
    for bad in ((0, 512, 512), (1, 2, 512), (1, 512, 2)):
        assert lib.wsu_ws_ordered_workspace_bytes(*bad) == 0 and lib.wsu_ws_ordered_fold_workspace_bytes(*bad) == 0
    taps = (ctypes.c_float * 9)(*[0.125] * 9)
    assert _ord(lib, x=None) == -1 and b"null" in lib.wsu_last_error()
    assert _ord(lib, path=None) == -1 and b"null" in lib.wsu_last_error()
    assert _ord(lib, k=None) == -1 and b"null" in lib.wsu_last_error()
    assert _ord(lib, ws=None) == -1 and b"null" in lib.wsu_last_error()
    assert _ord(lib, x_hat=None) == -1 and b"exactly one" in lib.wsu_last_error()
    assert _ord(lib, pf=ctypes.addressof(taps)) == -1 and b"exactly one" in lib.wsu_last_error()
    assert _ord(lib, x_hat=None, pf=ctypes.addressof(taps), pfs=1) == -1 and b"exactly one" in lib.wsu_last_error()
    assert _ord(lib, weighted=-1, mean=ctypes.addressof(taps)) == -1 and b"weighted=-1" in lib.wsu_last_error()
    assert _ord(lib, weighted=2, mean=ctypes.addressof(taps)) == -1 and b"weighted=2" in lib.wsu_last_error()
    assert _ord(lib, weighted=1) == -1 and b"mean_filter" in lib.wsu_last_error()
    for tau in (0.0, -0.25, 0.5000001, float("nan")):
        assert _ord(lib, tau=tau) == -1 and b"tau=" in lib.wsu_last_error()
    assert _ord(lib, h=2) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _ord(lib, w=2) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _ord(lib, n=0) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _ord(lib, n=65536) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _ord(lib, h=11588, w=11588) == -1 and b"2^27" in lib.wsu_last_error()          # 11586^2 = 2^27 + 17668
    assert _ord(lib, ws_bytes=36 * 8 + 24 - 1) == -1 and b"workspace too small" in lib.wsu_last_error()
    assert _ord(lib, ws=12) == -1 and b"aligned" in lib.wsu_last_error()
    f = lib.wsu_ws_ordered_fold
    assert f(None, 4, 1, 1, 1, 8, 24, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert f(8, None, 1, 1, 1, 8, 24, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert f(8, 4, 1, 1, 1, 8, 23, 1, 8, 8, None) == -1 and b"workspace too small" in lib.wsu_last_error()
    assert f(8, 6, 1, 1, 1, 8, 24, 1, 8, 8, None) == -1 and b"aligned" in lib.wsu_last_error()
    assert f(8, 4, 1, 1, 1, 8, 24, 1, 2, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    t = lib.wsu_ws_ordered_terms
    assert t(1, 1, None, None, None, 1, 255.0, 0, 0.5, None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert t(1, 1, None, None, None, 1, 255.0, 0, 0.5, 12, 1, 8, 8, None) == -1 and b"aligned" in lib.wsu_last_error()
    # K34
    e = lib.wsu_embed_threshold_lsbr
    assert e(None, 1, 1, 1, 1, 1, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert e(1, 1, 1, None, 1, 1, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert e(1, 1, 1, 1, 1, 1, 1, 0, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert e(1, 1, 1, 1, 1, 1, 1, 65536, 65536, None) == -1 and b"32-bit" in lib.wsu_last_error()
