"""CPU: the host side of the sequential-payload WS estimator and of the LSBRS simulator: ws.sequential.payload on numpy and torch inputs,
the names, folders and counts of ws_unet_amd.embed, the option errors of ws.estimate raised up front, the argument errors of the two C
entries (no GPU call is made) and the numpy restatement's own edge cases."""
import ctypes

import numpy as np
import pytest
import torch

import embed_np
import sequential_np
from ws_unet_amd import _lib, embed, filters, ops
from ws_unet_amd.ws import estimate, roc, sequential, structural

ORDERS = ("rows", "rows_up")


# ---- payload() --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("h,w", [(3, 3), (3, 4), (5, 7), (512, 512), (67, 259)])
def test_payload_of_numpy_and_torch_changepoints(h, w, order):
    m = (h - 2) * (w - 2)
    ks = np.unique(np.concatenate([np.arange(0, min(m, 40) + 1), np.arange(max(m - 40, 0), m + 1),
                                   np.random.default_rng(h * w).integers(0, m + 1, 50)])).astype(np.int64)
    want = np.array([sequential_np.payload(int(k), h, w, order) for k in ks])
    got = sequential.payload(ks, h, w, order)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    got_t = sequential.payload(torch.from_numpy(ks), h, w, order)
    assert isinstance(got_t, torch.Tensor) and got_t.dtype == torch.float64
    np.testing.assert_array_equal(got_t.numpy(), want)
    np.testing.assert_array_equal(sequential.beta(ks, h, w, order), want / 2)
    assert got[0] == 0.0 and float(sequential.payload(0, h, w, order)) == 0.0              # k = 0 -> 0
    # k = M: the last interior pixel of the path; top-down that is plane pixel (H-2, W-2), bottom-up (1, W-2) which lies H-2 rows up
    assert got[-1] == ((h - 2) * w + (w - 2) + 1) / (h * w)
    assert float(sequential.payload(1, h, w, order)) == (w + 2) / (h * w)                    # the first interior pixel: one row and one pixel in
    assert (np.diff(got) > 0).all()                                                          # strictly monotone in k
    assert got[-1] < 1.0


def test_payload_counts_positions_on_the_path_over_the_whole_plane():
    h, w = 6, 5
    for order in ORDERS:
        pos = sequential_np.path_positions(h, w, order)
        interior = pos[1:-1, 1:-1] if order == "rows" else pos[1:-1, 1:-1][::-1]
        want = (interior.reshape(-1) + 1) / (h * w)
        np.testing.assert_array_equal(sequential.payload(np.arange(1, 13), h, w, order), want)
    with pytest.raises(ValueError, match="unknown order"):
        sequential.payload(np.arange(3), 6, 5, "columns")
    with pytest.raises(ValueError, match="3 x 3"):
        sequential.payload(np.arange(3), 2, 5)


# ---- embed ------------------------------------------------------------------------------------------------------------------

def test_lsbrs_names_folders_and_counts():
    assert embed.method_name("lsbrs") == "LSBRS" and embed.method_name("LSBrs") == "LSBRS" and "LSBRS" in embed.METHODS
    assert embed.METHODS[:2] == ("LSBR", "HILLR")
    assert embed.folder_name("lsbrs", 0.4) == "stego_LSBRS_alpha_0.4_independent_images"
    assert embed.folder_name("LSBRS", 0.4, "rows") == "stego_LSBRS_alpha_0.4_independent_images"
    assert embed.folder_name("LSBRS", 0.4, "rows_up") == "stego_LSBRS_alpha_0.4_rows_up_independent_images"
    assert embed.folder_name("LSBR", 0.4) == "stego_LSBR_alpha_0.4_independent_images" == embed.folder_name("LSBR", 0.4, "rows_up")
    with pytest.raises(ValueError, match="unknown order"):
        embed.folder_name("LSBRS", 0.4, "columns")
    for h, w in ((512, 512), (67, 259), (1, 1), (3, 5)):
        for alpha, want in ((0.0, 0), (1e-9, 0), (0.3, int(np.floor(0.3 * (h * w)))), (1.0, h * w)):
            assert embed.lsbrs_count(alpha, h, w) == want == sequential_np.lsbrs_count(alpha, h, w)
    assert embed.lsbrs_count(0.3, 512, 512) == 78643
    with pytest.raises(ValueError, match="unknown order"):
        embed.simulate(torch.zeros((1, 4, 4), dtype=torch.uint8), "LSBRS", 0.5, [1], order="columns")
    with pytest.raises(ValueError, match="seed"):
        embed.simulate(torch.zeros((1, 4, 4), dtype=torch.uint8), "LSBRS", 0.5)


def test_pair_loader_rejects_sequential_twins(tmp_path):
    from ws_unet_amd.data.pairs import PairLoader
    with pytest.raises(ValueError, match="LSBRS"):
        PairLoader(tmp_path, None, "LSBRS", 0.4, batch_size=2, simulate=True, device="cuda")
    with pytest.raises(ValueError, match="LSBRS"):
        PairLoader(tmp_path, None, ["LSBR", "lsbrs"], [0.4, 0.2], batch_size=2, simulate=True, device="cuda")


def test_restated_simulator_is_a_prefix_of_the_full_lsbr_twin():
    cover = np.random.default_rng(5).integers(0, 256, (7, 9), dtype=np.uint8)
    seed = (3 << 32) | 12345
    full = embed_np.lsbr_np(cover, 1.0, seed)
    for order in ORDERS:
        np.testing.assert_array_equal(sequential_np.lsbrs_np(cover, 1.0, seed, order), full)
        np.testing.assert_array_equal(sequential_np.lsbrs_np(cover, 0.0, seed, order), cover)
        twin = sequential_np.lsbrs_np(cover, 0.3, seed, order)
        m = sequential_np.lsbrs_count(0.3, 7, 9)
        used = sequential_np.path_positions(7, 9, order) < m
        assert m == 18 and used.sum() == m
        np.testing.assert_array_equal(twin[used], full[used])
        np.testing.assert_array_equal(twin[~used], cover[~used])
    assert (sequential_np.path_positions(7, 9, "rows_up")[-1] == np.arange(9)).all()


# ---- the restated statistic -------------------------------------------------------------------------------------------------

def test_restated_changepoint_takes_the_first_of_equal_maxima_and_the_empty_prefix():
    one = 1 << 24
    q = np.array([[one, -one, one, -one]], dtype=np.int64)
    assert sequential_np.changepoint(q)[:3] == (1, one, 0)
    assert sequential_np.changepoint(-q)[:3] == (0, 0, 0)
    assert sequential_np.changepoint(np.zeros((2, 3), dtype=np.int64))[:3] == (0, 0, 0)
    q2 = np.array([[-one, -one], [one, one]], dtype=np.int64)
    k, t_max, t_all, curve = sequential_np.changepoint(q2, "rows")
    assert (k, t_max, t_all) == (0, 0, 0) and curve.tolist() == [-2 * one, 0]
    k, t_max, t_all, curve = sequential_np.changepoint(q2, "rows_up")
    assert (k, t_max, t_all) == (2, 2 * one, 0) and curve.tolist() == [2 * one, 0]


def test_restated_terms_on_a_prediction_with_nan_inf_and_a_huge_value():
    x = np.full((3, 6), 100, dtype=np.uint8)
    hat = np.array([[np.nan, np.inf, -np.inf, 1e30]], dtype=np.float32)
    q = sequential_np.ws_terms(x, x_hat=hat, hat_scale=1.0, weighted=0)
    assert q.tolist() == [[0, 4096 << 24, -(4096 << 24), 4096 << 24]]                  # x even: s = -1, t = -(100 - hat) - 1/4
    exact = sequential_np.ws_terms(x, x_hat=np.full((1, 4), 101.25, dtype=np.float32), hat_scale=1.0, weighted=0)
    assert exact.tolist() == [[1 << 24] * 4]


# ---- option errors, raised up front -----------------------------------------------------------------------------------------

def test_estimate_rejects_what_the_sequential_statistic_does_not_have(tmp_path):
    kb = filters.get_filter_estimator(filter_name="KB", flatten=False)
    for name in structural.NAMES:
        with pytest.raises(ValueError, match="structural"):
            estimate.attack("missing.png", (3,), structural.StructuralEstimator(name), weighted=0, placement="sequential")
        with pytest.raises(ValueError, match="structural"):
            estimate.run(tmp_path, "LSBRS", 0.4, name, None, (3,), weighted=0, correct_bias=False, placement="sequential")
        with pytest.raises(ValueError, match="structural"):
            roc.collect_ws_scores(tmp_path, ["LSBRS"], [0.4], ("KB", name), placement="sequential")
    for bad in (dict(weighted=-1), dict(weighted=1, correct_bias=True)):
        with pytest.raises(ValueError, match="weighted 0 or 1 and correct_bias=False"):
            estimate.attack("missing.png", (3,), kb, placement="sequential", **bad)
        with pytest.raises(ValueError, match="weighted 0 or 1 and correct_bias=False"):
            estimate.attack_batch(["missing.png"], [{}], channels=(3,), pixel_estimator=kb, placement="sequential", **bad)
        with pytest.raises(ValueError, match="weighted 0 or 1 and correct_bias=False"):
            estimate.run(tmp_path, "LSBRS", 0.4, "KB", None, (3,), placement="sequential", batched=True, **bad)
    with pytest.raises(ValueError, match="unknown placement"):
        estimate.attack("missing.png", (3,), kb, placement="clustered")
    with pytest.raises(ValueError, match="unknown placement"):
        estimate.run(tmp_path, "LSBRS", 0.4, "KB", None, (3,), placement="clustered")
    with pytest.raises(ValueError, match="unknown order"):
        estimate.attack("missing.png", (3,), kb, placement="sequential", order="columns")
    with pytest.raises(ValueError, match="unknown order"):
        estimate.run(tmp_path, "LSBRS", 0.4, "KB", None, (3,), placement="sequential", order="columns", batched=True)
    with pytest.raises(ValueError, match="unknown order"):
        roc.collect_ws_scores(tmp_path, ["LSBRS"], [0.4], ("KB",), placement="sequential", order="columns")
    assert estimate._placement_tail("random", "rows") == {}
    assert estimate._placement_tail("sequential", "rows_up") == {"placement": "sequential", "order": "rows_up"}


def test_cli_flags():
    a = estimate.parse_args(["--placement", "sequential", "--order", "rows_up"])
    assert (a.placement, a.order) == ("sequential", "rows_up")
    a = estimate.parse_args([])
    assert (a.placement, a.order) == ("random", "rows")
    a = roc.parse_args(["--data", "d", "--out-dir", "o", "--placement", "sequential"])
    assert (a.placement, a.order) == ("sequential", "rows")
    with pytest.raises(SystemExit):
        estimate.parse_args(["--placement", "clustered"])


def test_ops_argument_errors_before_any_device_work():
    x = torch.zeros((1, 8, 8), dtype=torch.uint8)
    kb = filters.NAMED_FILTERS_2D["KB"]
    with pytest.raises(ValueError, match="weighted=-1 is not defined"):
        ops.ws_sequential(x, pixel_filter=kb, weighted=-1)
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_sequential(x, weighted=0)
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_sequential(x, torch.zeros((1, 8, 8)), pixel_filter=kb, weighted=0)
    with pytest.raises(ValueError, match="unknown order"):
        ops.ws_sequential(x, pixel_filter=kb, weighted=0, order="columns")
    with pytest.raises(_lib.WsuError, match="CPU tensor"):
        ops.ws_sequential(x, pixel_filter=kb, weighted=0)
    with pytest.raises(ValueError, match="unknown order"):
        ops.embed_lsbr_seq(x, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), "columns")
    with pytest.raises(_lib.WsuError, match="CPU tensor"):
        ops.embed_lsbr_seq(x, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), "rows")


# ---- the C entries' argument errors: errno-style code + message before any HIP call ------------------------------------------

def _seq(lib, *, x=1, x_hat=1, pf=None, pfs=None, mean=None, weighted=0, order=0, k=1, t_max=1, t_all=1, ws=8, ws_bytes=1 << 40, n=1, h=8, w=8):
    return lib.wsu_ws_sequential(x, x_hat, pf, pfs, mean, 1, 255.0, weighted, order, k, t_max, t_all, None, ws, ws_bytes, n, h, w, None)


def test_c_entries_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.wsu_ws_sequential_workspace_bytes(3, 512) == 3 * 510 * 24
    assert lib.wsu_ws_sequential_workspace_bytes(0, 512) == 0 and lib.wsu_ws_sequential_workspace_bytes(1, 2) == 0
    taps = (ctypes.c_float * 9)(*[0.125] * 9)
    assert _seq(lib, x=None) == -1 and b"null" in lib.wsu_last_error()
    assert _seq(lib, k=None) == -1 and b"null" in lib.wsu_last_error()
    assert _seq(lib, ws=None) == -1 and b"null" in lib.wsu_last_error()
    assert _seq(lib, x_hat=None) == -1 and b"exactly one" in lib.wsu_last_error()
    assert _seq(lib, pf=ctypes.addressof(taps)) == -1 and b"exactly one" in lib.wsu_last_error()
    assert _seq(lib, x_hat=None, pf=ctypes.addressof(taps), pfs=1) == -1 and b"exactly one" in lib.wsu_last_error()
    assert _seq(lib, weighted=-1, mean=ctypes.addressof(taps)) == -1 and b"weighted=-1" in lib.wsu_last_error()
    assert _seq(lib, weighted=2, mean=ctypes.addressof(taps)) == -1 and b"weighted=2" in lib.wsu_last_error()
    assert _seq(lib, weighted=1) == -1 and b"mean_filter" in lib.wsu_last_error()
    assert _seq(lib, order=2) == -1 and b"order=2" in lib.wsu_last_error()
    assert _seq(lib, h=2) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _seq(lib, w=2) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _seq(lib, n=0) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _seq(lib, n=65536) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _seq(lib, h=11588, w=11588) == -1 and b"2^27" in lib.wsu_last_error()          # 11586^2 = 2^27 + 17668
    assert _seq(lib, ws_bytes=6 * 24 - 1) == -1 and b"workspace too small" in lib.wsu_last_error()
    assert _seq(lib, ws=12) == -1 and b"aligned" in lib.wsu_last_error()
    # K28
    e = lib.wsu_embed_lsbr_seq
    assert e(None, 1, 1, 0, 1, 1, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert e(1, 1, None, 0, 1, 1, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert e(1, 1, 1, 2, 1, 1, 1, 8, 8, None) == -1 and b"order=2" in lib.wsu_last_error()
    assert e(1, 1, 1, 0, 1, 1, 1, 0, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert e(1, 1, 1, 1, 1, 1, 1, 65536, 65536, None) == -1 and b"32-bit" in lib.wsu_last_error()
