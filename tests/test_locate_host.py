"""CPU: the host side of the payload locator and of the LSBRK simulator: the mean, the two decisions and the confusion counts of ws.locate
on numpy arrays against hand counts, the names, folders and thresholds of ws_unet_amd.embed, the validation errors raised up front, the
argument errors of the new C entries (no GPU call is made), the CLI parser and the numpy restatement's own edge cases."""
import ctypes

import numpy as np
import pytest
import torch

import embed_np
import locate_np
from ws_unet_amd import _lib, embed, filters, ops
from ws_unet_amd.ws import estimate, locate, structural

NAN = float("nan")


# ---- the mean, the decisions, the confusion counts --------------------------------------------------------------------------

def test_mean_of_exact_integers_and_nan_without_a_weight():
    num = np.array([[1 << 23, 0, -(1 << 24)], [5, 0, 2 ** 53 - 1]], dtype=np.int64)
    den = np.array([[1 << 32, 1 << 32, 1 << 31], [0, 0, 2 ** 53 - 1]], dtype=np.int64)
    want = np.array([[0.5, 0.0, -2.0], [NAN, NAN, 256.0]])
    for got in (locate.residual_mean(num, den), locate.residual_mean(torch.from_numpy(num), torch.from_numpy(den)).numpy(),
                locate_np.residual_mean(num, den)):
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, want)
    third = locate.residual_mean(np.array([1], dtype=np.int64), np.array([3 << 8], dtype=np.int64))
    assert third[0] == 1.0 / 3.0                                                            # the correctly rounded quotient


def test_decisions_on_hand_made_means():
    mean = np.array([[0.5, NAN, 0.5, 0.25], [0.1, 0.5, 0.3, -0.2]])
    for m in (mean, torch.from_numpy(mean)):
        as_np = (lambda t: t.numpy()) if isinstance(m, torch.Tensor) else (lambda t: t)
        assert as_np(locate.decide(m)).tolist() == [[True, False, True, False], [False, True, True, False]]        # > 1/4, not >=
        assert as_np(locate.decide(m, threshold=0.4)).tolist() == [[True, False, True, False], [False, True, False, False]]
        assert as_np(locate.decide(m, threshold=-1.0)).tolist() == [[True, False, True, True], [True, True, True, True]]
        assert as_np(locate.decide(m, count=0)).sum() == 0
        assert as_np(locate.decide(m, count=1)).tolist() == [[True, False, False, False], [False, False, False, False]]
        assert as_np(locate.decide(m, count=2)).tolist() == [[True, False, True, False], [False, False, False, False]]  # equal means: the smaller index
        assert as_np(locate.decide(m, count=4)).tolist() == [[True, False, True, False], [False, True, True, False]]
        assert as_np(locate.decide(m, count=7)).tolist() == [[True, False, True, True], [True, True, True, True]]
        assert as_np(locate.decide(m, count=8)).tolist() == [[True, False, True, True], [True, True, True, True]]      # the NaN ranks last and is never used
        assert as_np(locate.decide(m, count=99)).sum() == 7
    for count in range(9):
        np.testing.assert_array_equal(locate.decide(mean, count=count), locate_np.decide_count(mean, count))
    np.testing.assert_array_equal(locate.decide(mean), locate_np.decide_threshold(mean))
    with pytest.raises(ValueError, match="not both"):
        locate.decide(mean, threshold=0.25, count=2)
    with pytest.raises(ValueError, match="negative"):
        locate.decide(mean, count=-1)


def test_confusion_counts_on_hand_made_maps():
    used = np.array([[1, 1, 0, 0], [1, 0, 0, 1]], dtype=bool)
    truth = np.array([[1, 0, 0, 1], [1, 1, 0, 0]], dtype=np.uint8)
    want = {"tp": 2, "fp": 2, "tn": 2, "fn": 2, "accuracy": 0.5}
    assert locate.confusion(used, truth) == want == locate_np.confusion(used, truth)
    assert locate.confusion(torch.from_numpy(used), torch.from_numpy(truth)) == want
    assert locate.confusion(truth, truth) == {"tp": 4, "fp": 0, "tn": 4, "fn": 0, "accuracy": 1.0}
    assert locate.confusion(~used, used) == {"tp": 0, "fp": 4, "tn": 0, "fn": 4, "accuracy": 0.0}
    assert all(type(v) is int for k, v in locate.confusion(used, truth).items() if k != "accuracy")
    with pytest.raises(ValueError, match="shape"):
        locate.confusion(used, truth[:1])


# ---- embed: names, folders, thresholds --------------------------------------------------------------------------------------

def test_lsbrk_names_folders_and_thresholds():
    assert embed.method_name("lsbrk") == "LSBRK" and "LSBRK" in embed.METHODS and embed.METHODS[:3] == ("LSBR", "HILLR", "LSBRS")
    assert embed.folder_name("lsbrk", 0.5, placement_key=7) == "stego_LSBRK_alpha_0.5_key_7_independent_images"
    assert embed.folder_name("LSBRK", 0.5, "rows_up", 2 ** 64 - 1) == f"stego_LSBRK_alpha_0.5_key_{2 ** 64 - 1}_independent_images"
    assert embed.folder_name("LSBR", 0.4, placement_key=7) == "stego_LSBR_alpha_0.4_independent_images"      # the other methods have no key
    with pytest.raises(ValueError, match="placement_key"):
        embed.folder_name("LSBRK", 0.5)
    with pytest.raises(ValueError, match="outside"):
        embed.folder_name("LSBRK", 0.5, placement_key=2 ** 64)
    with pytest.raises(ValueError, match="outside"):
        embed.folder_name("LSBRK", 0.5, placement_key=-1)
    for alpha, want in ((0.0, 0), (1.0, 2 ** 32), (2.0 ** -32, 1), (0.5, 2 ** 31), (2.0 ** -33, 0), (1 - 2.0 ** -32, 2 ** 32 - 1)):
        assert ops.lsbr_key_threshold(alpha) == want == locate_np.key_threshold(alpha)
    assert ops.lsbr_key_threshold(0.3) == int(np.floor(0.3 * 2.0 ** 32)) == 1288490188
    for bad in (-0.1, 1.0000001, NAN):
        with pytest.raises(ValueError, match="outside"):
            ops.lsbr_key_threshold(bad)
    cover = torch.zeros((2, 4, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="placement_key"):
        embed.simulate(cover, "LSBRK", 0.5, [1, 2])
    with pytest.raises(ValueError, match="seed"):
        embed.simulate(cover, "LSBRK", 0.5, placement_key=3)
    with pytest.raises(ValueError, match="one alpha"):
        embed.simulate(cover, "LSBRK", [0.5, 0.25], [1, 2], placement_key=3)
    with pytest.raises(_lib.WsuError, match="CPU tensor"):
        embed.simulate(cover, "LSBRK", 0.5, [1, 2], placement_key=3)
    with pytest.raises(ValueError, match="placement_key"):
        embed.write_dataset("nowhere", "LSBRK", 0.5)


def test_restated_keyed_simulator():
    cover = np.random.default_rng(5).integers(0, 256, (7, 9), dtype=np.uint8)
    seed, key = (3 << 32) | 12345, 99
    np.testing.assert_array_equal(locate_np.lsbrk_np(cover, 1.0, seed, key), embed_np.lsbr_np(cover, 1.0, seed))
    np.testing.assert_array_equal(locate_np.lsbrk_np(cover, 0.0, seed, key), cover)
    assert locate_np.key_mask_np(key, 1.0, 7, 9).all() and not locate_np.key_mask_np(key, 0.0, 7, 9).any()
    mask = locate_np.key_mask_np(key, 0.4, 7, 9)
    twin = locate_np.lsbrk_np(cover, 0.4, seed, key)
    full = embed_np.lsbr_np(cover, 1.0, seed)
    np.testing.assert_array_equal(twin[mask == 1], full[mask == 1])
    np.testing.assert_array_equal(twin[mask == 0], cover[mask == 0])
    assert (locate_np.key_mask_np(key, 0.4, 7, 9) <= locate_np.key_mask_np(key, 0.6, 7, 9)).all()      # a larger payload uses a superset
    np.testing.assert_array_equal(locate_np.key_mask_np(seed, 0.5, 7, 9), embed_np.lsbr_np(np.zeros((7, 9), np.uint8), 1.0, seed))


def test_restated_terms_skip_a_nan_and_clamp():
    x = np.full((3, 6), 100, dtype=np.uint8)
    hat = np.array([[np.nan, np.inf, -np.inf, 1e30]], dtype=np.float32)
    q, dq = locate_np.terms(x, x_hat=hat, hat_scale=1.0, weighted=0)
    assert q.tolist() == [[0, 4096 << 24, -(4096 << 24), 4096 << 24]]                      # x even: s = -1, t = -(100 - hat)
    assert dq.tolist() == [[0, 1 << 32, 1 << 32, 1 << 32]]
    avg = np.asarray(filters.NAMED_FILTERS_2D["AVG"])[..., 0]
    q, dq = locate_np.terms(x, x_hat=np.full((1, 4), 100.5, dtype=np.float32), hat_scale=1.0, weighted=1, mean_kernel=avg)
    fifth = np.float32(1) / np.float32(5)                                                  # a constant plane: var = 0
    assert dq.tolist() == [[858993472] * 4] and q.tolist() == [[int(np.rint(np.float64(fifth * np.float32(0.5)) * 2.0 ** 24))] * 4]
    num, den = locate_np.accumulate(np.stack([x, x]), x_hats=[hat, hat], hat_scale=1.0, weighted=0)
    assert num.tolist() == [[0, 8192 << 24, -(8192 << 24), 8192 << 24]] and den.tolist() == [[0, 2 << 32, 2 << 32, 2 << 32]]
    assert np.isnan(locate_np.residual_mean(num, den)[0, 0])


# ---- validation errors, raised before any device work -----------------------------------------------------------------------

def test_ops_argument_errors_before_any_device_work():
    x = torch.zeros((1, 8, 8), dtype=torch.uint8)
    num, den = torch.zeros((6, 6), dtype=torch.int64), torch.zeros((6, 6), dtype=torch.int64)
    kb = filters.NAMED_FILTERS_2D["KB"]
    with pytest.raises(ValueError, match="weighted=-1 is not defined"):
        ops.ws_residual_accumulate(x, num, den, pixel_filter=kb, weighted=-1)
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_residual_accumulate(x, num, den, weighted=0)
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_residual_accumulate(x, num, den, torch.zeros((1, 8, 8)), pixel_filter=kb, weighted=0)
    with pytest.raises(_lib.WsuError, match="CPU tensor"):
        ops.ws_residual_accumulate(x, num, den, pixel_filter=kb, weighted=0)
    for key, thr in ((-1, 0), (2 ** 64, 0), (1, -1), (1, 2 ** 32 + 1)):
        with pytest.raises(ValueError, match="outside"):
            ops.embed_lsbr_keyed(x, torch.zeros(1, dtype=torch.int64), key, thr)
        with pytest.raises(ValueError, match="outside"):
            ops.lsbr_key_mask(key, thr, 8, 8)
    with pytest.raises(ValueError, match="bad shape"):
        ops.lsbr_key_mask(1, 1, 0, 8)
    with pytest.raises(_lib.WsuError, match="CPU tensor"):
        ops.embed_lsbr_keyed(x, torch.zeros(1, dtype=torch.int64), 1, 1)


def test_accumulator_validation_errors():
    kb = filters.get_filter_estimator(filter_name="KB", flatten=False)
    acc = locate.ResidualAccumulator(8, 8, "cpu")                                           # (host tensors: every error below comes before a launch)
    assert acc.images == 0 and acc.num.shape == (6, 6) and acc.den.dtype == torch.int64
    assert np.isnan(acc.mean().numpy()).all() and not acc.used().any() and not acc.used(count=5).any()
    x = torch.zeros((2, 8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="weighted must be 0 or 1"):
        acc.add(x, kb, weighted=-1)
    with pytest.raises(ValueError, match="pixel predictor"):
        acc.add(x, None)
    with pytest.raises(ValueError, match="pixel predictor"):
        acc.add(x, structural.StructuralEstimator("SPA"), weighted=0)
    with pytest.raises(ValueError, match="one size"):
        acc.add(torch.zeros((2, 8, 9), dtype=torch.uint8), kb)
    with pytest.raises(ValueError, match="uint8"):
        acc.add(torch.zeros((2, 8, 8)), kb)
    with pytest.raises(ValueError, match="uint8"):
        acc.add(torch.zeros((8, 8), dtype=torch.uint8), kb)
    with pytest.raises(ValueError, match="host_planes"):
        acc.add(x, lambda plane: plane[1:-1, 1:-1])
    acc.images = locate.MAX_IMAGES - 1
    assert locate.MAX_IMAGES == 65536
    with pytest.raises(ValueError, match="exceed 65536"):
        acc.add(x, kb)
    acc.images = 0
    with pytest.raises(ValueError, match="exceed 65536"):
        acc.add(torch.zeros((65537, 8, 8), dtype=torch.uint8), kb)
    with pytest.raises(_lib.WsuError, match="CPU tensor"):                                 # a valid call gets as far as the kernel's wrapper
        acc.add(x, kb)
    assert acc.images == 0
    with pytest.raises(ValueError, match="3 x 3"):
        locate.ResidualAccumulator(2, 8, "cpu")


def test_run_rejects_what_it_cannot_do(tmp_path):
    with pytest.raises(ValueError, match="only 'LSBRK'"):
        locate.run(tmp_path, "LSBR", 0.5, "KB", None, (3,), key=5)
    with pytest.raises(ValueError, match="only 'LSBRK'"):
        locate.run(tmp_path, "HILLX", 0.5, "KB", None, (3,), key=5)
    with pytest.raises(ValueError, match="only 'LSBRK'"):
        locate.run(tmp_path, None, 0.0, "KB", None, (3,), key=5)
    with pytest.raises(NotImplementedError, match="HILLX"):
        embed.simulate(torch.zeros((1, 4, 4), dtype=torch.uint8), "HILLX", 0.5, [1])
    for name in structural.NAMES:
        with pytest.raises(ValueError, match="structural"):
            locate.run(tmp_path, "LSBRK", 0.5, name, None, (3,))
    with pytest.raises(ValueError, match="weighted must be 0 or 1"):
        locate.run(tmp_path, "LSBRK", 0.5, "KB", None, (3,), weighted=-1)
    with pytest.raises(ValueError, match="positive"):
        locate.run(tmp_path, "LSBRK", 0.5, "KB", None, (3,), at=(0, 3))


def test_one_mapping_from_a_predictor_to_kernel_arguments():
    x = torch.zeros((2, 8, 8), dtype=torch.uint8)
    kb = filters.get_filter_estimator(filter_name="KB", flatten=False)
    kw = estimate.predictor_arguments(x, kb)
    assert list(kw) == ["pixel_filter"]
    np.testing.assert_array_equal(kw["pixel_filter"], np.asarray(kb.kernel)[..., ::-1])
    planes = [np.arange(64, dtype=np.float32).reshape(8, 8, 1), np.ones((8, 8, 1), dtype=np.float32)]
    kw = estimate.predictor_arguments(x, lambda p: p[1:-1, 1:-1] * 2, planes)
    assert list(kw) == ["x_hat", "hat_scale"] and kw["hat_scale"] == 1.0 and kw["x_hat"].shape == (2, 6, 6)
    np.testing.assert_array_equal(kw["x_hat"][0].numpy(), planes[0][1:-1, 1:-1, 0] * 2)
    kw = estimate.predictor_arguments(x, lambda p: p[1:-1, 1:-1] * 2, planes, correct_bias=True)
    assert list(kw) == ["x_hat", "hat_scale", "x_bias"] and kw["x_bias"].shape == (2, 6, 6)
    np.testing.assert_array_equal(kw["x_bias"][1].numpy(), np.full((6, 6), -2.0, dtype=np.float32))    # x = 1: x_bar - x = -1
    with pytest.raises(ValueError, match="returned"):
        estimate.predictor_arguments(x, lambda p: p, planes)


def test_cli_parser():
    a = locate.parse_args(["--data", "d", "--out-dir", "o", "--alpha", ".5"])
    assert (a.data, a.out_dir, a.stego_method, a.alpha, a.filters, a.model_dir, a.losses, a.weighted, a.key, a.at, a.per_image) == (
        "d", "o", "LSBRK", 0.5, ["AVG", "KB"], None, ["l1ws"], 1, None, [], False)
    a = locate.parse_args(["--data", "d", "--stego-method", "LSBRK", "--alpha", ".5", "--filters", "AVG", "KB", "OLSa", "--model-dir", "m",
                           "--losses", "l1ws", "l1", "--key", "18446744073709551615", "--at", "10", "100", "1000", "--out-dir", "o",
                           "--weighted", "0", "--per-image"])
    assert a.filters == ["AVG", "KB", "OLSa"] and a.model_dir == "m" and a.losses == ["l1ws", "l1"] and a.key == 2 ** 64 - 1
    assert a.at == [10, 100, 1000] and a.weighted == 0 and a.per_image
    for bad in (["--data", "d", "--out-dir", "o"], ["--data", "d", "--alpha", ".5"], ["--data", "d", "--out-dir", "o", "--alpha", ".5", "--weighted", "-1"]):
        with pytest.raises(SystemExit):
            locate.parse_args(bad)
    with pytest.raises(ValueError, match="placement_key"):                                 # the embed CLI hands --key on
        embed.main(["--data", "nowhere", "--stego-method", "LSBRK", "--alphas", "0.5"])


# ---- the C entries' argument errors: errno-style code + message before any HIP call ------------------------------------------

def _acc(lib, *, x=1, x_hat=1, pf=None, pfs=None, mean=None, weighted=0, parts=0, num=8, den=8, n=1, h=8, w=8):
    return lib.wsu_ws_residual_accumulate(x, x_hat, pf, pfs, mean, 1, 255.0, weighted, parts, num, den, n, h, w, None)


def test_c_entries_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    taps = (ctypes.c_float * 9)(*[0.125] * 9)
    assert _acc(lib, x=None) == -1 and b"null" in lib.wsu_last_error()
    assert _acc(lib, num=None) == -1 and b"null" in lib.wsu_last_error()
    assert _acc(lib, den=None) == -1 and b"null" in lib.wsu_last_error()
    assert _acc(lib, x_hat=None) == -1 and b"exactly one" in lib.wsu_last_error()
    assert _acc(lib, pf=ctypes.addressof(taps)) == -1 and b"exactly one" in lib.wsu_last_error()
    assert _acc(lib, x_hat=None, pf=ctypes.addressof(taps), pfs=1) == -1 and b"exactly one" in lib.wsu_last_error()
    assert _acc(lib, weighted=-1, mean=ctypes.addressof(taps)) == -1 and b"weighted=-1" in lib.wsu_last_error()
    assert _acc(lib, weighted=2, mean=ctypes.addressof(taps)) == -1 and b"weighted=2" in lib.wsu_last_error()
    assert _acc(lib, weighted=1) == -1 and b"mean_filter" in lib.wsu_last_error()
    assert _acc(lib, h=2) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _acc(lib, w=2) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _acc(lib, n=0) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _acc(lib, n=65536) == -1 and b"bad shape" in lib.wsu_last_error()
    assert _acc(lib, h=46343, w=46343) == -1 and b"2^31" in lib.wsu_last_error()           # 46341^2 = 2^31 + 4633
    assert _acc(lib, parts=-1) == -1 and b"parts=-1" in lib.wsu_last_error()
    assert _acc(lib, parts=65536) == -1 and b"parts=65536" in lib.wsu_last_error()
    assert _acc(lib, num=12) == -1 and b"aligned" in lib.wsu_last_error()
    assert _acc(lib, den=20) == -1 and b"aligned" in lib.wsu_last_error()
    # K30
    e = lib.wsu_embed_lsbr_keyed
    assert e(None, 1, 5, 7, 1, 1, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert e(1, None, 5, 7, 1, 1, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert e(1, 1, 5, 7, None, 1, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert e(1, 1, 5, 7, 1, None, 1, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert e(1, 1, 5, 2 ** 32 + 1, 1, 1, 1, 8, 8, None) == -1 and b"above 2^32" in lib.wsu_last_error()
    assert e(1, 1, 5, 7, 1, 1, 0, 8, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert e(1, 1, 5, 7, 1, 1, 65536, 8, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert e(1, 1, 5, 7, 1, 1, 1, 65536, 65536, None) == -1 and b"32-bit" in lib.wsu_last_error()
    m = lib.wsu_lsbr_key_mask
    assert m(5, 7, None, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert m(5, 2 ** 32 + 1, 1, 8, 8, None) == -1 and b"above 2^32" in lib.wsu_last_error()
    assert m(5, 7, 1, 0, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert m(5, 7, 1, 65536, 65536, None) == -1 and b"32-bit" in lib.wsu_last_error()
