"""CPU: the host side of the +-1 simulators (ws_unet_amd.embed_pm1, K37-K39): names, folders, thresholds and the argument checks of the C
entries (no GPU here), that `embed` is untouched, and the properties of the numpy restatement (pm1_np) on the very inputs and seed of the
GPU comparisons -- among them the precondition that makes a bit-for-bit comparison fair: no draw lies within 4 of a threshold."""
import ctypes

import numpy as np
import pytest

import pm1_np
from ws_unet_amd import embed, embed_pm1

CASES = [(c, s, a) for s in pm1_np.SHAPES for c in pm1_np.CONTENTS for a in pm1_np.ALPHAS]
SHORT = {("ends", (70, 90), 1.0), ("ends", (65, 130), 1.0)}                 # the payload exceeds the capacity: a band of clamp-cost 255s


@pytest.fixture(scope="module")
def lib():
    from ws_unet_amd import _lib
    return _lib.load()


def test_names_and_folders():
    assert embed_pm1.METHODS == ("LSBM", "HILL")
    assert embed_pm1.method_name("lsbm") == "LSBM" and embed_pm1.method_name("Hill") == "HILL"
    for bad in ("HILLR", "LSBR", "WOW"):
        with pytest.raises(NotImplementedError, match="LSBM / HILL"):
            embed_pm1.method_name(bad)
    assert embed_pm1.folder_name("hill", 0.4) == "stego_HILL_alpha_0.4_independent_images"
    assert embed_pm1.folder_name("LSBM", 1) == "stego_LSBM_alpha_1.0_independent_images"
    with pytest.raises(NotImplementedError):
        embed_pm1.folder_name("HILLR", 0.4)
    import ws_unet_amd
    assert ws_unet_amd.embed_pm1 is embed_pm1


def test_embed_is_untouched():
    import torch
    assert embed.METHODS == ("LSBR", "HILLR", "LSBRS", "LSBRK", "HILLRM")
    x = torch.zeros((1, 4, 4), dtype=torch.uint8)
    for name in ("HILL", "LSBM"):
        with pytest.raises(NotImplementedError, match="LSBR / HILLR"):
            embed.simulate(x, name, 0.4, [1])
        with pytest.raises(NotImplementedError):
            embed.folder_name(name, 0.4)


def test_lsbm_threshold(lib):
    from ws_unet_amd import ops
    assert [ops.lsbm_threshold(a) for a in (0.0, 0.01, 0.4, 1.0)] == [0, 10737418, 429496729, 2 ** 30]
    assert [pm1_np.lsbm_threshold(a) for a in (0.0, 0.01, 0.4, 1.0)] == [0, 10737418, 429496729, 2 ** 30]
    t = ctypes.c_uint32(7)
    for bad in (-0.01, 1.0000001, float("nan")):
        assert lib.wsu_lsbm_threshold(bad, ctypes.byref(t)) == -1 and b"outside [0, 1]" in lib.wsu_last_error()
    assert t.value == 7
    assert lib.wsu_lsbm_threshold(0.5, None) == -1 and b"null" in lib.wsu_last_error()
    with pytest.raises(Exception, match="outside"):
        ops.lsbm_threshold(1.5)


def test_entries_validate_before_any_gpu_call(lib):
    """errno-style code + message for null pointers, bad shapes and bad counts, with no GPU present"""
    assert lib.wsu_ternary_entropy_workspace_bytes(0) == 0 and lib.wsu_ternary_entropy_workspace_bytes(3) == 3 * 64 * 16 * 8
    big = 1 << 20
    assert lib.wsu_ternary_entropy(None, None, None, 1, None, None, 0, 1, 8, 8, None) == -1 and b"ternary_entropy: null" in lib.wsu_last_error()
    assert lib.wsu_ternary_entropy(16, 16, 16, 1, 16, 16, big, 0, 8, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_ternary_entropy(16, 16, 16, 1, 16, 16, big, 70000, 8, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_ternary_entropy(16, 16, 16, 1, 16, 16, big, 1, 65536, 65536, None) == -1 and b"32-bit" in lib.wsu_last_error()
    for l in (0, 17, -1):
        assert lib.wsu_ternary_entropy(16, 16, 16, l, 16, 16, big, 1, 8, 8, None) == -1 and b"outside 1..16" in lib.wsu_last_error()
    assert lib.wsu_ternary_entropy(16, 16, 16, 1, 16, 16, 8, 1, 8, 8, None) == -1 and b"workspace too small" in lib.wsu_last_error()
    assert lib.wsu_ternary_entropy(16, 16, 16, 1, 16, 12, big, 1, 8, 8, None) == -1 and b"8-byte aligned" in lib.wsu_last_error()
    assert lib.wsu_embed_ternary(None, None, None, None, None, None, 1, 8, 8, None) == -1 and b"embed_ternary: null" in lib.wsu_last_error()
    assert lib.wsu_embed_ternary(16, 16, 16, 16, 16, 16, 1, 8, 0, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_embed_ternary(16, 16, 16, 16, 16, 16, 1, 65536, 65536, None) == -1 and b"32-bit" in lib.wsu_last_error()
    assert lib.wsu_embed_lsbm(None, None, None, None, None, 1, 8, 8, None) == -1 and b"embed_lsbm: null" in lib.wsu_last_error()
    assert lib.wsu_embed_lsbm(16, 16, 16, 16, 16, 70000, 8, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()


def test_simulate_rejects_what_it_cannot_do():
    import torch
    x = torch.zeros((2, 4, 4), dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="LSBM / HILL"):
        embed_pm1.simulate(x, "HILLR", 0.4, [1, 2])
    with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
        embed_pm1.simulate(x, "LSBM", 1.2, [1, 2])
    with pytest.raises(ValueError, match=r"outside \[0, log2 3\)"):
        embed_pm1.simulate(x, "HILL", np.log2(3.0), [1, 2])
    with pytest.raises(ValueError, match=r"outside \[0, log2 3\)"):
        embed_pm1.simulate(x, "HILL", [0.4, -0.1], [1, 2])
    with pytest.raises(ValueError, match="one value per image"):
        embed_pm1.simulate(x, "HILL", [0.1, 0.2, 0.3], [1, 2])
    with pytest.raises(ValueError, match="seed"):
        embed_pm1.simulate(x, "LSBM", 0.4, None)
    with pytest.raises(ValueError, match="1 seeds for 2 images"):
        embed_pm1.simulate(x, "LSBM", 0.4, [1])
    with pytest.raises(ValueError, match="uint8"):
        embed_pm1.simulate(x.float(), "LSBM", 0.4, [1, 2])
    with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
        embed_pm1.write_dataset("nowhere", "LSBM", [0.4, 1.5])


def test_spam_names_the_new_methods():
    from ws_unet_amd import spam
    assert spam.SIMULATED == ("LSBR", "HILLR", "LSBM", "HILL")


# ---- the restatement on the inputs of the GPU tests -------------------------------------------------------------------------------------

def test_inputs_are_what_they_claim():
    for shape in pm1_np.SHAPES:
        x, rho = pm1_np.case("flat", shape)
        assert (x == 77).all() and (rho == 1e10).all()
        x, rho = pm1_np.case("ends", shape)
        assert set(np.unique(x)) <= {0, 255} and (x == 0).any() and (x == 255).any()
        assert (rho[:, 80:] == 1e10).all() and np.median(rho[:, :70]) < 1.0
        x, rho = pm1_np.case("noise", shape)
        assert len(np.unique(x)) > 40 and (rho < 1.0).all()
        assert len(np.unique(pm1_np.case("photo", shape)[0])) > 10


def test_entropy_limits_and_monotony():
    """lam -> 0: log2 3 bits per pixel, 1 bit at a pixel of 0 or 255; lam -> inf: none; in between it falls; rho = inf adds nothing"""
    x, rho = pm1_np.case("photo", (64, 64))
    hs = [pm1_np.entropy(x, rho, lam) for lam in pm1_np.LADDER]
    assert abs(hs[0] - x.size * np.log2(3.0)) < 1e-6 and hs[-1] == 0.0 and all(a >= b for a, b in zip(hs, hs[1:]))
    x, rho = pm1_np.case("ends", (64, 64))
    assert pm1_np.entropy(x, rho, pm1_np.LADDER[0]) == x.size
    wet = np.array(rho)
    wet[::3] = np.inf
    assert pm1_np.entropy(x, wet, 1e3) == pm1_np.entropy(x[np.isfinite(wet)], rho[np.isfinite(wet)], 1e3)
    # against -sum p log2 p, term by term
    x, rho = pm1_np.case("noise", (8, 8))
    pp, pm = pm1_np.probabilities(x, rho, 500.0)
    p0 = 1.0 - pp - pm
    with np.errstate(divide="ignore", invalid="ignore"):
        direct = -sum(np.where(p > 0, p * np.log2(p), 0.0).sum() for p in (p0, pp, pm))
    assert abs(direct - pm1_np.entropy(x, rho, 500.0)) < 1e-9


@pytest.mark.parametrize("content,shape,alpha", CASES)
def test_lambda_brackets_the_payload(content, shape, alpha):
    x, rho = pm1_np.case(content, shape)
    lo, hi, ok = pm1_np.case_lambda(content, shape, alpha)
    m = alpha * x.size
    assert ok == ((content, shape, alpha) not in SHORT)
    if ok:
        assert pm1_np.entropy(x, rho, lo) >= m >= pm1_np.entropy(x, rho, hi)
        assert 0 <= hi / lo - 1 <= 2.0 ** -29
    else:
        assert lo == hi == pm1_np.LADDER[0] and pm1_np.entropy(x, rho, lo) < m <= x.size


@pytest.mark.parametrize("content,shape,alpha", CASES)
def test_draws_of_the_gpu_cases(content, shape, alpha):
    """(a) the number of changes is within 5 sigma + 1 of its expectation; (b) no value leaves 0..255; (c) no draw is within 4 of a
    threshold, so a device exp one unit in the last place from numpy's (which moves a threshold by at most 1) draws the same image"""
    x, rho = pm1_np.case(content, shape)
    lam = pm1_np.case_lambda(content, shape, alpha)[0]
    pp, pm = pm1_np.probabilities(x, rho, lam)
    t = 2.0 ** -32 * np.float64(pm1_np.lsbm_threshold(alpha))
    lp, lm = pm1_np.lsbm_thresholds(x, alpha)
    for name, (stego, changes), q, (tp, tm) in (
            ("HILL", pm1_np.ternary_np(x, rho, lam, pm1_np.SEED), pp + pm, pm1_np.ternary_thresholds(x, rho, lam)),
            ("LSBM", pm1_np.lsbm_np(x, alpha, pm1_np.SEED), np.full(x.shape, 2 * t), (lp, lm))):
        assert abs(changes - q.sum()) <= 5 * np.sqrt((q * (1 - q)).sum()) + 1, name
        assert stego.min() >= 0 and stego.max() <= 255 and np.abs(stego - x).max() <= 1, name
        assert changes == np.count_nonzero(stego != x), name
        assert pm1_np.min_gap(x, tp, tm, pm1_np.SEED) > 4, name
        assert (tp[x == 255] == 0).all() and (tm[x == 0] == 0).all() and (tp + tm < 2 ** 32).all(), name
    if content == "ends" and alpha == 1.0:                                    # LSBM at full payload moves half of the pixels, all inwards
        stego = pm1_np.lsbm_np(x, alpha, pm1_np.SEED)[0]
        assert set(np.unique(stego)) <= {0, 1, 254, 255}
