"""CPU: the restatement of the ternary two-layer syndrome-trellis embedder (stc_ml_np) on the fixture grid the GPU tests use: every fixture
at alpha <= 0.4 has a solution and reads back, the changes are +-1 inside the range and spare the wet pixels, the `ends` planes run on the
low layer alone, no high-layer entropy lies where the device's floor could differ, and the alpha 1.0 fixtures are pinned as found; the
names, folders and argument errors of ws_unet_amd.stc_ml, and that the older modules' method lists are what they were."""
import math

import numpy as np
import pytest
import torch

import pm1_np
import stc_ml_np
from ws_unet_amd import embed, embed_pm1, stc, stc_ml

LOW = [f for f in stc_ml_np.FIXTURES if f[2] <= 0.4]
FULL = [f for f in stc_ml_np.FIXTURES if f[2] == 1.0]
# the alpha 1.0 fixtures in which the restatement finds no solution, all in the low layer (the high layer and the capacity hold everywhere)
NO_SOLUTION = {
    ("photo", (8, 16), 6), ("photo", (33, 31), 6), ("photo", (33, 31), 7),
}


def test_the_grid():
    assert len(stc_ml_np.FIXTURES) == 4 * (2 + 3 + 2) * 3
    assert {f[3] for f in stc_ml_np.FIXTURES if f[1] == (24, 40)} == {6, 7, 10} and {f[3] for f in stc_ml_np.FIXTURES if f[1] != (24, 40)} == {6, 7}


@pytest.mark.parametrize("content,shape,alpha,h", LOW)
def test_low_payloads_embed_and_read_back(content, shape, alpha, h):
    x, rho = stc_ml_np.case(content, shape)
    m = stc_ml_np.message(shape, alpha)
    r = stc_ml_np.reference(content, shape, alpha, h)
    assert r["ok"] and r["fits"] and r["ok1"] and r["ok0"]
    assert r["k1"] + r["k0"] == len(m) and r["k0"] >= 1 and 0 <= r["k1"] <= len(m) - 1
    _changes_are_sound(x, rho, r)
    np.testing.assert_array_equal(stc_ml_np.extract(r["stego"], r["k1"], r["k0"], h), m)
    if content == "ends":
        assert r["H1"] == 0.0 and r["k1"] == 0 and np.isinf(r["rho1"]).all()


def _changes_are_sound(x, rho, r):
    s = r["stego"].astype(np.int64)
    d = s - x
    assert set(np.unique(d)) <= {-1, 0, 1} and s.min() >= 0 and s.max() <= 255
    assert not d[np.isinf(rho)].any() and r["changes"] == np.count_nonzero(d)
    assert r["distortion"] == math.fsum(rho[d != 0].tolist())
    if r["ok"]:
        np.testing.assert_array_equal((r["stego"] >> 1) & 1, r["y1"])
        np.testing.assert_array_equal(r["stego"] & 1, r["y0"])
        assert r["changes"] > 0
    else:
        assert not d.any() and r["distortion"] == 0.0


@pytest.mark.parametrize("content,shape,alpha,h", stc_ml_np.FIXTURES)
def test_no_entropy_lies_near_an_integer(content, shape, alpha, h):
    """the device sums in another order and with its own exp / log: its H1 differs from this one by at most (H W + 64) 2^-52 H1, so the
    two floors agree when no H1 is that near an integer (or is capped by k - 1 on both sides)"""
    r = stc_ml_np.reference(content, shape, alpha, h)
    H1, hw = r["H1"], shape[0] * shape[1]
    assert abs(H1 - round(H1)) > (hw + 64) * 2.0 ** -52 * H1 or H1 == 0.0
    assert r["k1"] == min(math.floor(H1), stc_ml_np.bits_of(shape, alpha) - 1)


@pytest.mark.parametrize("content,shape,alpha,h", FULL)
def test_full_payloads_are_what_the_restatement_finds(content, shape, alpha, h):
    """alpha 1.0: some planes leave the low layer without a solution; such an image is reported and copied, not repaired"""
    x, rho = stc_ml_np.case(content, shape)
    r = stc_ml_np.reference(content, shape, alpha, h)
    assert r["fits"] and r["ok1"]
    assert r["ok"] == ((content, shape, h) not in NO_SOLUTION), (content, shape, h, r["ok0"])
    _changes_are_sound(x, rho, r)
    if r["ok"]:
        np.testing.assert_array_equal(stc_ml_np.extract(r["stego"], r["k1"], r["k0"], h), stc_ml_np.message(shape, alpha))


def test_the_layers_split_the_ternary_sender():
    """the chain rule behind the costs: q1 and the low layer's flip probability given that bit 1 is kept multiply out to the sender's p+-,
    and rho1 is the log-odds of q1"""
    x, rho = stc_ml_np.case("noise", (24, 40))
    lam = pm1_np.case_lambda("noise", (24, 40), 0.4)[0]
    pp, pm = pm1_np.probabilities(x, rho, lam)
    ad, ao, ed, eo, z = stc_ml_np.directions(x, rho, lam)
    u1, rho1, h1 = stc_ml_np.high_planes(x, rho, lam)
    odd = (x & 1) == 1
    q1 = np.where(odd, pp, pm)
    inner = (x > 0) & (x < 255)
    np.testing.assert_allclose(1.0 / (1.0 + np.exp(rho1[inner])), q1[inner], rtol=1e-12)
    q0 = 1.0 / (1.0 + np.exp(ao))                                            # the low layer's flip probability where bit 1 is kept
    np.testing.assert_allclose((1.0 - q1) * q0, np.where(odd, pm, pp), rtol=1e-12)
    with np.errstate(divide="ignore", invalid="ignore"):
        hb = -(q1 * np.log2(q1) + (1 - q1) * np.log2(1 - q1))                # (nan at a wet end, which `inner` leaves out)
    np.testing.assert_allclose(h1[inner], hb[inner], rtol=1e-10)
    assert np.array_equal(u1, (x >> 1) & 1)


def test_names_and_folders():
    assert stc_ml.METHODS == ("STCT",)
    assert stc_ml.method_name("stct") == "STCT" and stc_ml.method_name() == "STCT"
    assert stc_ml.folder_name("STCT", 0.4) == "stego_STCT_alpha_0.4_independent_images"
    for other in ("STCM", "STCR", "HILL", "STC"):
        with pytest.raises(NotImplementedError, match="STCT"):
            stc_ml.method_name(other)
    import ws_unet_amd
    assert ws_unet_amd.stc_ml is stc_ml


def test_the_older_method_lists_are_unchanged():
    assert stc.METHODS == ("STCR", "STCM") and embed_pm1.METHODS == ("LSBM", "HILL")
    assert embed.METHODS == ("LSBR", "HILLR", "LSBRS", "LSBRK", "HILLRM")
    with pytest.raises(NotImplementedError):
        stc.method_name("STCT")


def test_argument_errors_before_any_device_work(tmp_path):
    cover = torch.zeros((2, 8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        stc_ml.embed(cover.float(), 0.4, seeds=[1, 2])
    with pytest.raises(ValueError, match="log2 3"):
        stc_ml.embed(cover, 1.6, seeds=[1, 2])
    with pytest.raises(ValueError, match="log2 3"):
        stc_ml.embed(cover, 0.0, seeds=[1, 2])
    with pytest.raises(ValueError, match="at least 2"):
        stc_ml.embed(cover, 0.01, seeds=[1, 2])
    with pytest.raises(ValueError, match="at least 2"):
        stc_ml.embed(cover, torch.zeros((2, 1), dtype=torch.uint8), seeds=[1, 2])
    with pytest.raises(ValueError, match="message must be"):
        stc_ml.embed(cover, torch.zeros((3, 9), dtype=torch.uint8), seeds=[1, 2])
    with pytest.raises(ValueError, match="outside 1..10"):
        stc_ml.embed(cover, 0.4, seeds=[1, 2], h=11)
    with pytest.raises(ValueError, match="seed"):
        stc_ml.embed(cover, 0.4, seeds=None)
    with pytest.raises(ValueError, match="layers must be"):
        stc_ml.extract(cover, [[3, 4]], seeds=[1, 2])
    with pytest.raises(ValueError, match="layers must be"):
        stc_ml.extract(cover, [[3, 0], [3, 4]], seeds=[1, 2])
    with pytest.raises(ValueError, match="outside 1..10"):
        stc_ml.extract(cover, [[3, 4], [3, 4]], seeds=[1, 2], h=0)
    with pytest.raises(ValueError, match="either alpha"):
        stc_ml.write_dataset(tmp_path, "STCT")
    with pytest.raises(ValueError, match="either alpha"):
        stc_ml.write_dataset(tmp_path, "STCT", 0.4, message=b"x")
    with pytest.raises(ValueError, match="log2 3"):
        stc_ml.write_dataset(tmp_path, "STCT", 1.7)
    with pytest.raises(NotImplementedError):
        stc_ml.write_dataset(tmp_path, "STCM", 0.4)
    with pytest.raises(SystemExit):
        stc_ml.main(["embed", "--data", str(tmp_path)])
    with pytest.raises(SystemExit):
        stc_ml.main(["extract", "--data", str(tmp_path), "--alpha", "0.4", "--bits", "9", "--out", str(tmp_path)])


def test_c_entries_check_their_arguments_before_any_device_work():
    """errno-style code and message, no GPU needed: null ks, a row stride below the bits in use, the bit, the workspace"""
    from ws_unet_amd import _lib
    lib = _lib.load()
    one = 8                                                                  # any non-null, 8-byte aligned address: nothing is dereferenced
    per = lib.wsu_stc_workspace_bytes(64, 7)
    assert per == 64 * 16 and lib.wsu_stc_layer_workspace_bytes(3) == 3 * 64 * 16 and lib.wsu_stc_layer_workspace_bytes(0) == 0

    def embed(ks=one, first=one, stride=20, max_bits=20, cols_len=4, change=0, height=7, ws=one, ws_bytes=2 * per, n=2):
        return lib.wsu_stc_embed_ragged(one, one, one, stride, ks, first, max_bits, one, cols_len, None, one, change, height, one, one, one, one,
                                        ws, ws_bytes, n, 8, 8, None)

    def extract(ks=one, first=one, stride=20, max_bits=20, cols_len=4, bit=0, height=7):
        return lib.wsu_stc_extract_ragged(one, one, cols_len, None, height, bit, ks, first, max_bits, one, stride, 2, 8, 8, None)

    for call, word in ((lambda: embed(ks=None), b"null ks"), (lambda: embed(first=None), b"null ks or first"),
                       (lambda: embed(stride=19), b"message_stride=19"), (lambda: embed(max_bits=0), b"max_bits=0"),
                       (lambda: embed(cols_len=0), b"cols_len=0"), (lambda: embed(change=2), b"change=2"),
                       (lambda: embed(height=11), b"height 11"), (lambda: embed(ws_bytes=2 * per - 1), b"workspace too small"),
                       (lambda: embed(ws=12), b"8-byte aligned"), (lambda: embed(n=0), b"bad shape"),
                       (lambda: extract(ks=None), b"null ks"), (lambda: extract(stride=19), b"message_stride=19"),
                       (lambda: extract(bit=8), b"bit=8"), (lambda: extract(bit=-1), b"bit=-1"), (lambda: extract(height=0), b"height 0")):
        assert call() == -1 and word in lib.wsu_last_error(), (word, lib.wsu_last_error())
    assert lib.wsu_stc_layer_high(one, one, one, one, one, one, None, 0, 2, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_stc_layer_high(one, one, one, one, one, one, one, 2 * 64 * 16 - 1, 2, 8, 8, None) == -1 and b"workspace too small" in lib.wsu_last_error()
    assert lib.wsu_stc_layer_low(one, one, one, one, None, one, one, 2, 8, 8, None) == -1 and b"null" in lib.wsu_last_error()
    assert lib.wsu_stc_layer_compose(one, one, one, one, one, one, one, one, one, one, one, 12, 2 * 64 * 16, 2, 8, 8, None) == -1
    assert b"8-byte aligned" in lib.wsu_last_error()
