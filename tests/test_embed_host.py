"""CPU: the host side of the stego simulators (ws_unet_amd.embed) -- the numpy oracle against the reference's HILLR files, the
generator's known answers, seeds, thresholds and the argument checks of the new C entries (no GPU here)."""
import ctypes

import numpy as np
import pytest

from conftest import GOLDEN
import embed_np
import hill_np
from ws_unet_amd import embed
from ws_unet_amd.imread import imread4_u8

COVERS = (6, 7, 8, 9, 10)


@pytest.fixture(scope="module")
def lib():
    from ws_unet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("k", COVERS)
def test_hillr_np_reproduces_the_reference_files(k):
    cover = imread4_u8(GOLDEN / f"cover_{k}.png")[..., 3]
    cost = hill_np.hill_cost(cover)
    for alpha, changes in ((0.01, 1311), (0.4, 52429)):
        ref = imread4_u8(GOLDEN / f"stego_HILLR_{alpha}_{k}.png")[..., 3]
        got = embed_np.hillr_np(cover, alpha, cost)
        assert np.array_equal(got, ref)
        assert int((got != cover).sum()) == changes and np.array_equal(got >> 1, cover >> 1)
    assert np.array_equal(embed_np.hillr_np(cover, 0.0), cover)


def test_philox_known_answers():
    zero = embed_np.philox4x32_10(np.zeros(4, np.uint32), (0, 0))
    assert [f"{v:08x}" for v in zero] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = embed_np.philox4x32_10(np.full(4, 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))
    assert [f"{v:08x}" for v in ones] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    # vectorised over counters = one call per counter
    ctr = np.zeros((5, 4), np.uint32)
    ctr[:, 0] = [0, 1, 2, 0xFFFFFFFF, 77]
    many = embed_np.philox4x32_10(ctr, (123, 0x80000001))
    for i in range(5):
        assert np.array_equal(many[i], embed_np.philox4x32_10(ctr[i], (123, 0x80000001)))


def test_lsbr_np_rate_and_lsb_only():
    cover = np.random.default_rng(0).integers(0, 256, (96, 100), dtype=np.uint8)
    assert np.array_equal(embed_np.lsbr_np(cover, 0.0, 5), cover)
    st = embed_np.lsbr_np(cover, 0.4, 5)
    assert np.array_equal(st >> 1, cover >> 1)
    rate = (st != cover).mean()
    assert abs(rate - 0.2) < 4 * np.sqrt(0.2 * 0.8 / cover.size)          # 4 sigma of a binomial count
    assert not np.array_equal(st, embed_np.lsbr_np(cover, 0.4, 6))
    assert not np.array_equal(st, embed_np.lsbr_np(cover, 0.4, 5 | (1 << 32)))


def test_image_seed_is_a_function_of_stem_and_stream():
    a = embed.image_seed("images/6.png")
    assert a == embed.image_seed("/somewhere/else/6.pgm") == embed.image_seed("6.png", stream=0)
    assert a != embed.image_seed("images/7.png")
    assert 0 <= a < 2 ** 31
    b = embed.image_seed("images/6.png", stream=3)
    assert b != a and b & 0xFFFFFFFF == a and b >> 32 == 3
    with pytest.raises(ValueError):
        embed.image_seed("6.png", stream=-1)


def test_lsbr_threshold(lib):
    from ws_unet_amd import ops
    assert [ops.lsbr_threshold(a) for a in (0.0, 0.4, 1.0)] == [0, 858993459, 2 ** 31]
    assert [embed_np.lsbr_threshold(a) for a in (0.0, 0.4, 1.0)] == [0, 858993459, 2 ** 31]
    t = ctypes.c_uint32(7)
    for bad in (-0.01, 1.0000001, float("nan")):
        assert lib.wsu_lsbr_threshold(bad, ctypes.byref(t)) == -1 and b"outside [0, 1]" in lib.wsu_last_error()
    assert t.value == 7
    assert lib.wsu_lsbr_threshold(0.5, None) == -1 and b"null" in lib.wsu_last_error()


def test_hillr_rank():
    assert [embed.hillr_rank(a, 512, 512) + 1 for a in (0.01, 0.05, 0.1, 0.2, 0.4)] == [1311, 6554, 13108, 26215, 52429]
    assert embed.hillr_rank(0.0, 512, 512) == -1 and embed.hillr_rank(1.0, 3, 5) == 7
    assert [embed_np.hillr_rank(a, 70, 90) for a in (0.01, 0.4, 1.0)] == [embed.hillr_rank(a, 70, 90) for a in (0.01, 0.4, 1.0)]


def test_entries_validate_before_any_gpu_call(lib):
    """errno-style code + message for null pointers and bad shapes, with no GPU present"""
    assert lib.wsu_hill_cost_f64(None, None, 1e10, 1, 8, 8, None) == -1 and b"hill_cost_f64: null" in lib.wsu_last_error()
    assert lib.wsu_hill_cost_f64(16, 16, 0.0, 1, 8, 8, None) == -1 and b"clamp" in lib.wsu_last_error()
    assert lib.wsu_hill_cost_f64(16, 16, 1e10, 1, 0, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_rank_select_f64(None, None, None, None, 0, 1, 8, 8, None) == -1 and b"rank_select_f64: null" in lib.wsu_last_error()
    assert lib.wsu_rank_select_f64(16, 16, 16, 16, 8, 1, 8, 8, None) == -1 and b"workspace too small" in lib.wsu_last_error()
    assert lib.wsu_rank_select_f64(16, 16, 16, 16, 1 << 30, 1, 65536, 65536, None) == -1 and b"32-bit" in lib.wsu_last_error()
    assert lib.wsu_rank_select_f64_workspace_bytes(0) == 0 and lib.wsu_rank_select_f64_workspace_bytes(3) == 3 * (16 + 6 * 2048 * 4)
    assert lib.wsu_embed_threshold(None, None, None, None, None, 1, 8, 8, None) == -1 and b"embed_threshold: null" in lib.wsu_last_error()
    assert lib.wsu_embed_threshold(16, 16, 16, 16, 16, 70000, 8, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_embed_lsbr(None, None, None, None, None, 1, 8, 8, None) == -1 and b"embed_lsbr: null" in lib.wsu_last_error()
    assert lib.wsu_embed_lsbr(16, 16, 16, 16, 16, 1, 8, -1, None) == -1 and b"bad shape" in lib.wsu_last_error()


def test_simulate_rejects_what_it_cannot_do():
    import torch
    x = torch.zeros((1, 4, 4), dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="LSBR / HILLR"):
        embed.simulate(x, "WOW", 0.4)
    assert embed.method_name("LSBr") == "LSBR" and embed.method_name("hillr") == "HILLR"
    with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
        embed.simulate(x, "LSBR", 1.5, [1])
    with pytest.raises(ValueError, match="seed"):
        embed.simulate(x, "LSBR", 0.4)
    with pytest.raises(ValueError, match="one value per image"):
        embed.simulate(x, "HILLR", [0.1, 0.2])
    assert embed.folder_name("HILLr", 0.4) == "stego_HILLR_alpha_0.4_independent_images"
    import ws_unet_amd
    assert ws_unet_amd.simulate is embed.simulate and ws_unet_amd.image_seed is embed.image_seed


def test_pair_loader_simulate_needs_a_device(tmp_path):
    import shutil
    from ws_unet_amd.data.pairs import PairLoader
    (tmp_path / "images").mkdir()
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", tmp_path / "images" / f"{k}.png")
    (tmp_path / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    with pytest.raises(ValueError, match="simulate=True"):
        PairLoader(tmp_path, None, "HILLR", 0.4, batch_size=2, device=None, simulate=True)
