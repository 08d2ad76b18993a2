"""CPU: the syndrome-trellis code's definition and host side (ws_unet_amd.stc, K40-K42): the numpy restatement (stc_np) against a brute
force over all stego vectors and against a dense parity-check matrix, the column table, block widths, bit packing, names and folders,
that `embed` and `embed_pm1` are untouched, and the argument checks of the C entries (no GPU here)."""
import ctypes

import numpy as np
import pytest

import stc_np
from ws_unet_amd import embed, embed_pm1, stc

SMALL_CASES = [(n, k, h, t) for (n, k, h) in stc_np.SMALL for t in range(stc_np.SMALL_TRIALS)]


@pytest.fixture(scope="module")
def lib():
    from ws_unet_amd import _lib
    return _lib.load()


# ---- the code ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k,h,trial", SMALL_CASES)
def test_restatement_is_the_minimum_over_all_solutions(n, k, h, trial):
    """cost == the brute-force minimum, exactly (the costs' sums are exact); H y = m through a matrix built apart; the cost is the sum
    of the changed positions' costs; an infeasible case gives ok False and y = x"""
    x, rho, m, cols = stc_np.small_case(n, k, h, trial)
    y, cost, ok = stc_np.viterbi(x, rho, m, cols, h)
    best = stc_np.brute_force(x, rho, m, cols, h)
    assert cost == best and ok == bool(np.isfinite(best))
    if trial == 1:
        assert not ok
    if ok:
        H = stc_np.dense_matrix(n, k, h, cols)
        np.testing.assert_array_equal((H.astype(np.int64) @ y) % 2, m)
        np.testing.assert_array_equal(stc_np.syndrome(y, k, cols, h), m)
        assert np.where(y != x, rho, 0.0).sum() == cost
    else:
        np.testing.assert_array_equal(y, x)
        assert np.isinf(cost)


def test_every_triple_has_wet_and_infeasible_cases():
    for n, k, h in stc_np.SMALL:
        oks = [stc_np.viterbi(*stc_np.small_case(n, k, h, t), h)[2] for t in range(stc_np.SMALL_TRIALS)]
        assert not oks[1] and sum(oks) >= stc_np.SMALL_TRIALS // 2
        assert all(np.isinf(stc_np.small_case(n, k, h, t)[1]).sum() in (1, 2) for t in (0, 3, 6, 9))


def test_free_message_and_ties():
    """a message the cover already carries costs nothing and changes nothing; where every cost is 0 all solutions tie and the one with
    y = 0 wherever the trellis has a choice is taken: the zero vector for the zero message"""
    cols = stc_np.columns(3, 3)
    x = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1], np.uint8)
    m = stc_np.syndrome(x, 4, cols, 3)
    y, cost, ok = stc_np.viterbi(x, np.ones(10), m, cols, 3)
    assert ok and cost == 0.0
    np.testing.assert_array_equal(y, x)
    y, cost, ok = stc_np.viterbi(x, np.zeros(10), np.zeros(4, np.uint8), cols, 3)
    assert ok and cost == 0.0 and not y.any()


def test_efficiency_on_a_constant_profile():
    """n = 4096, k = 1024, h = 8, unit costs: the embedding efficiency k / changes stays below the bound alpha / H^-1(alpha) = 6.0 at
    alpha = 1 / 4 and above 4.5 (the paper's h = 8 codes reach about 5 there; random embedding would give 2)"""
    rng = np.random.default_rng(3)
    x, m = rng.integers(0, 2, 4096).astype(np.uint8), rng.integers(0, 2, 1024).astype(np.uint8)
    cols = stc_np.columns(8, 4)
    y, cost, ok = stc_np.viterbi(x, np.ones(4096), m, cols, 8)
    assert ok and cost == np.count_nonzero(y != x)
    np.testing.assert_array_equal(stc_np.syndrome(y, 1024, cols, 8), m)
    print(f"efficiency {1024 / cost:.3f}")
    assert 4.5 < 1024 / cost < 6.0


# ---- columns, widths, bits ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", range(1, 11))
def test_columns(h):
    mid = 1 << max(h - 2, 0)
    cols = stc.columns(h, 2 * mid + 3)
    assert cols.dtype == np.uint32 and cols.shape == (2 * mid + 3,)
    assert ((cols & 1) == 1).all() and ((cols >> (h - 1)) & 1 == 1).all() and (cols < (1 << h)).all()
    assert len(set(cols[:mid].tolist())) == mid                                 # pairwise distinct up to 2^max(h-2, 0) ...
    np.testing.assert_array_equal(cols[mid:2 * mid], cols[:mid])                # ... then they repeat
    np.testing.assert_array_equal(cols, stc_np.columns(h, 2 * mid + 3))
    np.testing.assert_array_equal(stc.columns(h, 3), cols[:3])                  # a prefix, whatever wmax
    if h > 3:
        assert not np.array_equal(stc.columns(h, mid, key=1), cols[:mid])
        np.testing.assert_array_equal(stc.columns(h, mid, key=2 ** 40 + 5), stc_np.columns(h, mid, key=2 ** 40 + 5))


def test_columns_reject_bad_arguments():
    for bad in (0, 11, -1):
        with pytest.raises(ValueError, match="outside 1..10"):
            stc.columns(bad, 4)
    with pytest.raises(ValueError, match="wmax"):
        stc.columns(4, 0)
    with pytest.raises(ValueError, match="key"):
        stc.columns(4, 4, key=-1)


@pytest.mark.parametrize("n,k", [(14, 5), (16, 7), (13, 13), (1023, 410), (262144, 104858), (960, 1), (128, 9)])
def test_block_widths(n, k):
    wd = stc.block_widths(n, k)
    assert wd.shape == (k,) and wd.sum() == n and set(wd.tolist()) <= {n // k, n // k + 1} and wd.max() == -(-n // k)
    assert wd.tolist() == stc_np.widths(n, k)
    # the block of a position as the kernels find it: floor(((j + 1) k - 1) / n)
    if n <= 2048:
        starts = np.concatenate([[0], np.cumsum(wd)])
        for j in range(n):
            i = ((j + 1) * k - 1) // n
            assert starts[i] <= j < starts[i + 1]


def test_bits_and_bytes():
    data = bytes(range(256)) + b"syndrome-trellis"
    bits = stc.bits_from_bytes(data)
    assert bits.dtype == np.uint8 and bits.shape == (8 * len(data),) and set(bits.tolist()) == {0, 1}
    assert bits[8:16].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]                      # byte 1, most significant bit first
    assert stc.bytes_from_bits(bits) == data
    assert stc.bytes_from_bits(bits[:21]) == data[:2]                           # a trailing partial byte is dropped
    assert stc.bytes_from_bits([]) == b""
    with pytest.raises(ValueError, match="0 / 1"):
        stc.bytes_from_bits([0, 2, 1])


# ---- names ------------------------------------------------------------------------------------------------------------------------------

def test_names_and_folders():
    assert stc.METHODS == ("STCR", "STCM") and stc.CHANGE == {"STCR": "flip", "STCM": "pm1"}
    assert stc.method_name("stcr") == "STCR" and stc.method_name("Stcm") == "STCM"
    for bad in ("HILL", "LSBR", "STC"):
        with pytest.raises(NotImplementedError, match="STCR / STCM"):
            stc.method_name(bad)
    assert stc.folder_name("stcr", 0.4) == "stego_STCR_alpha_0.4_independent_images"
    assert stc.folder_name("STCM", 1) == "stego_STCM_alpha_1.0_independent_images"
    with pytest.raises(NotImplementedError):
        stc.folder_name("HILL", 0.4)
    import ws_unet_amd
    assert ws_unet_amd.stc is stc
    assert stc.MESSAGE_STREAM == stc_np.MESSAGE_STREAM


def test_the_other_embedders_are_untouched():
    assert embed.METHODS == ("LSBR", "HILLR", "LSBRS", "LSBRK", "HILLRM")
    assert embed_pm1.METHODS == ("LSBM", "HILL")
    for name in stc.METHODS:
        with pytest.raises(NotImplementedError):
            embed.method_name(name)
        with pytest.raises(NotImplementedError):
            embed_pm1.method_name(name)


def test_embed_and_extract_reject_what_they_cannot_do():
    import torch
    x = torch.zeros((2, 4, 4), dtype=torch.uint8)
    m = torch.zeros((2, 5), dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        stc.embed(x.float(), m, seeds=[1, 2])
    with pytest.raises(ValueError, match="message must be"):
        stc.embed(x, m[:1], seeds=[1, 2])
    with pytest.raises(ValueError, match="message must be"):
        stc.embed(x, m.float(), seeds=[1, 2])
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match=r"alpha outside \(0, 1\]"):
            stc.embed(x, bad, seeds=[1, 2])
    with pytest.raises(ValueError, match="less than one bit"):
        stc.embed(x, 0.01, seeds=[1, 2])
    with pytest.raises(ValueError, match="change"):
        stc.embed(x, m, seeds=[1, 2], change="ternary")
    with pytest.raises(ValueError, match="seed"):
        stc.embed(x, m, seeds=None)
    with pytest.raises(ValueError, match="1 seeds for 2 images"):
        stc.embed(x, m, seeds=[1])
    with pytest.raises(ValueError, match="outside 1..16"):
        stc.embed(x, torch.zeros((2, 17), dtype=torch.uint8), seeds=[1, 2])
    with pytest.raises(ValueError, match="outside 1..16"):
        stc.extract(x, 17, seeds=[1, 2])
    with pytest.raises(ValueError, match="uint8"):
        stc.extract(x.float(), 4, seeds=[1, 2])
    with pytest.raises(NotImplementedError, match="STCR / STCM"):
        stc.write_dataset("nowhere", "HILL", 0.4)
    with pytest.raises(ValueError, match=r"alpha outside \(0, 1\]"):
        stc.write_dataset("nowhere", "STCR", [0.4, 1.5])
    with pytest.raises(ValueError, match="either alpha"):
        stc.write_dataset("nowhere", "STCR")
    with pytest.raises(ValueError, match="either alpha"):
        stc.write_dataset("nowhere", "STCR", 0.4, message=b"x")
    with pytest.raises(ValueError, match="empty"):
        stc.write_dataset("nowhere", "STCR", message=b"")
    with pytest.raises(ValueError, match="outside 1..10"):
        stc.write_dataset("nowhere", "STCR", 0.4, h=11)


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------------

def test_gpu_cases_are_what_they_claim():
    for shape in stc_np.SHAPES:
        n = shape[0] * shape[1]
        for h in stc_np.HEIGHTS:
            k_odd, k_small, k_all = stc_np.ks_of(shape, h)
            assert n % k_odd and k_all == n and (k_small < h or h == 1)
        cover, rho = stc_np.image_case(shape, "wet")
        assert np.isinf(rho.reshape(-1)[::7]).all() and np.isfinite(rho).sum() == n - len(range(0, n, 7))
        assert np.isinf(stc_np.image_case(shape, "allwet")[1]).all()
        assert set(np.unique(stc_np.image_case(shape, "ends")[0])) == {0, 255}
        assert not np.array_equal(stc_np.image_case(shape, "a")[0], stc_np.image_case(shape, "b")[0])
    # all wet and the cover is no solution: infeasible; the stego is the cover
    shape, h = (8, 16), 6
    k = stc_np.ks_of(shape, h)[0]
    cover, _ = stc_np.image_case(shape, "allwet")
    assert not np.array_equal(stc_np.syndrome(cover.reshape(-1) & 1, k, stc_np.columns(h, -(-128 // k)), h), stc_np.message_case(shape, k, "a"))
    out, cost, changes, ok = stc_np.reference(shape, "allwet", h, k)
    assert not ok and np.isinf(cost) and changes == 0 and np.array_equal(out, cover)
    # a keyed path is a permutation that differs from the raster, and the message stream differs from the path's
    p = stc_np.key_path(stc_np.SEED, 128)
    assert sorted(p.tolist()) == list(range(128)) and p.tolist() != list(range(128))
    assert not np.array_equal(stc_np.random_message(stc_np.SEED, 128), (stc_np.words(128, stc_np.SEED) & 1).astype(np.uint8))


def test_reference_reads_back_and_pm1_keeps_the_parity():
    shape, h = (8, 16), 7
    k = stc_np.ks_of(shape, h)[0]
    cols = stc_np.columns(h, -(-128 // k))
    cover, rho = stc_np.image_case(shape, "a")
    flip = stc_np.reference(shape, "a", h, k, "flip", True)
    pm1 = stc_np.reference(shape, "a", h, k, "pm1", True)
    assert flip[3] and pm1[3] and flip[1] == pm1[1] and flip[2] == pm1[2] == np.count_nonzero(flip[0] != cover)
    np.testing.assert_array_equal(flip[0] & 1, pm1[0] & 1)
    assert np.abs(pm1[0].astype(int) - cover).max() == 1
    path = stc_np.key_path(stc_np.SEED, 128)
    np.testing.assert_array_equal(stc_np.syndrome(pm1[0].reshape(-1)[path] & 1, k, cols, h), stc_np.message_case(shape, k, "a"))
    assert abs(flip[1] - rho[flip[0] != cover].sum()) < 128 * 2.0 ** -52 * flip[1]  # the same terms in another order


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------

def test_entries_validate_before_any_gpu_call(lib):
    """errno-style code + message for null pointers, bad heights, counts and shapes, with no GPU present"""
    assert lib.wsu_stc_workspace_bytes(512 * 512, 10) == 32 << 20
    assert lib.wsu_stc_workspace_bytes(1000, 7) == 1000 * 16 and lib.wsu_stc_workspace_bytes(1000, 6) == lib.wsu_stc_workspace_bytes(1000, 1) == 8000
    assert lib.wsu_stc_workspace_bytes(0, 7) == lib.wsu_stc_workspace_bytes(10, 0) == lib.wsu_stc_workspace_bytes(10, 11) == 0
    big = 1 << 20

    def emb(*, ptr=16, change=0, height=7, k=5, phases=3, ws=16, ws_bytes=big, n=1, h=8, w=8):
        return lib.wsu_stc_embed(ptr, ptr, ptr, ptr, None, ptr, change, height, k, phases, ptr, ptr, ptr, ptr, ws, ws_bytes, n, h, w, None)

    assert emb(ptr=None) == -1 and b"stc_embed: null" in lib.wsu_last_error()
    assert emb(ws=None) == -1 and b"stc_embed: null" in lib.wsu_last_error()
    for bad in (0, 11, -3):
        assert emb(height=bad) == -1 and b"outside 1..10" in lib.wsu_last_error()
    assert emb(k=0) == -1 and b"at least 1" in lib.wsu_last_error()
    assert emb(k=65) == -1 and b"exceed the 64 pixels" in lib.wsu_last_error()
    for bad in (2, -1):
        assert emb(change=bad) == -1 and b"neither 0 (flip) nor 1 (pm1)" in lib.wsu_last_error()
    for bad in (0, 4):
        assert emb(phases=bad) == -1 and b"phases" in lib.wsu_last_error()
    assert emb(n=0) == -1 and b"bad shape" in lib.wsu_last_error()
    assert emb(w=0) == -1 and b"bad shape" in lib.wsu_last_error()
    assert emb(h=65536, w=32768, k=5) == -1 and b"32-bit path" in lib.wsu_last_error()
    assert emb(ws_bytes=64 * 16 - 1) == -1 and b"workspace too small" in lib.wsu_last_error()
    assert emb(ws=12) == -1 and b"8-byte aligned" in lib.wsu_last_error()

    def ext(*, ptr=16, height=7, k=5, n=1, h=8, w=8):
        return lib.wsu_stc_extract(ptr, ptr, None, height, k, ptr, n, h, w, None)

    assert ext(ptr=None) == -1 and b"stc_extract: null" in lib.wsu_last_error()
    for bad in (0, 11):
        assert ext(height=bad) == -1 and b"outside 1..10" in lib.wsu_last_error()
    assert ext(k=0) == -1 and b"at least 1" in lib.wsu_last_error()
    assert ext(k=65) == -1 and b"exceed the 64 pixels" in lib.wsu_last_error()
    assert ext(n=70000) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_philox_words(None, None, 1, 8, 8, None) == -1 and b"philox_words: null" in lib.wsu_last_error()
    assert lib.wsu_philox_words(16, 16, 1, 0, 8, None) == -1 and b"bad shape" in lib.wsu_last_error()
    assert lib.wsu_philox_words(16, 16, 1, 65536, 65536, None) == -1 and b"32-bit" in lib.wsu_last_error()
