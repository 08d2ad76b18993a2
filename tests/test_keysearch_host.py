"""CPU: the host side of the stego-key search (K35, ws_unet_amd/ws/keysearch.py): the argument errors of the C entry (no GPU call is made),
the numpy restatement's own properties, `scores` / `standardise` on numpy arrays and torch tensors against the restatement, the
argument checks of ops.ws_key_search and of the search, the CLI parser and the keys file."""
import numpy as np
import pytest
import torch

import keysearch_np
import locate_np
from ws_unet_amd import _lib, ops
from ws_unet_amd.ws import keysearch, locate

NAN = float("nan")


# ---- the C entry's argument errors: errno-style code + message before any HIP call -----------------------------------------------

def _call(lib, *, num=8, den=8, count=16, keys=None, first=5, key_range=1, k=4, thr=7, parts=0, snum=8, sden=8):
    return lib.wsu_ws_key_search(num, den, count, keys, first, key_range, k, thr, parts, snum, sden, None)


def test_c_entry_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lib.wsu_last_error
    for name in ("num", "den", "snum", "sden"):
        assert _call(lib, **{name: None}) == -1 and b"null" in err(), name
    assert _call(lib, thr=2 ** 32 + 1) == -1 and b"above 2^32" in err()
    assert _call(lib, k=0) == -1 and b"k=0" in err()
    assert _call(lib, k=-3) == -1 and b"k=-3" in err()
    assert _call(lib, count=0) == -1 and b"count=0" in err()
    assert _call(lib, count=2 ** 34 + 1) == -1 and b"2^34" in err()
    assert _call(lib, keys=8, key_range=1) == -1 and b"exactly one" in err()               # both the array and the range
    assert _call(lib, keys=None, key_range=0) == -1 and b"exactly one" in err()            # neither
    assert _call(lib, keys=None, key_range=2) == -1 and b"key_range=2" in err()
    assert _call(lib, parts=-1) == -1 and b"parts=-1" in err()
    assert _call(lib, parts=65536) == -1 and b"parts=65536" in err()
    for name in ("num", "den", "snum", "sden"):
        assert _call(lib, **{name: 12}) == -1 and b"aligned" in err(), name
    assert _call(lib, keys=12, key_range=0) == -1 and b"aligned" in err()
    assert "wsu_ws_key_search" in _lib.SIGNATURES


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------

def _planes(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-2 ** 40, 2 ** 40, (h - 2, w - 2), dtype=np.int64), rng.integers(0, 2 ** 34, (h - 2, w - 2), dtype=np.int64)


def test_restatement_ends_nesting_and_mask():
    h, w = 11, 13
    num, den = _planes(h, w, 3)
    fn, fd = keysearch_np.frames(num, den)
    assert fn.shape == (h, w) and (fn[0] == 0).all() and (fn[:, -1] == 0).all() and (fn[1:-1, 1:-1] == num).all()
    keys = [0, 1, 2 ** 32, 2 ** 64 - 1, 12345678901234567890]
    sn, sd = keysearch_np.key_sums(fn, fd, keys, 2 ** 32)
    assert sn.dtype == np.int64 and (sn == num.sum()).all() and (sd == den.sum()).all()    # every word is below 2^32: the total
    sn, sd = keysearch_np.key_sums(fn, fd, keys, 0)
    assert not sn.any() and not sd.any()
    for key in keys:
        for alpha in (0.05, 0.5):
            mask = locate_np.key_mask_np(key, alpha, h, w).astype(np.int64)
            sn, sd = keysearch_np.key_sums(fn, fd, [key], locate_np.key_threshold(alpha))
            assert sn[0] == (mask * fn).sum() == (mask[1:-1, 1:-1] * num).sum() and sd[0] == (mask * fd).sum()
    # thresholds nest: the count of selected pixels never falls as the threshold grows, and ends at every pixel
    ones = np.ones((h, w), dtype=np.int64)
    last = np.zeros(len(keys), dtype=np.int64)
    for thr in (1, 2 ** 20, 2 ** 30, 2 ** 31, 2 ** 32 - 1, 2 ** 32):
        cnt, sd = keysearch_np.key_sums(ones, fd, keys, thr)
        assert (cnt >= last).all()
        last = cnt
    assert (last == h * w).all()
    wd = keysearch_np.words(h * w, keys)
    assert ((wd < np.uint64(2 ** 20)) <= (wd < np.uint64(2 ** 31))).all() and wd.shape == (len(keys), h * w)     # a subset, pixel by pixel
    # a prefix: rows = 1 reads the top border only
    sn, sd = keysearch_np.key_sums(fn, fd, keys, 2 ** 31, count=w)
    assert not sn.any() and not sd.any()
    sn, _ = keysearch_np.key_sums(fn, fd, keys, 2 ** 32, count=3 * w)
    assert (sn == num[:2].sum()).all()
    assert keysearch_np.key_range(2 ** 64 - 2, 4) == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1]


def test_restatement_sums_wrap_as_int64():
    big = np.array([2 ** 62, 2 ** 62, 2 ** 62, -5], dtype=np.int64)
    sn, sd = keysearch_np.key_sums(big, big, [7], 2 ** 32)
    assert sn[0] == (3 * 2 ** 62 - 5) - 2 ** 64 == sd[0]


# ---- the score and its standardisation -----------------------------------------------------------------------------------------------

def test_scores_and_standardise_on_numpy_and_torch():
    snum = np.array([1 << 23, 0, -(1 << 24), 5, 3 << 22, 1 << 22], dtype=np.int64)
    sden = np.array([1 << 32, 1 << 32, 1 << 31, 0, 1 << 32, 1 << 32], dtype=np.int64)
    want = np.array([0.5, 0.0, -2.0, NAN, 0.75, 0.25])
    for got in (keysearch.scores(snum, sden), keysearch.scores(torch.from_numpy(snum), torch.from_numpy(sden)).numpy(),
                keysearch_np.scores(snum, sden)):
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, want)
    # finite scores -2, 0, .25, .5, .75: median .25; |dev| 2.25, .25, 0, .25, .5: MAD .25
    assert keysearch.null_of(want) == (0.25, 0.25) == keysearch.null_of(torch.from_numpy(want))
    z = np.array([0.25, -0.25, -2.25, NAN, 0.5, 0.0]) / (1.4826 * 0.25)
    for got in (keysearch.standardise(want), keysearch.standardise(torch.from_numpy(want)).numpy(), keysearch_np.standardise(want)):
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, z)
    np.testing.assert_array_equal(keysearch.standardise(want, (0.5, 1.0)), (want - 0.5) / 1.4826)
    even = np.array([4.0, 1.0, 3.0, 2.0])                                                   # an even count: the mean of the two middle values
    assert keysearch.null_of(even) == (2.5, 1.0) and keysearch.null_of(torch.from_numpy(even)) == (2.5, 1.0)
    rng = np.random.default_rng(1).standard_normal(1001)
    np.testing.assert_array_equal(keysearch.standardise(rng), keysearch_np.standardise(rng))
    np.testing.assert_array_equal(keysearch.standardise(torch.from_numpy(rng)).numpy(), keysearch_np.standardise(rng))
    with np.errstate(all="ignore"):
        one = keysearch.standardise(np.array([0.5]))                                       # one key: MAD = 0
    assert np.isnan(one[0]) and np.isnan(keysearch.null_of(np.array([NAN]))[0])
    assert keysearch.hex_key(255) == "0x00000000000000ff" and keysearch.hex_key(-1) == "0x" + "f" * 16


# ---- argument checks before any device work ----------------------------------------------------------------------------------------------

def test_op_argument_errors_before_any_device_work():
    num, den = torch.zeros((6, 6), dtype=torch.int64), torch.ones((6, 6), dtype=torch.int64)
    keys = torch.arange(4, dtype=torch.int64)
    ok = dict(keys=keys, alpha_threshold=7)
    with pytest.raises(ValueError, match="3 x 3"):
        ops.ws_key_search(num, den, 2, 8, **ok)
    with pytest.raises(ValueError, match="shape"):
        ops.ws_key_search(num, den, 8, 9, **ok)
    with pytest.raises(ValueError, match="int64"):
        ops.ws_key_search(num.to(torch.int32), den, 8, 8, **ok)
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_key_search(num, den, 8, 8, alpha_threshold=7)
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_key_search(num, den, 8, 8, keys=keys, key_first=0, count=4, alpha_threshold=7)
    with pytest.raises(ValueError, match="both key_first and count"):
        ops.ws_key_search(num, den, 8, 8, key_first=0, alpha_threshold=7)
    for thr in (-1, 2 ** 32 + 1):
        with pytest.raises(ValueError, match="alpha_threshold"):
            ops.ws_key_search(num, den, 8, 8, keys=keys, alpha_threshold=thr)
    for rows in (0, 9):
        with pytest.raises(ValueError, match="rows"):
            ops.ws_key_search(num, den, 8, 8, rows=rows, **ok)
    for parts in (-1, 65536):
        with pytest.raises(ValueError, match="parts"):
            ops.ws_key_search(num, den, 8, 8, parts=parts, **ok)
    with pytest.raises(ValueError, match="keys must be"):
        ops.ws_key_search(num, den, 8, 8, keys=keys.to(torch.int32), alpha_threshold=7)
    with pytest.raises(ValueError, match="keys must be"):
        ops.ws_key_search(num, den, 8, 8, keys=keys[:0], alpha_threshold=7)
    for count in (0, 2 ** 31):
        with pytest.raises(ValueError, match="count"):
            ops.ws_key_search(num, den, 8, 8, key_first=0, count=count, alpha_threshold=7)
    for first in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="key_first"):
            ops.ws_key_search(num, den, 8, 8, key_first=first, count=4, alpha_threshold=7)
    with pytest.raises(_lib.WsuError, match="CPU tensor"):                                 # a valid call gets as far as the device check
        ops.ws_key_search(num, den, 8, 8, **ok)
    # the exact |sum| the overflow guard compares: high and low halves apart, so it cannot wrap itself
    big = torch.full((6, 6), 2 ** 58, dtype=torch.int64)
    assert ops._abs_sum(big) == 36 * 2 ** 58 and ops._abs_sum(-big) == 36 * 2 ** 58 and ops._abs_sum(num) == 0
    assert ops._abs_sum(torch.tensor([-2 ** 63, 5])) >= 2 ** 63 and ops._abs_sum(torch.tensor([-7, 2 ** 40 + 3, -(2 ** 33)])) == 10 + 2 ** 40 + 2 ** 33
    assert ops.KEY_SEARCH_SUM_LIMIT == 2 ** 62


def test_search_and_cli_argument_errors(tmp_path):
    acc = locate.ResidualAccumulator(8, 8, "cpu")
    with pytest.raises(ValueError, match="search_alpha"):
        keysearch.search(acc, first=0, count=4, search_alpha=0.0)
    with pytest.raises(ValueError, match="exactly one"):
        keysearch.search(acc, search_alpha=0.1)
    with pytest.raises(ValueError, match="exactly one"):
        keysearch.search(acc, keys=[1, 2], first=0, count=2, search_alpha=0.1)
    with pytest.raises(ValueError, match="both first and count"):
        keysearch.search(acc, first=0, search_alpha=0.1)
    with pytest.raises(ValueError, match="outside"):
        keysearch.search(acc, keys=[2 ** 64], search_alpha=0.1)
    with pytest.raises(ValueError, match="prefilter_rows"):
        keysearch.search(acc, first=0, count=4, search_alpha=0.1, prefilter_rows=9)
    with pytest.raises(ValueError, match="positive"):
        keysearch.search(acc, first=0, count=4, search_alpha=0.1, keep=0)
    assert keysearch.default_search_alpha(acc) == 1 / 64                                   # nothing accumulated: the floor
    acc.num.fill_(3 << 20)
    acc.den.fill_(1 << 32)                                                                 # every mean term 3/16
    assert keysearch.default_search_alpha(acc) == 3 / 16
    chunks = list(keysearch._Candidates(None, 2 ** 64 - 2, 5, "cpu").chunks())
    assert len(chunks) == 1 and chunks[0][0] == {"key_first": 2 ** 64 - 2, "count": 5} and chunks[0][1].tolist() == [-2, -1, 0, 1, 2]
    assert [kw["count"] for kw, _ in keysearch._Candidates(None, 7, keysearch.CHUNK_KEYS + 3, "cpu").chunks()] == [keysearch.CHUNK_KEYS, 3]
    assert keysearch._Candidates([1, 2 ** 63], None, None, "cpu").keys.tolist() == [1, -2 ** 63]
    f = tmp_path / "keys.txt"
    f.write_text("12\n0x1F\n\n 18446744073709551615 \n")
    assert keysearch.read_keys_file(f) == [12, 31, 2 ** 64 - 1]
    a = keysearch.parse_args(["--data", "d", "--alpha", ".2", "--first", "0x10", "--count", "256", "--out", "k.csv"])
    assert (a.data, a.stego_method, a.alpha, a.filter, a.first, a.count, a.keys_file, a.search_alpha, a.prefilter_rows, a.keep, a.key, a.out) == (
        "d", "LSBRK", 0.2, "KB", 16, 256, None, None, 0, 1024, None, "k.csv")
    a = keysearch.parse_args(["--data", "d", "--alpha", ".2", "--keys-file", str(f), "--search-alpha", ".1", "--prefilter-rows", "32", "--keep", "16",
                              "--key", "0xffffffffffffffff", "--filter", "OLSa", "--out", "k.csv"])
    assert a.keys_file == str(f) and a.search_alpha == 0.1 and a.prefilter_rows == 32 and a.keep == 16 and a.key == 2 ** 64 - 1 and a.filter == "OLSa"
    for bad in (["--data", "d", "--alpha", ".2", "--out", "k.csv"], ["--data", "d", "--alpha", ".2", "--first", "1", "--out", "k.csv"],
                ["--data", "d", "--alpha", ".2", "--first", "1", "--count", "2", "--keys-file", "f", "--out", "k.csv"]):
        with pytest.raises(SystemExit):
            keysearch.parse_args(bad)
