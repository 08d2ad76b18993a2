"""GPU: the stego-key scan (K35, ops.ws_key_search) against numpy (keysearch_np), equal as integers in every case; its launch shapes;
the search of ws.keysearch end to end on crops of the golden covers, in one and in two stages; the CLI."""
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import keysearch_np
import locate_np
from ws_unet_amd import embed, filters, ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import keysearch, locate

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
KB = np.asarray(filters.NAMED_FILTERS_2D["KB"])[..., 0]
AVG = np.asarray(filters.NAMED_FILTERS_2D["AVG"])[..., 0]
FRAMES = [(3, 3), (4, 5), (11, 13), (16, 16), (33, 7)]     # one interior pixel; ...; quads straddle rows and the border; whole quads; a narrow one
COUNTS = (1, 255, 256, 257, 600)                           # keys: below, at and above one workgroup of 256, and three workgroups
T05 = int(np.floor(.05 * 2.0 ** 32))
THRESHOLDS = (0, 1, T05, 2 ** 31, 2 ** 32)
FIRST = 2 ** 32 - 100                                      # the end-to-end range: its keys carry into the high word ...
KEY = FIRST + 97                                           # ... before the true one
SEEDS = [(35 << 32) | i for i in range(5)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _planes(h, w, seed):
    """random int64 num of both signs up to 2^40, den up to 2^34"""
    rng = np.random.default_rng(seed)
    return rng.integers(-2 ** 40, 2 ** 40, (h - 2, w - 2), dtype=np.int64), rng.integers(0, 2 ** 34, (h - 2, w - 2), dtype=np.int64)


def _pat(keys):
    return _dev(np.array([k % 2 ** 64 for k in keys], dtype=np.uint64).view(np.int64))


def _got(num, den, h, w, **kw):
    snum, sden = ops.ws_key_search(_dev(num), _dev(den), h, w, **kw)
    assert snum.dtype == torch.int64 and sden.dtype == torch.int64 and snum.is_cuda and snum.shape == sden.shape and snum.dim() == 1
    return snum.cpu().numpy(), sden.cpu().numpy()


def _assert_equal(got, want, what):
    for name, g, w in zip(("snum", "sden"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


# ---- K35 against the restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", FRAMES)
def test_sums_equal_numpy_as_integers(frame):
    """every frame x every threshold on 600 keys of a range and of the same keys as a list; every key count at thr = .05 * 2^32"""
    h, w = frame
    num, den = _planes(h, w, 11 * h + w)
    fn, fd = keysearch_np.frames(num, den)
    first = 77 + h
    keys = keysearch_np.key_range(first, 600)
    wd = keysearch_np.words(h * w, keys)
    for thr in THRESHOLDS:
        want = keysearch_np.sums_under(wd, fn, fd, thr)
        _assert_equal(_got(num, den, h, w, key_first=first, count=600, alpha_threshold=thr), want, f"range thr {thr}")
        _assert_equal(_got(num, den, h, w, keys=_pat(keys), alpha_threshold=thr), want, f"list thr {thr}")
        if thr == 0:
            assert not want[0].any() and not want[1].any()
        if thr == 2 ** 32:
            assert (want[0] == num.sum()).all() and (want[1] == den.sum()).all()
    want = keysearch_np.sums_under(wd, fn, fd, T05)
    for k in COUNTS:
        _assert_equal(_got(num, den, h, w, key_first=first, count=k, alpha_threshold=T05), [p[:k] for p in want], f"range of {k}")
        _assert_equal(_got(num, den, h, w, keys=_pat(keys[:k]), alpha_threshold=T05), [p[:k] for p in want], f"list of {k}")


@pytest.mark.parametrize("first", [2 ** 32 - 3, 2 ** 64 - 2])
def test_key_ranges_carry_into_the_high_word_and_wrap(first):
    h, w = 11, 13
    num, den = _planes(h, w, 5)
    fn, fd = keysearch_np.frames(num, den)
    keys = keysearch_np.key_range(first, 8)
    assert keys[3] in (2 ** 32, 1)
    for thr in (T05, 2 ** 31):
        want = keysearch_np.key_sums(fn, fd, keys, thr)
        _assert_equal(_got(num, den, h, w, key_first=first, count=8, alpha_threshold=thr), want, f"range from {first}")
        _assert_equal(_got(num, den, h, w, keys=_pat(keys), alpha_threshold=thr), want, f"the same keys as a list from {first}")
    assert len({int(v) for v in want[1]}) == 8                                             # eight keys, eight selections


def test_key_list_with_duplicates_and_keys_differing_in_the_high_word():
    h, w = 16, 16
    num, den = _planes(h, w, 6)
    fn, fd = keysearch_np.frames(num, den)
    keys = [5, 5, 5 + 2 ** 32, 5 + 2 ** 63, 2 ** 64 - 1, 0, 5, 2 ** 63]
    for thr in (T05, 2 ** 31):
        want = keysearch_np.key_sums(fn, fd, keys, thr)
        got = _got(num, den, h, w, keys=_pat(keys), alpha_threshold=thr)
        _assert_equal(got, want, f"list thr {thr}")
        assert got[1][0] == got[1][1] == got[1][6] and len({int(got[1][i]) for i in (0, 2, 3, 4, 5, 7)}) == 6


# ---- the launch shape --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", [(11, 13), (33, 7), (64, 64)])
def test_parts_and_rows_give_the_restatement(frame):
    """parts 1 (plain stores), 2, 7 (atomics, ragged slices), more than there are quads, and the automatic choice: identical bits; rows = 1
    reads the top border only, rows = H - 1 all but the bottom border: the restatement on the prefix"""
    h, w = frame
    num, den = _planes(h, w, 7 * h)
    fn, fd = keysearch_np.frames(num, den)
    keys = keysearch_np.key_range(2 ** 40, 300)
    wd = keysearch_np.words(h * w, keys)
    want = keysearch_np.sums_under(wd, fn, fd, 2 ** 31)
    quads = (h * w + 3) // 4
    for parts in (0, 1, 2, 7, quads, quads + 5, 65535):
        _assert_equal(_got(num, den, h, w, key_first=2 ** 40, count=300, alpha_threshold=2 ** 31, parts=parts), want, f"range parts {parts}")
        _assert_equal(_got(num, den, h, w, keys=_pat(keys), alpha_threshold=2 ** 31, parts=parts), want, f"list parts {parts}")
    for rows in (1, 2, h - 1, h):
        want = keysearch_np.sums_under(wd[:, :rows * w], fn, fd, 2 ** 31)
        for parts in (0, 1, 3):
            _assert_equal(_got(num, den, h, w, key_first=2 ** 40, count=300, alpha_threshold=2 ** 31, rows=rows, parts=parts), want,
                          f"rows {rows} parts {parts}")
        if rows == 1:
            assert not want[0].any() and not want[1].any()


def test_c_entry_adds_in_wrapping_int64_and_zeroes_its_outputs():
    """the definition of the sums on planes the op's guard would refuse: 3 * 2^62 + 4 wraps (two quads, the second partial); outputs filled
    beforehand are overwritten"""
    lib = ops._lib.load()
    num = _dev(np.array([2 ** 62, 2 ** 62, 2 ** 62, -5, 9], dtype=np.int64))
    den = _dev(np.array([2 ** 63 - 1, 1, 0, 0, 9], dtype=np.int64))
    for parts in (1, 2):
        snum = torch.full((3,), 12345, dtype=torch.int64, device=DEV)
        sden = torch.full((3,), -6, dtype=torch.int64, device=DEV)
        ops.check(lib.wsu_ws_key_search(num.data_ptr(), den.data_ptr(), 5, None, 2 ** 64 - 1, 1, 3, 2 ** 32, parts, snum.data_ptr(), sden.data_ptr(),
                                        ops._stream()), "wsu_ws_key_search")
        assert snum.tolist() == [3 * 2 ** 62 + 4 - 2 ** 64] * 3 and sden.tolist() == [9 - 2 ** 63] * 3
        ops.check(lib.wsu_ws_key_search(num.data_ptr(), den.data_ptr(), 5, None, 0, 1, 3, 0, parts, snum.data_ptr(), sden.data_ptr(), ops._stream()),
                  "wsu_ws_key_search")
        assert snum.tolist() == [0, 0, 0] == sden.tolist()


# ---- the same selection as K30 -------------------------------------------------------------------------------------------------

def test_sums_are_the_sums_under_the_mask_of_the_keyed_simulator():
    h, w = 33, 7
    num, den = _planes(h, w, 8)
    keys = [2008, 2 ** 32 + 2008, 2 ** 64 - 1, 0]
    for thr in (T05, ops.lsbr_key_threshold(0.5)):
        snum, sden = ops.ws_key_search(_dev(num), _dev(den), h, w, keys=_pat(keys), alpha_threshold=thr)
        for j, key in enumerate(keys):
            mask = ops.lsbr_key_mask(key, thr, h, w)[1:-1, 1:-1].to(torch.int64)
            assert int(snum[j]) == int((mask * _dev(num)).sum()) and int(sden[j]) == int((mask * _dev(den)).sum())


# ---- the op's checks -----------------------------------------------------------------------------------------------------------

def test_op_overflow_guard_and_argument_checks_on_the_device():
    h, w = 8, 8
    num, den = (_dev(p) for p in _planes(h, w, 9))
    ok = dict(key_first=0, count=4, alpha_threshold=7)
    big = torch.zeros_like(num)
    big[0, 0], big[5, 5] = 2 ** 61, -2 ** 61                                               # |.| sums to 2^62 although the plain sum is 0
    with pytest.raises(ValueError, match=r"\|num\| is 2\^62 or more"):
        ops.ws_key_search(big, den, h, w, **ok)
    with pytest.raises(ValueError, match=r"\|den\| is 2\^62 or more"):
        ops.ws_key_search(num, big.abs(), h, w, **ok)
    big[5, 5] += 1                                                                          # 2^62 - 1: allowed
    snum, sden = ops.ws_key_search(big, den, h, w, key_first=0, count=4, alpha_threshold=2 ** 32)
    assert snum.tolist() == [1] * 4 and sden.tolist() == [int(den.sum())] * 4
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_key_search(num, den, h, w, alpha_threshold=7)
    with pytest.raises(ValueError, match="exactly one"):
        ops.ws_key_search(num, den, h, w, keys=_pat([1]), key_first=0, count=1, alpha_threshold=7)
    with pytest.raises(ValueError, match="rows"):
        ops.ws_key_search(num, den, h, w, rows=h + 1, **ok)
    with pytest.raises(ValueError, match="shape"):
        ops.ws_key_search(num, den, h, w + 1, **ok)
    with pytest.raises(ops._lib.WsuError, match="CPU tensor"):
        ops.ws_key_search(num, den, h, w, keys=torch.zeros(3, dtype=torch.int64), alpha_threshold=7)
    strided = _dev(np.arange(8, dtype=np.int64))[::2]                                       # a strided key list is made contiguous
    a = ops.ws_key_search(num, den, h, w, keys=strided, alpha_threshold=2 ** 31)
    b = ops.ws_key_search(num, den, h, w, keys=strided.clone(), alpha_threshold=2 ** 31)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- end to end on the golden covers -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crops():
    return np.stack([np.ascontiguousarray(imread4_u8(GOLDEN / f"cover_{k}.png")[..., 3])[:64, :64] for k in COVERS])


@pytest.fixture(scope="module")
def accumulated(crops):
    """the 64 x 64 top-left crops of the five golden covers, LSBRK at alpha 0.2 under KEY, accumulated with KB, weighted, the project's AVG;
    the accumulators equal the restatement's"""
    sd = torch.tensor(np.array(SEEDS, dtype=np.uint64).view(np.int64)).to(DEV)
    stego = ops.embed_lsbr_keyed(_dev(crops), sd, KEY, ops.lsbr_key_threshold(0.2))[0]
    twins = stego.cpu().numpy()
    np.testing.assert_array_equal(twins[3], locate_np.lsbrk_np(crops[3], 0.2, SEEDS[3], KEY))
    acc = locate.ResidualAccumulator(64, 64, DEV).add(stego, filters.get_filter_estimator(filter_name="KB", flatten=False), weighted=1)
    num, den = locate_np.accumulate(twins, pixel_kernels=[KB] * 5, mean_kernel=AVG, weighted=1)
    np.testing.assert_array_equal(acc.num.cpu().numpy(), num)
    np.testing.assert_array_equal(acc.den.cpu().numpy(), den)
    return acc, num, den


def test_search_finds_the_key_among_256(accumulated):
    """The restatement alone on the CPU, with the project's AVG as the mean kernel: the true key scores 0.50056, the runner-up 0.17301
    (z 12.4 against 2.4).  The margin is not asserted, the order is."""
    acc, num, den = accumulated
    thr = ops.lsbr_key_threshold(0.1)
    want = keysearch_np.key_sums(*keysearch_np.frames(num, den), keysearch_np.key_range(FIRST, 256), thr)
    got = ops.ws_key_search(acc.num, acc.den, 64, 64, key_first=FIRST, count=256, alpha_threshold=thr)
    _assert_equal([g.cpu().numpy() for g in got], want, "the scan of the search")
    score = keysearch_np.scores(*want)
    order = np.argsort(-score, kind="stable")
    print("true key", score[97], "runner-up", score[order[1]], "z", keysearch_np.standardise(score)[order[:2]])
    assert order[0] == 97                                                                   # the restatement ranks it first, ...
    rows = keysearch.search(acc, first=FIRST, count=256, search_alpha=0.1, top=5, key=KEY)
    assert [r["rank"] for r in rows] == [1, 2, 3, 4, 5] and rows[0]["key"] == keysearch.hex_key(KEY) == f"0x{KEY:016x}"       # ... and so does the search
    assert [r["key"] for r in rows] == [keysearch.hex_key(FIRST + int(j)) for j in order[:5]]
    assert [r["score"] for r in rows] == score[order[:5]].tolist()
    np.testing.assert_array_equal([r["z"] for r in rows], keysearch_np.standardise(score)[order[:5]])
    assert all(r["true_key"] == rows[0]["key"] and r["true_rank"] == 1 and r["true_score"] == score[97] for r in rows)
    listed = keysearch.search(acc, keys=keysearch_np.key_range(FIRST, 256), search_alpha=0.1, top=5)
    assert listed == [{k: r[k] for k in ("key", "score", "z", "rank")} for r in rows]


def test_search_in_chunks_keeps_the_running_best(accumulated, monkeypatch):
    acc, _, _ = accumulated
    whole = keysearch.search(acc, first=FIRST, count=256, search_alpha=0.1, top=7, key=KEY)
    monkeypatch.setattr(keysearch, "CHUNK_KEYS", 60)                                        # five launches, the last one ragged
    parts = keysearch.search(acc, first=FIRST, count=256, search_alpha=0.1, top=7, key=KEY)
    assert [(r["key"], r["score"], r["rank"], r["true_rank"]) for r in parts] == [(r["key"], r["score"], r["rank"], r["true_rank"]) for r in whole]
    assert parts[0]["key"] == keysearch.hex_key(KEY)                                        # (z differs: it is taken against the first chunk)


def test_two_stage_search_returns_the_same_top_key(accumulated):
    acc, num, den = accumulated
    one = keysearch.search(acc, first=FIRST, count=256, search_alpha=0.1, top=3, key=KEY)
    two = keysearch.search(acc, first=FIRST, count=256, search_alpha=0.1, prefilter_rows=32, keep=16, top=3, key=KEY)
    assert two[0]["key"] == one[0]["key"] == keysearch.hex_key(KEY) and two[0]["score"] == one[0]["score"] and two[0]["true_rank"] == 1
    # stage 1 is the restatement's ranking on the first 32 rows; stage 2 re-scores its 16 best over the whole frame
    fn, fd = keysearch_np.frames(num, den)
    keys = keysearch_np.key_range(FIRST, 256)
    thr = ops.lsbr_key_threshold(0.1)
    kept = np.argsort(-keysearch_np.scores(*keysearch_np.key_sums(fn, fd, keys, thr, count=32 * 64)), kind="stable")[:16]
    full = keysearch_np.scores(*keysearch_np.key_sums(fn, fd, [keys[j] for j in kept], thr))
    best = np.argsort(-full, kind="stable")[:3]
    assert [r["key"] for r in two] == [keysearch.hex_key(keys[kept[j]]) for j in best] and [r["score"] for r in two] == full[best].tolist()
    gone = keysearch.search(acc, first=FIRST, count=256, search_alpha=0.1, prefilter_rows=1, keep=2, top=3, key=KEY)    # the top border says nothing
    assert np.isnan(gone[0]["true_rank"]) and gone[0]["key"] != keysearch.hex_key(KEY)


def test_default_search_alpha_is_half_the_estimated_payload(accumulated):
    acc, num, den = accumulated
    beta = float(locate_np.residual_mean(np.array([num.sum()]), np.array([den.sum()]))[0])
    assert keysearch.default_search_alpha(acc) == max(1 / 64, beta) and 0.0 < beta < 0.2   # a change rate: below the payload 0.2


# ---- the CLI -----------------------------------------------------------------------------------------------------------------

def test_cli_finds_the_key_of_a_written_data_set(tmp_path, capsys):
    """the five golden covers, their LSBRK twins written by the embed CLI, and the search over a range and over a keys file"""
    root = tmp_path / "data"
    (root / "images").mkdir(parents=True)
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    embed.main(["--data", str(root), "--stego-method", "LSBRK", "--alphas", "0.2", "--key", str(KEY)])
    out = tmp_path / "out" / "keys.csv"
    keysearch.main(["--data", str(root), "--stego-method", "LSBRK", "--alpha", "0.2", "--filter", "KB", "--first", hex(FIRST), "--count", "256",
                    "--prefilter-rows", "64", "--keep", "32", "--key", str(KEY), "--out", str(out)])
    assert f"output saved to {out}" in capsys.readouterr().out
    import pandas as pd
    table = pd.read_csv(out)
    assert list(table.columns) == ["model_name", "stego_method", "alpha", "images", "search_alpha", "key", "score", "z", "rank", "true_key",
                                   "true_score", "true_rank"]
    assert table["key"][0] == keysearch.hex_key(KEY) and table["rank"].tolist() == list(range(1, 11)) and table["true_rank"][0] == 1
    assert (table["images"] == 5).all() and (table["model_name"] == "KB").all() and 1 / 64 <= table["search_alpha"][0] <= 1
    listed = tmp_path / "keys.txt"
    listed.write_text("".join(f"{FIRST + j}\n" if j % 2 else f"{hex(FIRST + j)}\n" for j in range(90, 110)))
    keysearch.main(["--data", str(root), "--alpha", "0.2", "--keys-file", str(listed), "--search-alpha", "0.1", "--top", "3", "--out", str(out)])
    table = pd.read_csv(out)
    assert table["key"][0] == keysearch.hex_key(KEY) and len(table) == 3 and "true_key" not in table.columns
