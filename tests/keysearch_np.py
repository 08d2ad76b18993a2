"""numpy-only restatement of the stego-key search (include/wsu.h K35, ws_unet_amd/ws/keysearch.py) on locate_np's Philox words.

frames: the (H-2,W-2) accumulators as zero-bordered (H,W) frames.  words / sums_under / key_sums: per key the wrapping int64 sums of the
two planes over the pixels i < count whose word under the key is below thr.  scores / standardise: the float64 mean snum * 256 / sden and its robust z."""
import numpy as np

import locate_np


def frames(num, den):
    return tuple(np.pad(np.asarray(p, dtype=np.int64), 1) for p in (num, den))


def words(count, keys):
    """(K, count) uint64: row j = the Philox words of pixels 0..count-1 under keys[j]"""
    return np.stack([locate_np._words(count, key) for key in keys])


def sums_under(wd, num, den, thr):
    """wd: `words` of the first wd.shape[1] entries of num / den (int64, linear frame order) -> (snum, sden) int64 (K,): per key the
    two's-complement sums over words < thr"""
    num, den = (np.ascontiguousarray(p, dtype=np.int64).reshape(-1).view(np.uint64)[:wd.shape[1]] for p in (num, den))
    on = wd < np.uint64(thr)
    snum = np.where(on, num[None], np.uint64(0)).sum(axis=1, dtype=np.uint64)                # (unsigned sums wrap silently)
    sden = np.where(on, den[None], np.uint64(0)).sum(axis=1, dtype=np.uint64)
    return snum.view(np.int64), sden.view(np.int64)


def key_sums(num, den, keys, thr, count=None):
    """num, den: int64 arrays read in linear (frame) order; keys: Python ints (any, taken mod 2^64); thr: 0..2^32; count: the first `count`
    entries only -> (snum, sden) int64 (K,), two's-complement sums"""
    count = np.asarray(num).size if count is None else int(count)
    return sums_under(words(count, keys), num, den, thr)


def key_range(first, count):
    return [(int(first) + j) % 2 ** 64 for j in range(count)]


def scores(snum, sden):
    return locate_np.residual_mean(np.asarray(snum), np.asarray(sden))


def standardise(score):
    """(score - median) / (1.4826 * MAD) over the finite scores; NaN stays NaN"""
    s = np.asarray(score, dtype=np.float64)
    ok = ~np.isnan(s)
    med = np.median(s[ok]) if ok.any() else np.nan
    mad = np.median(np.abs(s[ok] - med)) if ok.any() else np.nan
    with np.errstate(all="ignore"):
        return (s - med) / (1.4826 * mad)
