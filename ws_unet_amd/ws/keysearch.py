"""Searching for the stego key of a keyed embedder from WS residuals (J. Fridrich, M. Goljan, D. Soukal, "Searching for the stego-key",
Proc. SPIE 5306, 2004, with the per-pixel terms of A. D. Ker, MM&Sec 2008, as the evidence).  Not part of the reference.

ws.locate decides every pixel on its own and so needs many images under one key.  A key is ONE hypothesis about all pixels at once: the
per-pixel WS term r = (s - s_bar)(s - s_hat) has expectation 1/2 at a used pixel and 0 at an unused one, so the weighted mean of r over
the pixels a candidate key selects is about 1/2 for the right key and, for a wrong key, the whole image's mean term, about half the
change rate.  One image can suffice.  The whole cost is the scan over the candidates, ops.ws_key_search (K35): per key the sums of the two
accumulators of ws.locate's `ResidualAccumulator` over the pixels the key selects, exact integers.

The selection is nested in alpha: 'LSBRK' uses pixel i iff its Philox word under the key is below floor(alpha * 2^32), so a search
threshold BELOW the embedder's selects only used pixels, and the right key's mean stays at 1/2 whatever the true payload is; above it the
selection is diluted with unused pixels.  Hence `search_alpha` should err low: by default half of the payload the plain WS statistic
estimates from the accumulated images themselves, floored at 1/64 (fewer pixels, more noise).

`scores` / `standardise`: the mean in ws.locate's scale and its robust z over the searched keys, for numpy arrays and torch tensors.
`search`: one or two stages over a key list or a key range, walked in chunks.  `run`: a data set's stego images through locate.walk, then
the search; `python -m ws_unet_amd.ws.keysearch` writes the table.  Keys are raw 64-bit integers: hashing a passphrase into one, reading
the message out, and other embedders' key schedules are not here."""
from __future__ import annotations

import argparse
import pathlib
import typing

import numpy as np
import torch

from .. import ops
from . import locate, predictors

CHUNK_KEYS = 1 << 22                                       # keys per launch when a range is walked
NULL_KEYS = 4096                                           # two stages: candidates scanned over the whole frame for the z of the second stage
MIN_SEARCH_ALPHA = 1.0 / 64.0


# ---- the score and its standardisation: numpy arrays or torch tensors -------------------------------------------------------------

def scores(snum, sden):
    """int64 masked sums -> float64 snum * 256 / sden, the scale of locate.residual_mean (about 1/2 for the right key); NaN where sden = 0"""
    return locate.residual_mean(snum, sden)


def _median(x):
    """of a 1-D array / tensor without NaN, numpy's convention (the mean of the two middle values); NaN for none"""
    n = x.shape[0]
    if n == 0:
        return float("nan")
    s = torch.sort(x)[0] if isinstance(x, torch.Tensor) else np.sort(x)
    return float(s[(n - 1) // 2] + s[n // 2]) / 2.0


def null_of(score) -> typing.Tuple[float, float]:
    """(median, MAD) of the finite scores: the location and scale of the wrong keys, which nearly all keys are"""
    xp = torch if isinstance(score, torch.Tensor) else np
    s = score.reshape(-1)
    s = s[~xp.isnan(s)]
    med = _median(s)
    return med, _median(abs(s - med))


def standardise(score, null: typing.Optional[typing.Tuple[float, float]] = None):
    """(score - median) / (1.4826 * MAD), float64 of score's kind, the median and MAD over the searched keys (the finite scores) or the
    given `null` = (median, MAD); a NaN score stays NaN, MAD = 0 gives +-inf / NaN."""
    med, mad = null_of(score) if null is None else null
    if isinstance(score, torch.Tensor):
        return (score - med) / torch.tensor(1.4826 * mad, dtype=torch.float64, device=score.device)
    with np.errstate(all="ignore"):
        return (np.asarray(score, dtype=np.float64) - med) / np.float64(1.4826 * mad)


def hex_key(pattern: int) -> str:
    return f"0x{int(pattern) % 2 ** 64:016x}"


# ---- the search --------------------------------------------------------------------------------------------------------------------

def _patterns(values) -> torch.Tensor:
    """Python ints in [0, 2^64) -> int64 tensor holding their patterns"""
    vals = [int(v) for v in values]
    if any(not 0 <= v < 2 ** 64 for v in vals):
        raise ValueError("keysearch: a key outside [0, 2^64)")
    return torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64))


def _best(score: torch.Tensor, keys: torch.Tensor, m: int):
    """the m best (score descending, NaN last, the earlier candidate first among equals) of parallel tensors"""
    order = torch.sort(torch.where(torch.isnan(score), torch.full_like(score, -float("inf")), score), descending=True, stable=True)[1][:m]
    return score[order], keys[order]


class _Candidates:
    """A key list or a key range as chunks of at most CHUNK_KEYS keys: (keyword arguments of ops.ws_key_search, the keys as patterns)."""

    def __init__(self, keys, first, count, device):
        if (keys is None) == (first is None and count is None):
            raise ValueError("keysearch: give exactly one of keys and (first, count)")
        self.device = device
        if keys is not None:
            self.keys = (keys if isinstance(keys, torch.Tensor) else _patterns(keys)).to(device=device, dtype=torch.int64).reshape(-1)
            self.first, self.count = None, int(self.keys.shape[0])
        else:
            if first is None or count is None:
                raise ValueError("keysearch: a key range needs both first and count")
            self.keys, self.first, self.count = None, int(first), int(count)
            if not 0 <= self.first < 2 ** 64:
                raise ValueError(f"keysearch: first {first!r} outside [0, 2^64)")
        if self.count < 1:
            raise ValueError("keysearch: no candidate keys")

    def chunks(self, limit: typing.Optional[int] = None):
        total = self.count if limit is None else min(self.count, limit)
        for at in range(0, total, CHUNK_KEYS):
            n = min(CHUNK_KEYS, total - at)
            if self.keys is not None:
                part = self.keys[at:at + n]
                yield {"keys": part}, part
            else:
                start = (self.first + at) % 2 ** 64
                signed = start - 2 ** 64 if start >= 2 ** 63 else start
                yield {"key_first": start, "count": n}, torch.arange(n, dtype=torch.int64, device=self.device) + signed      # (wraps as the kernel's keys do)


def _scan(acc, cand: _Candidates, thr: int, rows, keep: int, limit=None, track=None):
    """One stage: all candidates (the first `limit`) scored over `rows` frame rows; only the running `keep` best are kept between chunks.
    -> (scores, keys) of the kept, best first; the first chunk's (median, MAD); how many candidates beat the score `track`."""
    best_s = torch.empty(0, dtype=torch.float64, device=acc.device)
    best_k = torch.empty(0, dtype=torch.int64, device=acc.device)
    null, above = None, 0
    for kw, keys in cand.chunks(limit):
        s = scores(*ops.ws_key_search(acc.num, acc.den, acc.h, acc.w, alpha_threshold=thr, rows=rows, **kw))
        if null is None:
            null = null_of(s)
        if track is not None:
            above += int((s > track).sum())
        best_s, best_k = _best(torch.cat([best_s, s]), torch.cat([best_k, keys]), keep)
    return best_s, best_k, null, above


def search(acc, *, keys=None, first: typing.Optional[int] = None, count: typing.Optional[int] = None, search_alpha: float,
           prefilter_rows: int = 0, keep: int = 1024, top: int = 10, key: typing.Optional[int] = None) -> typing.List[dict]:
    """The `top` best candidate keys for the sums of `acc` (a locate.ResidualAccumulator): rows {key ('0x...'), score, z, rank}, best first.
    Candidates: `keys` (Python ints or an int64 tensor of patterns) or the range first + j, j < count, mod 2^64, walked in chunks of at most
    2^22 keys with only the running best kept.  search_alpha: the payload whose pixels are scored (see the module's text: err low).
    prefilter_rows = R > 0: stage 1 scores the first R frame rows only over all candidates, stage 2 the whole frame over the `keep` best of
    stage 1 as an explicit list.  z: `standardise` against the wrong keys' median and MAD, taken from the first chunk (one stage) or from
    a whole-frame scan of the first 4096 candidates (two stages: the kept keys are no sample of the wrong ones).
    key: the true key, if known: every row gains true_key, true_score and true_rank (1 + the candidates scoring above it in the final
    stage; NaN when a prefilter dropped it)."""
    if not 0.0 < float(search_alpha) <= 1.0:
        raise ValueError(f"keysearch: search_alpha={search_alpha!r} outside (0, 1]")
    keep, top, rows = int(keep), int(top), int(prefilter_rows)
    if keep < 1 or top < 1:
        raise ValueError(f"keysearch: keep={keep} and top={top} must be positive")
    if rows < 0 or rows > acc.h:
        raise ValueError(f"keysearch: prefilter_rows={prefilter_rows} outside 0..{acc.h}")
    thr = ops.lsbr_key_threshold(search_alpha)
    cand = _Candidates(keys, first, count, acc.device)
    truth = None
    if key is not None:
        true_pat = _patterns([key]).to(acc.device)
        truth = float(scores(*ops.ws_key_search(acc.num, acc.den, acc.h, acc.w, keys=true_pat, alpha_threshold=thr))[0])
    two_stage = 0 < rows < acc.h
    if two_stage:
        _, kept, _, _ = _scan(acc, cand, thr, rows, keep)
        _, _, null, _ = _scan(acc, cand, thr, None, 1, limit=NULL_KEYS)
        final = _Candidates(kept, None, None, acc.device)
    else:
        final, null = cand, None
    s, k, first_null, above = _scan(acc, final, thr, None, max(top, 1), track=truth)
    null = first_null if null is None else null
    z = standardise(s, null)
    out = []
    for i, (kk, ss, zz) in enumerate(zip(k[:top].tolist(), s[:top].tolist(), z[:top].tolist())):
        row = {"key": hex_key(kk), "score": ss, "z": zz, "rank": i + 1}
        if key is not None:
            kept_true = not two_stage or bool((kept == true_pat).any())
            row |= {"true_key": hex_key(key), "true_score": truth, "true_rank": above + 1 if kept_true else float("nan")}
        out.append(row)
    return out


def default_search_alpha(acc) -> float:
    """Half of the payload the plain WS statistic estimates from the accumulated images: the weighted mean term over all pixels and images
    is the change rate beta_hat, the payload 2 beta_hat, so its half is beta_hat itself; floored at 1/64, at most 1."""
    beta = float(locate.residual_mean(acc.num.sum().reshape(1), acc.den.sum().reshape(1))[0])
    return min(1.0, max(MIN_SEARCH_ALPHA, beta)) if beta == beta else MIN_SEARCH_ALPHA


def run(input_dir: pathlib.Path, stego_method: str, alpha: float, model_name: str, model_path, channels: typing.Tuple[int] = (3,), *,
        keys=None, first: typing.Optional[int] = None, count: typing.Optional[int] = None, search_alpha: typing.Optional[float] = None,
        key: typing.Optional[int] = None, prefilter_rows: int = 0, keep: int = 1024, top: int = 10, weighted: int = 1, batched: bool = True,
        **kw):
    """Accumulates the WS terms of a data set's (stego_method, alpha) images -- one image or many of one size, any pixel predictor ws.locate
    knows (a named filter, 'OLSa' / 'OLSa2', 'JPEG', a trained UNet) -- and searches the candidate keys: a table of `search`'s rows with
    model_name, stego_method, alpha, images and search_alpha in front.  search_alpha None: `default_search_alpha`.  Other keywords go to the
    fabrika iterators (take_num_images, split, ...)."""
    import pandas as pd
    pixel_estimator, name = locate.pixel_predictor(model_name, model_path, channels)
    state = locate.walk(input_dir, stego_method, alpha, pixel_estimator, channels, weighted, (), batched, **kw)
    if state.acc is None:
        raise ValueError(f"keysearch: no {stego_method} images at alpha {alpha} under {input_dir}")
    sa = default_search_alpha(state.acc) if search_alpha is None else float(search_alpha)
    rows = search(state.acc, keys=keys, first=first, count=count, search_alpha=sa, prefilter_rows=prefilter_rows, keep=keep, top=top, key=key)
    head = {"model_name": name, "stego_method": stego_method, "alpha": alpha, "images": state.acc.images, "search_alpha": sa}
    return pd.DataFrame([head | r for r in rows])


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------

def _int(text: str) -> int:
    return int(text, 0)


def read_keys_file(path) -> typing.List[int]:
    """one decimal or 0x integer per line; blank lines are skipped"""
    return [int(ln.strip(), 0) for ln in pathlib.Path(path).read_text().splitlines() if ln.strip()]


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Search the stego key of a data set's keyed stego images from their WS residuals: a table of the "
                                             "best candidate keys, the best first.")
    ap.add_argument("--data", required=True, help="data set root with stego*/files.csv")
    ap.add_argument("--out", required=True, help="the table (CSV)")
    ap.add_argument("--stego-method", default="LSBRK")
    ap.add_argument("--alpha", type=float, required=True, help="the payload of the images to read (names their folder)")
    ap.add_argument("--filter", default="KB", help="one of the " + predictors.filters_help(structural=False))
    ap.add_argument("--first", type=_int, default=None, help="the first key of a range (decimal or 0x)")
    ap.add_argument("--count", type=_int, default=None, help="the number of keys of the range")
    ap.add_argument("--keys-file", default=None, help="candidate keys, one decimal or 0x integer per line")
    ap.add_argument("--search-alpha", type=float, default=None, help="payload whose pixels are scored; default: half the WS estimate, at least 1/64")
    ap.add_argument("--prefilter-rows", type=int, default=0, help="stage 1 scores these first rows only; 0: one stage")
    ap.add_argument("--keep", type=int, default=1024, help="candidates stage 1 hands to stage 2")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--key", type=_int, default=None, help="the true key, if known: adds its score and rank")
    ap.add_argument("--weighted", type=int, choices=(0, 1), default=1)
    ap.add_argument("--per-image", action="store_true", help="use the per-image iterator instead of the batched one")
    predictors.add_arguments(ap)
    a = ap.parse_args(argv)
    if (a.keys_file is None) == (a.first is None and a.count is None) or (a.keys_file is None and (a.first is None or a.count is None)):
        ap.error("give either --first and --count or --keys-file")
    return a


def main(argv=None) -> None:
    a = parse_args(argv)
    predictors.register_from_args(a)
    keys = read_keys_file(a.keys_file) if a.keys_file else None
    res = run(pathlib.Path(a.data), a.stego_method, a.alpha, a.filter, None, (3,), keys=keys, first=a.first, count=a.count,
              search_alpha=a.search_alpha, key=a.key, prefilter_rows=a.prefilter_rows, keep=a.keep, top=a.top, weighted=a.weighted,
              batched=not a.per_image)
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res.to_csv(out, index=False)
    print(f"output saved to {out}")


if __name__ == "__main__":
    main()
