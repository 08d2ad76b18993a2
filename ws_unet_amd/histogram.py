"""The histogram attacks: the oldest untrained baselines of the two embedding families this package simulates.  Not part of the reference.

    python -m ws_unet_amd.histogram score --data DIR --detector HCF2C --stego-methods LSBM --alphas 1.0 [--split S] [--simulate] --out scores.csv
    python -m ws_unet_amd.histogram curve --data DIR [--stego-method LSBRS --alpha 0.3 [--simulate]] [--segments 100] [--order rows|rows_up] --out chi2_curve.csv
    python -m ws_unet_amd.ws.roc --data DIR --out-dir OUT --scores scores.csv B0_HCF2C

  * The chi-square attack (A. Westfeld, A. Pfitzmann, "Attacks on steganographic systems", IH 1999) tests the pairs of values (2k, 2k+1),
    which LSB replacement of a full message equalises.  Its p-value along the file order (`curve`) is the classical detector and length
    estimator (`length`) of SEQUENTIAL LSB replacement: what `embed --stego-method LSBRS` writes and `ws.estimate --placement sequential`
    attacks.
  * The histogram characteristic function centre of mass (HCF-COM; J. Harmsen, W. Pearlman, SPIE 2003) with the calibrated and adjacency
    variants of A. Ker ("Steganalysis of LSB matching in grayscale images", IEEE SPL 12(6), 2005): the classical targeted detectors of LSB
    matching (`embed_pm1`'s LSBM), which adds noise and so pulls the centre of mass of the histogram's DFT towards 0.

The package's pattern for per-image statistics: the device counts exact integers -- ops.hist_segments (K58), ops.adjacency_hist (K59), and
both again on the calibration image of ops.downsample2x2 (K60) -- and a few float64 operations follow.  `chi2` and `length` run on the host;
`com` and `com2` take their DFT with torch.fft, on the device when their input lives there: the FFT is torch's, not a kernel of this library.

`score` writes the schema of results/detection/b0.csv, which `ws.roc --scores FILE NAME` takes unchanged (NAME must contain 'B0').  The
detectors are not change-rate estimators and are no rows of ws/predictors.py.

Not checked: no other implementation of either attack was at hand.  As remembered, and unverified: the DFT range k = 0..127 of the centre
of mass (the half below the Nyquist index); k + l as the weight of the two-dimensional one; dropping the pairs of values with fewer than
`min_pair` pixels from the chi-square statistic, where some implementations merge neighbouring categories instead.
"""
from __future__ import annotations

import argparse
import logging
import typing
import warnings

import numpy as np
import torch

from . import fabrika, spam

DETECTORS = ("CHI2", "HCF", "HCFC", "HCF2", "HCF2C")
CSV_COLUMNS = spam.CSV_COLUMNS
SIMULATED = spam.SIMULATED
# `prediction` of `score`: output > threshold.  Conventions, not fitted: 0.5 for a p-value, 1 (no change under calibration) for the ratios,
# none for the uncalibrated centres of mass, whose scale differs from image to image.
THRESHOLDS = {"CHI2": 0.5, "HCFC": 1.0, "HCF2C": 1.0, "HCF": None, "HCF2": None}


def _f64(t, device=None) -> torch.Tensor:
    t = t.detach() if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t, dtype=np.float64))      # (a Python float is not to pass through float32)
    return t.to(device=t.device if device is None else device, dtype=torch.float64)


_GAMMA_CAP = 100000


def gammaincc(a, x) -> torch.Tensor:
    """Q(a, x), the regularised upper incomplete gamma function, element by element in float64 (a > 0, x >= 0): the series of P = 1 - Q
    where x < a + 1, the continued fraction of Q (modified Lentz) beyond, both times the prefactor exp(-x + a ln x - lgamma(a)).  Its own
    few lines because torch.special.gammaincc is not good to 1e-9 in the bulk: at a = 38.5, x = 48.05 it returns 0.06939346292930 where
    scipy.special.gammaincc and this function give 0.06939346282759, 1.5e-9 off in relative terms (tests/test_histogram_host.py compares).
    Both branches run on every element and the loops end when ALL elements have converged, so one slow element keeps its whole batch
    iterating: right for the N x S values of a curve (a few hundred passes at most for dof <= 127), not for millions.  A loop that reaches
    its cap of _GAMMA_CAP passes warns."""
    a, x = torch.broadcast_tensors(_f64(a, "cpu"), _f64(x, "cpu"))
    series = x < a + 1.
    xs = torch.where(series, x, torch.zeros_like(x))                   # each branch runs on harmless values where the other one holds
    xc = torch.where(series, a + 1., x)
    term = 1. / a
    total = term.clone()
    for n in range(1, _GAMMA_CAP):
        term = term * xs / (a + n)
        total = total + term
        if bool((term.abs() <= total.abs() * 1e-16).all()):
            break
    else:
        warnings.warn(f"gammaincc: the series has not converged after {_GAMMA_CAP} terms")
    tiny = 1e-300
    b = xc + 1. - a
    c, d = torch.full_like(b, 1. / tiny), 1. / b
    f = d.clone()
    done = torch.zeros_like(series)                                    # sticky: a converged element may still flicker by an ulp
    for i in range(1, _GAMMA_CAP):
        an = -i * (i - a)
        b = b + 2.
        d = an * d + b
        d = torch.where(d.abs() < tiny, torch.full_like(d, tiny), d)
        c = b + an / c
        c = torch.where(c.abs() < tiny, torch.full_like(c, tiny), c)
        d = 1. / d
        delta = d * c
        f = f * delta
        done = done | ((delta - 1.).abs() < 1e-15)
        if bool(done.all()):
            break
    else:
        warnings.warn(f"gammaincc: the continued fraction has not converged after {_GAMMA_CAP} passes")
    pre = torch.exp(-x + a * torch.log(x.clamp(min=tiny)) - torch.lgamma(a))
    return torch.where(x <= 0., torch.ones_like(x), torch.where(series, 1. - total * pre, f * pre))


def chi2(h, min_pair: int = 10):
    """h: (..., 256) histogram(s), a numpy array or a torch tensor -> (statistic, dof, p), numpy arrays of the leading shape (float64,
    int64, float64).  n_k = h[2k] + h[2k+1]; pair k is kept iff n_k >= min_pair (an expected count of at least min_pair / 2 in both cells;
    sparser pairs are dropped, not merged); statistic = sum over the kept pairs of (h[2k] - h[2k+1])^2 / (2 n_k), which is
    sum (h[2k] - n_k/2)^2 / (n_k/2); dof = kept - 1; p = Q(dof / 2, statistic / 2), the regularised upper incomplete gamma function
    (`gammaincc` of this module, float64 on the host): the 'probability of embedding'.  p = 0 where dof < 1."""
    t = _f64(h, "cpu")
    if t.shape[-1] != 256:
        raise ValueError(f"chi2: last dimension {t.shape[-1]}, expected 256 bins")
    even, odd = t[..., 0::2], t[..., 1::2]
    n = even + odd
    keep = n >= min_pair
    stat = torch.where(keep, (even - odd) ** 2 / (2. * n.clamp(min=1.)), torch.zeros_like(n)).sum(-1)
    dof = keep.sum(-1) - 1
    p = torch.where(dof >= 1, gammaincc(dof.clamp(min=1).to(torch.float64) / 2., stat / 2.), torch.zeros_like(stat))
    return stat.numpy(), dof.numpy(), p.numpy()


def curve(x_u8: torch.Tensor, segments: int = 100, order: str = "rows", min_pair: int = 10) -> np.ndarray:
    """x_u8: (N,H,W) uint8 on the device -> p (N,S) float64: p[:, j] is `chi2` of the histogram of the first ceil((j+1) H W / S) pixels of
    the path (ops.hist_segments, summed up over the segments)."""
    from . import ops
    return chi2(ops.hist_segments(x_u8, segments, order).cumsum(1), min_pair)[2]


def length(p, threshold: float = 0.5) -> np.ndarray:
    """p: (..., S) p-values of the prefixes of a path -> the number of leading prefixes with p >= threshold, divided by S: the estimated
    fraction of the path that carries a message (an overestimate, as the p-value falls only some way past the message's end)."""
    ok = np.asarray(p) >= threshold
    return np.cumprod(ok, axis=-1).sum(axis=-1) / ok.shape[-1]


def com(h) -> np.ndarray:
    """h: (..., 256) histogram(s) -> C = sum_{k=0}^{127} k |F[k]| / sum_{k=0}^{127} |F[k]|, F the length-256 DFT of h (torch.fft in
    float64, on the device of h); NaN for an all-zero histogram."""
    t = _f64(h)
    if t.shape[-1] != 256:
        raise ValueError(f"com: last dimension {t.shape[-1]}, expected 256 bins")
    mag = torch.fft.fft(t, dim=-1)[..., :128].abs()
    k = torch.arange(128, dtype=torch.float64, device=t.device)
    return ((mag * k).sum(-1) / mag.sum(-1)).cpu().numpy()


def com2(A) -> np.ndarray:
    """A: (..., 256, 256) adjacency histogram(s) -> C2 = sum_{k,l=0}^{127} (k + l) |F2[k,l]| / sum |F2[k,l]|, F2 the 256 x 256 DFT of A
    (torch.fft in float64, on the device of A)."""
    t = _f64(A)
    if tuple(t.shape[-2:]) != (256, 256):
        raise ValueError(f"com2: last dimensions {tuple(t.shape[-2:])}, expected (256, 256)")
    mag = torch.fft.fft2(t, dim=(-2, -1))[..., :128, :128].abs()
    k = torch.arange(128, dtype=torch.float64, device=t.device)
    return ((mag * (k[:, None] + k[None, :])).sum((-2, -1)) / mag.sum((-2, -1))).cpu().numpy()


def check_detector(detector: str) -> str:
    if detector not in DETECTORS:
        raise ValueError(f"unknown detector {detector!r}; choose from {DETECTORS}")
    return detector


def tables(x_u8: torch.Tensor, detector: str):
    """the count tables that `detector` is made of, all on the device: the histogram or the adjacency histogram of the planes and, for the
    calibrated ratios, of their ops.downsample2x2 image"""
    from . import ops
    check_detector(detector)
    count = (lambda x: ops.adjacency_hist(x)) if detector.startswith("HCF2") else (lambda x: ops.hist_segments(x)[:, 0])
    return (count(x_u8), count(ops.downsample2x2(x_u8))) if detector.endswith("C") else (count(x_u8),)


def from_tables(tabs, detector: str) -> np.ndarray:
    """the scores of `outputs` from the tables of `tables`"""
    check_detector(detector)
    if detector == "CHI2":
        return chi2(tabs[0])[2]
    c = com2 if detector.startswith("HCF2") else com
    return c(tabs[1]) / c(tabs[0]) if detector.endswith("C") else -c(tabs[0])


def outputs(x_u8: torch.Tensor, detector: str) -> np.ndarray:
    """x_u8: (N,H,W) uint8 on the device -> (N,) float64, one score per image; higher means 'more likely stego'.
    'CHI2': p of `chi2` of the whole image's histogram.  'HCF': -C(h), `com` of the histogram.  'HCF2': -C2(A), `com2` of the adjacency
    histogram.  'HCFC': C(h') / C(h) and 'HCF2C': C2(A') / C2(A) with h', A' of the image ops.downsample2x2(x): +-1 embedding lowers the
    numerator of Ker's ratio C(h) / C(h') and leaves the calibration image's nearly alone, so the inverse rises."""
    return from_tables(tables(x_u8, detector), detector)


# ---- a data set ------------------------------------------------------------------------------------------------------------------------

def _submit(fnames, clean, *, detector=None, path=None, twin=None, prefetched=None):
    """Upload the chunk's Y planes once, make their twins when asked (spam.device_planes), queue the count kernels of `detector` or, with
    path = (segments, order), K58 along the path; nothing waits for the GPU."""
    from . import ops
    work = []
    for x, _ in spam.device_planes(fnames, twin, prefetched):
        work.append(tables(x, detector) if path is None else ops.hist_segments(x, *path))
    return clean, work, detector


def _collect(handle):
    clean, work, detector = handle
    if detector is not None:
        value = np.concatenate([from_tables(t, detector) for t in work])
    else:
        value = np.concatenate([t.cumsum(1).cpu().numpy() for t in work])
    return [{**kw, "value": value[i]} for i, kw in enumerate(clean)]


def _chunk(fnames, kws, prefetched=None, **shared):
    return _collect(_submit(fnames, kws, prefetched=prefetched, **shared))


_chunk.submit, _chunk.collect = _submit, _collect
_chunk = fabrika.shared_kwargs(_chunk, ("detector", "path", "twin"), spam._prefetch)


def _iterators(batch_size: int):
    kw = dict(iterator="batched", convert_to=None, ignore_missing=True, batch_size=batch_size)
    return fabrika.precovers(**kw)(_chunk), fabrika.stego_spatial(**kw)(_chunk)


def _pair(stego_method, alpha, who):
    if (stego_method is None) != (alpha is None):
        raise ValueError(f"{who}: give both stego_method and alpha, or neither (the covers)")


def extract(data_dir, detector: str, stego_method: typing.Optional[str] = None, alpha: typing.Optional[float] = None, *, split=None,
            simulate: bool = False, stream: int = 0, batch_size: int = 32, progress_on: bool = False, **kw):
    """(rows, output): the file rows (name, height, width, stego_method, alpha) and `outputs` of the Y plane of the covers of `data_dir`
    (stego_method None) or of one stego folder, through the fabrika iterators of spam.extract: batched, decoded a chunk ahead.
    simulate=True makes LSBR / HILLR / LSBM / HILL twins of the covers on the device instead (spam.file_set)."""
    check_detector(detector)
    _pair(stego_method, alpha, "extract")
    res = spam.file_set(*_iterators(batch_size), data_dir, stego_method, alpha, simulate, stream, detector=detector, split=split,
                        progress_on=progress_on, **kw)
    return spam.file_rows(res, ("value",)), np.array([r["value"] for r in res], dtype=np.float64)


def score(data_dir, detector: str, stego_methods, alphas, *, split=None, simulate: bool = False, stream: int = 0, batch_size: int = 32, **kw):
    """The frame of results/detection/b0.csv (spam.CSV_COLUMNS): the covers (empty stego_method and alpha), then the stegos method by
    method and alpha by alpha; output = `outputs` of the image.  prediction = output > 0.5 for 'CHI2', output > 1.0 for the ratios 'HCFC'
    and 'HCF2C', False for 'HCF' and 'HCF2'.  These thresholds are conventions, not fitted: a p-value's middle, and the ratio of an image
    whose centre of mass calibration leaves alone."""
    import pandas as pd
    check_detector(detector)
    thr = THRESHOLDS[detector]
    frames = []
    for m, al in [(None, None)] + [(m, al) for m in stego_methods for al in alphas]:
        rows, out = extract(data_dir, detector, m, al, split=split, simulate=simulate and m is not None, stream=stream, batch_size=batch_size, **kw)
        frames.append(rows.assign(output=out, prediction=np.zeros(len(out), dtype=bool) if thr is None else out > thr))
    return pd.concat(frames).reset_index(drop=True)[CSV_COLUMNS]


def curves(data_dir, stego_method: typing.Optional[str] = None, alpha: typing.Optional[float] = None, segments: int = 100, order: str = "rows",
           *, min_pair: int = 10, threshold: float = 0.5, split=None, simulate: bool = False, stream: int = 0, batch_size: int = 32,
           progress_on: bool = False, **kw):
    """A frame with the file columns (name, height, width, stego_method, alpha), `length` and p_0 .. p_{S-1}: the chi-square p-values of the
    prefixes of every image's path (`curve`) and the message length estimated from them (`length` at `threshold`).  The covers of `data_dir`
    or one stego folder; simulate=True makes the twins on the device, 'LSBRS' along `order` among them.  'LSBRS' files are read from the
    folder that embed.write_dataset gives the twins of `order` (`..._rows_up_...` for 'rows_up') where the data set has one; otherwise
    every LSBRS row of that alpha is read and a warning is logged."""
    import pandas as pd
    from . import ops
    if isinstance(segments, bool) or int(segments) != segments or not 1 <= segments <= ops.HIST_MAX_SEGMENTS:
        raise ValueError(f"curves: segments={segments!r} outside 1..{ops.HIST_MAX_SEGMENTS}")
    ops.order_id(order)
    _pair(stego_method, alpha, "curves")
    lsbrs = simulate and str(stego_method).upper() == "LSBRS"
    res = spam.file_set(*_iterators(batch_size), data_dir, stego_method, alpha, simulate, stream, simulated=SIMULATED + ("LSBRS",),
                        twin_order=order if lsbrs else None, path=(int(segments), order), split=split, progress_on=progress_on, **kw)
    if not simulate and str(stego_method).upper() == "LSBRS":
        # the files.csv rows of top-down and bottom-up twins differ in their folder only (embed.folder_name): keep the ones embedded along
        # `order` where the data set has them, and say so where it has not -- the curve then runs along a path the message does not follow
        from . import embed
        folder = embed.folder_name("LSBRS", alpha, order)
        mine = [r for r in res if str(r["name"]).startswith(folder + "/")]
        if mine:
            res = mine
        elif res:
            logging.warning(f"curves: no LSBRS files under {folder}/: the files read were not written for order {order!r}")
    p = chi2(np.stack([r["value"] for r in res]), min_pair)[2] if res else np.zeros((0, int(segments)))
    rows = spam.file_rows(res, ("value",)).assign(length=length(p, threshold))
    return pd.concat([rows, pd.DataFrame(p, columns=[f"p_{j}" for j in range(int(segments))], index=rows.index)], axis=1)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------

def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="The histogram attacks: the chi-square p-value and its curve along the file order, and the HCF "
                                             "centre of mass with Ker's calibrated and adjacency variants.  `score` files go into "
                                             "`python -m ws_unet_amd.ws.roc --scores FILE B0_<detector>`.")
    sub = ap.add_subparsers(dest="command", required=True)

    def common(p):
        p.add_argument("--data", required=True, help="data set directory (images*/files.csv, stego*/files.csv)")
        p.add_argument("--split", default=None, help="a split CSV of the data set instead of every file")
        p.add_argument("--simulate", action="store_true", help="make the twins of the covers on the device instead of reading stego files")
        p.add_argument("--stream", type=int, default=0, help="--simulate: realisation number (embed.image_seed)")
        p.add_argument("--batch-size", type=int, default=32)
        p.add_argument("--progress", action="store_true")
        p.add_argument("--out", required=True)

    p = sub.add_parser("score", help="write detector scores in the schema of results/detection/b0.csv")
    common(p)
    p.add_argument("--detector", required=True, choices=DETECTORS)
    p.add_argument("--stego-methods", nargs="+", default=["LSBR"])
    p.add_argument("--alphas", nargs="+", type=float, required=True)
    p = sub.add_parser("curve", help="write the chi-square p-value of every prefix of the path and the estimated message length")
    common(p)
    p.add_argument("--stego-method", default=None, help="the stego folder to read (default: the covers), e.g. LSBRS")
    p.add_argument("--alpha", type=float, default=None)
    p.add_argument("--segments", type=int, default=100)
    p.add_argument("--order", choices=("rows", "rows_up"), default="rows", help="the path: rows from the top, or from the bottom")
    p.add_argument("--min-pair", type=int, default=10, help="pairs of values with fewer pixels are dropped from the statistic")
    p.add_argument("--threshold", type=float, default=0.5, help="the p-value down to which a prefix counts as carrying a message")
    a = ap.parse_args(argv)
    if a.command == "curve":
        if (a.stego_method is None) != (a.alpha is None):
            ap.error("--stego-method and --alpha go together (neither: the covers)")
        if not 1 <= a.segments <= 4096:
            ap.error(f"--segments {a.segments} outside 1..4096")
    return a


def main(argv=None) -> None:
    a = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    run = dict(split=a.split, simulate=a.simulate, stream=a.stream, batch_size=a.batch_size, progress_on=a.progress)
    if a.command == "score":
        score(a.data, a.detector, a.stego_methods, a.alphas, **run).to_csv(a.out, index=False)
    else:
        curves(a.data, a.stego_method, a.alpha, a.segments, a.order, min_pair=a.min_pair, threshold=a.threshold, **run).to_csv(a.out, index=False)
    logging.info(f"output saved to {a.out}")


if __name__ == "__main__":
    main()
