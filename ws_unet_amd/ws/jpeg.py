"""WS for covers that were a JPEG once (R. Boehme, "Weighted stego-image steganalysis for JPEG covers", IH 2008; the companion of the
Ker-Boehme improvements that 'OLSa', the moderated weights and the bias correction cover).  Not part of the reference.

A bitmap that was decompressed from a JPEG file sits on the lattice of that file's quantisation table.  LSB replacement moves pixels by
+-1, far less than a quantisation step, so compressing the stego image again with the same table and decompressing it gives back an
estimate of the COVER that no 3x3 filter can match on such images: the predictor is the image itself after a round trip through JPEG.
It needs no library and no training:

  * `estimate_quality` finds the table: the residual energy of the image's 8x8 DCT coefficients against the IJG luminance tables of
    quality 1 .. max_quality (ops.jpeg_energies, K31: exact integers), and the LOWEST quality whose energy per pixel is at most tau is
    the history; none (0) means the image shows no JPEG history.  tau = 1.0: at the true table the residual is the decoder's rounding
    (1/12 per pixel) plus the embedding (at most 1/2 per pixel at full payload), measured at most 0.65 on the golden covers, while
    never-compressed covers measured at least 1.7 at quality 95;
  * `JPEGEstimator` is the pixel predictor: the round trip of every image through its own table (ops.jpeg_predict, K32) as a full-frame
    x_hat in pixel units, which the three WS statistics take as they take a UNet's output (ws.estimate, random and sequential placement;
    ws.locate).  Model name 'JPEG'.  An image without history is predicted with KB (the estimator counts and logs them like
    ols.AdaptiveOLSEstimator), or with fallback=None gets no estimate.  The predictor is not linear, so the bias correction of the
    reference (the predictor applied to x_bar - x) is not defined for it: correct_bias=True is an error.

Limits: grids other than the one at the plane's origin (cropped or shifted images) are not searched; at quality 90 and above the steps
are so small that the embedding noise survives the quantiser and the estimate falls short (-15 % at 90, useless at 98).  The integer
IDCT here is not a JPEG library's: accuracy on files decoded by one is unmeasured.

    python -m ws_unet_amd.ws.jpeg --data DIR [--out history.csv] [--recompress Q --write DIR2]

writes q_hat and the energies per pixel of every cover; --recompress writes a twin data set whose covers went through
ops.jpeg_recompress at quality Q (PNG, the same names), so that embed and the drivers can run on precompressed covers."""
from __future__ import annotations

import logging
import pathlib

import numpy as np
import torch

from .. import ops

NAMES = ("JPEG",)
MAX_QUALITY = 95
TAU = 1.0
FALLBACKS = ("KB", None)


def energy_bound(h: int, w: int, tau: float = TAU) -> int:
    """The largest energy (K31's 2^-20 units, summed over the image) that still counts as JPEG history: floor(tau 2^20 H W)."""
    return int(np.floor(float(tau) * 2.0 ** 20 * h * w))


def quality_rule(energies, bound: int):
    """energies: integer (N,M), column j the energy at quality j + 1 (numpy array or torch tensor) -> int64 (N,) of the same kind: the
    lowest quality whose energy is at most `bound`, 0 where none is."""
    ok = energies <= int(bound)
    if isinstance(energies, torch.Tensor):
        return torch.where(ok.any(dim=1), ok.to(torch.int8).argmax(dim=1) + 1, 0)
    return np.where(ok.any(axis=1), ok.argmax(axis=1) + 1, 0).astype(np.int64)


def _check_search(max_quality, tau) -> int:
    if not (isinstance(max_quality, (int, np.integer)) and 1 <= int(max_quality) <= 100):
        raise ValueError(f"max_quality: an integer in 1..100 expected, got {max_quality!r}")
    if not float(tau) > 0.:
        raise ValueError(f"tau must be positive, got {tau!r}")
    return int(max_quality)


def estimate_quality(x_u8: torch.Tensor, max_quality: int = MAX_QUALITY, tau: float = TAU, return_energies: bool = False):
    """(N,H,W) uint8 device planes -> int64 (N,) on the device: the IJG quality each image was compressed with, 0 for no JPEG history
    (with return_energies also K31's (N, max_quality) energies)."""
    max_quality = _check_search(max_quality, tau)
    energies = ops.jpeg_energies(x_u8, ops.jpeg_tables(np.arange(1, max_quality + 1)))
    q = quality_rule(energies, energy_bound(x_u8.shape[1], x_u8.shape[2], tau))
    return (q, energies) if return_energies else q


class JPEGEstimator:
    """The recompression predictor.  quality: None searches every image's history (1 .. max_quality, threshold tau); an integer uses that
    IJG quality for every image and skips the search.  fallback: 'KB' predicts an image without history with the KB filter, None gives it
    a plane of NaN, for which ws.estimate reports NaN (`without_estimate`), so that the drivers drop its row, and which adds nothing to
    ws.locate's sums.  ws.estimate.predictor_arguments recognises the estimator
    and keeps everything on the device's planes; called on a host (H,W,C) array like the reference's estimators it predicts that one
    image and returns (H-2,W-2,1).  `fallbacks` counts the images without history; the first one is logged (once per estimator)."""

    def __init__(self, quality=None, max_quality: int = MAX_QUALITY, fallback="KB", tau: float = TAU):
        if quality is not None and not (isinstance(quality, (int, np.integer)) and 1 <= int(quality) <= 100):
            raise ValueError(f"quality: None or an integer in 1..100 expected, got {quality!r}")
        if fallback not in FALLBACKS:
            raise ValueError(f"fallback: one of {FALLBACKS} expected, got {fallback!r}")
        self.quality = None if quality is None else int(quality)
        self.max_quality = _check_search(max_quality, tau)
        self.tau = float(tau)
        self.fallback = fallback
        self.fallbacks = 0

    def note(self, use) -> None:
        bad = int(np.size(use) - np.count_nonzero(use))
        if bad and not self.fallbacks:
            logging.warning("JPEG predictor: no JPEG history found; such images " +
                            ("are predicted with KB" if self.fallback == "KB" else "get no estimate"))
        self.fallbacks += bad

    def qualities(self, x_u8: torch.Tensor) -> np.ndarray:
        """host int64 (N,): the quality each image is recompressed with, 0 for none"""
        if self.quality is not None:
            return np.full(x_u8.shape[0], self.quality, dtype=np.int64)
        return estimate_quality(x_u8, self.max_quality, self.tau).cpu().numpy()

    def planes(self, x_u8: torch.Tensor) -> torch.Tensor:
        """(N,H,W) uint8 device planes -> float32 (N,H,W) predictions in pixel units (hat_scale = 1)."""
        q = self.qualities(x_u8)
        use = q > 0
        self.note(use)
        x_hat = ops.jpeg_predict(x_u8, ops.jpeg_tables(np.where(use, q, 1)), use)
        if self.fallback is None and not use.all():
            x_hat[torch.from_numpy(~use).to(x_hat.device)] = float("nan")
        return x_hat

    def device_arguments(self, x_u8: torch.Tensor, correct_bias: bool = False) -> dict:
        """The statistic kernels' keywords (ws.estimate.predictor_arguments): full frames in pixel units; no prediction of x_bar - x."""
        require_no_bias_correction(self, correct_bias)
        return dict(x_hat=self.planes(x_u8), hat_scale=1.0)

    def __call__(self, x: np.ndarray) -> np.ndarray:
        from ..imread import u8_plane
        plane = u8_plane(np.asarray(x)[..., 0], "the JPEG predictor needs integer pixel values in 0..255")
        hat = self.planes(torch.from_numpy(np.ascontiguousarray(plane))[None].cuda())[0]
        return hat[1:-1, 1:-1].cpu().numpy()[..., None]


def require_no_bias_correction(pixel_estimator, correct_bias) -> None:
    if correct_bias and isinstance(pixel_estimator, JPEGEstimator):
        raise ValueError("correct_bias=True is not defined for the JPEG predictor: it is not linear, so there is no prediction of x_bar - x")


def without_estimate(beta: torch.Tensor, x_hat: torch.Tensor) -> torch.Tensor:
    """beta (N,) with NaN where image i's plane of x_hat (N,H,W) is the NaN plane of fallback=None.  K11 carries a NaN of its prediction
    into its estimate itself (its clip at 0 keeps NaN, as np.clip does), so for placement='random' this changes nothing; the changepoint
    statistics K27 / K33 and the accumulator K29 skip NaN terms and would report a number for such a plane, so the function stays."""
    return torch.where(torch.isnan(x_hat[:, 0, 0]), torch.full_like(beta, float("nan")), beta)


def estimator(model_name: str):
    """'JPEG' -> a fresh JPEGEstimator, any other name -> None."""
    return JPEGEstimator() if model_name in NAMES else None


# ---- a data set -----------------------------------------------------------------------------------------------------------------------

def _history_chunk(fnames, kws, *, max_quality, tau, recompress=None, write=None, prefetched=None):
    """One chunk of covers -> one row per file: q_hat and the energies per pixel at q_hat, at q_hat - 1 and at max_quality (NaN where there
    is no such table); with `recompress` the twins are written under `write`."""
    from ..planes import plane_groups, upload_planes
    rows, i0 = [], 0
    for g, names in plane_groups(fnames, prefetched):             # (a ragged chunk: image by image)
        x = upload_planes(g, "cuda")
        q, e = estimate_quality(x, max_quality, tau, return_energies=True)
        q, e = q.cpu().numpy(), e.cpu().numpy().astype(np.float64) / 2.0 ** 20 / (x.shape[1] * x.shape[2])
        twins = ops.jpeg_recompress(x, recompress).cpu().numpy() if recompress is not None else None
        for j in range(len(names)):
            at = lambda k: float(e[j, k - 1]) if 1 <= k <= max_quality else float("nan")
            rows.append({"name": kws[i0 + j]["name"], "q_hat": int(q[j]), "energy_q_hat": at(int(q[j])), "energy_below": at(int(q[j]) - 1),
                         "energy_max_quality": at(max_quality), "height": int(x.shape[1]), "width": int(x.shape[2])})
            if twins is not None:
                from PIL import Image
                name = pathlib.Path(write) / pathlib.Path(kws[i0 + j]["name"]).with_suffix(".png")
                name.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(twins[j]).save(name)
        i0 += len(names)
    return rows


def history(data_dir, max_quality: int = MAX_QUALITY, tau: float = TAU, recompress=None, write=None, **kw):
    """The JPEG history of every cover of a data set (images*/files.csv, or the rows of `split`): a frame with name, q_hat, the energies
    per pixel at q_hat, at q_hat - 1 and at max_quality, height, width.  With `recompress` = Q and `write` = DIR2 also the twin data set
    DIR2/<name>.png of the covers after ops.jpeg_recompress at quality Q, with a files.csv per folder.  Other keywords go to the fabrika
    iterator (split, take_num_images, ...)."""
    import pandas as pd
    from .. import fabrika
    from ..planes import load_planes_u8
    max_quality = _check_search(max_quality, tau)
    if (recompress is None) != (write is None):
        raise ValueError("history: give recompress and write together")
    if recompress is not None and not 1 <= int(recompress) <= 100:
        raise ValueError(f"recompress: a quality in 1..100 expected, got {recompress!r}")
    keys = ("max_quality", "tau", "recompress", "write")
    chunk = fabrika.shared_kwargs(_history_chunk, keys, lambda fnames, kws: (load_planes_u8(fnames),))
    res = fabrika.precovers(iterator="batched", ignore_missing=True)(chunk)(
        pathlib.Path(data_dir), max_quality=max_quality, tau=float(tau), recompress=None if recompress is None else int(recompress),
        write=None if write is None else str(write), **kw)
    res = res[["name", "q_hat", "energy_q_hat", "energy_below", "energy_max_quality", "height", "width"]]
    if write is not None:
        twin = res.assign(name=[str(pathlib.Path(n).with_suffix(".png")) for n in res["name"]])
        for folder, rows in twin.groupby(twin["name"].map(lambda n: str(pathlib.Path(n).parent))):
            rows[["name", "height", "width"]].to_csv(pathlib.Path(write) / folder / "files.csv", index=False)
    return res


def main(argv=None) -> None:
    import argparse
    ap = argparse.ArgumentParser(description="JPEG history of a data set's covers: the IJG quality each was compressed with (0: none) and "
                                             "its residual energies per pixel; optionally a JPEG-precompressed twin of the data set.")
    ap.add_argument("--data", required=True, help="data set directory (images*/files.csv)")
    ap.add_argument("--out", default=None, help="history.csv (default: <data>/history.csv)")
    ap.add_argument("--split", default=None, help="a split CSV of the data set: only its covers")
    ap.add_argument("--max-quality", type=int, default=MAX_QUALITY)
    ap.add_argument("--tau", type=float, default=TAU, help="largest residual energy per pixel that counts as JPEG history")
    ap.add_argument("--recompress", type=int, default=None, metavar="Q", help="with --write: IJG quality of the twin data set")
    ap.add_argument("--write", default=None, metavar="DIR2", help="with --recompress: where the twin data set goes")
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    res = history(a.data, a.max_quality, a.tau, a.recompress, a.write, split=a.split)
    out = pathlib.Path(a.out or pathlib.Path(a.data) / "history.csv")
    out.parent.mkdir(parents=True, exist_ok=True)
    res.to_csv(out, index=False)
    print(f"output saved to {out}")


if __name__ == "__main__":
    main()
