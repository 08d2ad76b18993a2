"""The normal-equation fit that the least-squares pixel predictors share (ws_unet_amd.ols: the 3x3 window, 8 taps; ws_unet_amd.ols5: the
5x5 window, 24 taps).  A `Window` says what differs between them -- the number of variables, the indicator matrix of the symmetric fit,
the fallback taps, the moments kernel, the margin and a few words -- and its methods are the fit, written once: the device's exact
integer moments of V variables (the T = V - 1 neighbours, then the centre y) are the V (V + 1) / 2 products v_p * v_q, p <= q; they hold
A = X^T X (T x T), b = X^T y and y^T y, and they add over images.  Each module makes its window and binds the methods to its own names
(`ols.fit`, `ols5.load_kernels`, ...).

A fit is valid iff the matrix of the solved system is positive definite and its condition number is at most COND_MAX; otherwise the
taps are the window's fallback (KB) and ok is False."""
from __future__ import annotations

import collections
import dataclasses
import json
import logging
import pathlib
import typing

import numpy as np

from .planes import load_planes_u8, plane_groups, upload_planes

COND_MAX = 1e12
DatasetFit = collections.namedtuple("DatasetFit", "taps ok moments count")


@dataclasses.dataclass(frozen=True, eq=False)
class Window:
    vars: int                      # 9 or 25: the neighbours and the centre
    symmetric: np.ndarray          # (taps, parameters) indicator matrix of the symmetric fit
    kb: typing.Callable            # () -> the fallback taps of an invalid fit
    moments_op: str                # the entry of `ops` that sums the moments of (N,H,W) uint8 planes
    margin: int                    # rows / columns at each side without a full window
    register: typing.Callable      # (name, taps): where load_kernels(register=True) enters a kernel
    size: str                      # "3x3" / "5x5"
    label: str                     # the fit in a log line: "OLS" / "OLS 5x5"
    entries: typing.Tuple[str, str]  # the names `main` writes: (plain, symmetric)
    file: str                      # the kernels file in the help texts
    symmetric_help: str
    show: typing.Callable          # (name, taps) -> the line(s) `main` prints for fitted taps

    @property
    def taps(self) -> int:
        return self.vars - 1

    @property
    def moments(self) -> int:
        return self.vars * (self.vars + 1) // 2

    def unpack(self, moments):
        """(M,) or (N,M) integer moments -> (A (...,T,T), b (...,T), yty (...)) float64.  Float64 holds integers up to 2^53 exactly; a
        larger entry (about 5e5 images of 512^2 summed) raises."""
        m, T, M = np.asarray(moments), self.taps, self.moments
        if m.dtype.kind not in "iu" or m.shape[-1] != M or m.ndim not in (1, 2):
            raise ValueError(f"expected integer moments of shape ({M},) or (N,{M}), got {m.dtype} {m.shape}")
        if m.size and (m.min() < 0 or m.max() > 2 ** 53):
            raise OverflowError("a moment outside [0, 2^53] is not exact in float64")
        iu = np.triu_indices(self.vars)
        full = np.zeros(m.shape[:-1] + (self.vars, self.vars))
        full[..., iu[0], iu[1]] = m
        full[..., iu[1], iu[0]] = m
        return full[..., :T, :T], full[..., :T, T], full[..., T, T]

    def _solve(self, A, b, symmetric):
        S = self.symmetric if symmetric else None
        if symmetric:
            A, b = S.T @ A @ S, S.T @ b
        try:
            np.linalg.cholesky(A)
            if not np.linalg.cond(A) <= COND_MAX:
                raise np.linalg.LinAlgError
            k = np.linalg.solve(A, b)
        except np.linalg.LinAlgError:
            return self.kb(), False
        if not np.all(np.isfinite(k)):
            return self.kb(), False
        return (S @ k if symmetric else k), True

    def fit(self, moments, symmetric: bool = False):
        """Least-squares taps of one row of moments -> (taps (T,) float64, ok), or of every row of (N,M) -> ((N,T), ok (N,) bool).
        numpy.linalg.solve on the normal equations, no intercept.  symmetric=True fits one parameter per column of the window's indicator
        matrix S (A and b folded, S^T A S and S^T b) and expands them to T taps; validity is then judged on the folded system, the one
        that is solved.  An invalid fit returns the fallback taps (KB) and ok False."""
        A, b, _ = self.unpack(moments)
        if A.ndim == 2:
            return self._solve(A, b, symmetric)
        res = [self._solve(Ai, bi, symmetric) for Ai, bi in zip(A, b)]
        return np.array([r[0] for r in res]).reshape(len(res), self.taps), np.array([r[1] for r in res], dtype=bool)

    def residual_mse(self, moments, taps, count):
        """Mean squared residual of y - X k over the `count` pixels the moments were summed over: (yty - 2 k.b + k.A.k) / count, exact
        algebra on the moments (the pixel count is no moment of a fit without intercept, so the caller passes it)."""
        A, b, yty = self.unpack(moments)
        k = np.asarray(taps, dtype=np.float64).reshape(self.taps)
        return (yty - 2. * (b @ k) + k @ A @ k) / count

    def note(self, estimator, ok) -> None:
        """Counts the invalid fits among `ok` in estimator.fallbacks; the first one of an estimator (i.e. of a run) is logged."""
        bad = int(np.size(ok) - np.count_nonzero(ok))
        if bad and not estimator.fallbacks:
            logging.warning(f"{self.label} fit: singular or ill-conditioned normal equations; such images are predicted with KB")
        estimator.fallbacks += bad

    # ---- files ------------------------------------------------------------------------------------------------------------------

    def save_kernels(self, path, kernels) -> None:
        """{name: taps} -> JSON {name: [T floats], ...}; Python's float repr round-trips exactly."""
        out = {str(name): [float(t) for t in np.asarray(taps, dtype=np.float64).reshape(self.taps)] for name, taps in kernels.items()}
        path = pathlib.Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(out, indent=1) + "\n")

    def load_kernels(self, path, register: bool = False) -> dict:
        """The {name: taps (T,) float64} of a save_kernels file; register=True enters every one into the module's name registry."""
        raw = json.loads(pathlib.Path(path).read_text())
        if not isinstance(raw, dict):
            raise ValueError(f"{path}: expected a JSON object of name -> {self.taps} taps")
        kernels = {}
        for name, taps in raw.items():
            k = np.asarray(taps, dtype=np.float64)
            if k.shape != (self.taps,):
                raise ValueError(f"{path}: {name!r} has shape {k.shape}, expected {self.taps} taps")
            kernels[name] = k
        if register:
            for name, k in kernels.items():
                self.register(name, k)
        return kernels

    # ---- one fit for a data set -------------------------------------------------------------------------------------------------

    def fit_dataset(self, data_dir, split: str = None, take_num_images: int = None, symmetric: bool = False,
                    batch_size: int = 32) -> DatasetFit:
        """One fit over the cover images of a data set (fabrika's precovers; `split`, `take_num_images` as everywhere): the batched
        iterator with the native PNG decode one chunk ahead, one moments launch per chunk, the rows summed as int64 on the device and
        read back once.  -> DatasetFit(taps (T,) float64, ok, moments (M,) int64, count = pixels with a full window).  Single process."""
        from . import fabrika, ops
        total, count, cut = [None], [0], 2 * self.margin

        def chunk(fnames, kws, prefetched=None):
            for g, _ in plane_groups(fnames, prefetched):             # (a ragged chunk: image by image)
                m = getattr(ops, self.moments_op)(upload_planes(g, "cuda")).sum(dim=0)
                total[0] = m if total[0] is None else total[0] + m
                count[0] += g.shape[0] * (g.shape[1] - cut) * (g.shape[2] - cut)
            return [None] * len(fnames)

        chunk.prefetch = lambda fnames, kws: (load_planes_u8(fnames),)
        fabrika.precovers(iterator="batched", convert_to=None, ignore_missing=True, batch_size=batch_size)(chunk)(
            data_dir, split=split, take_num_images=take_num_images)
        moments = total[0].cpu().numpy()
        taps, ok = self.fit(moments, symmetric)
        return DatasetFit(taps, ok, moments, count[0])

    def main(self, argv=None) -> None:
        import argparse
        ap = argparse.ArgumentParser(description=f"fit a least-squares {self.size} pixel predictor on the cover images of a data set")
        ap.add_argument("--data", required=True, help="dataset root with images*/files.csv (the reference's ../data)")
        ap.add_argument("--split", default=None, help="split file under --data, e.g. split_tr.csv (default: every cover)")
        ap.add_argument("--take", type=int, default=None, help="the first N images")
        ap.add_argument("--symmetric", action="store_true", help=f"{self.symmetric_help}; the entry is named {self.entries[1]}")
        ap.add_argument("--out", required=True, help=f"{self.file}; an existing file keeps its other entries")
        a = ap.parse_args(argv)
        logging.basicConfig(level=logging.INFO)
        res = self.fit_dataset(a.data, split=a.split, take_num_images=a.take, symmetric=a.symmetric)
        name = self.entries[bool(a.symmetric)]
        if not res.ok:
            logging.warning(f"{name}: singular or ill-conditioned normal equations; writing KB's taps")
        out = pathlib.Path(a.out)
        kernels = self.load_kernels(out) if out.exists() else {}
        kernels[name] = res.taps
        self.save_kernels(out, kernels)
        print(self.show(name, res.taps))
        print(f"{name} residual mse {self.residual_mse(res.moments, res.taps, res.count):.6f}   "
              f"KB residual mse {self.residual_mse(res.moments, self.kb(), res.count):.6f}   over {res.count} pixels")
        print(f"output saved to {out}")
