"""A trainable feature-based detector: SPAM features (T. Pevny, P. Bas, J. Fridrich, "Steganalysis by subtractive pixel adjacency
matrix", IEEE TIFS 5(2), 2010) and a ridge-regularised Fisher linear discriminant.  Not part of the reference, whose detector rows come
from an EfficientNet-B0 that is out of scope here (its scores enter ws.roc as files); this one is trained in the package, in seconds.

    python -m ws_unet_amd.spam fit   --data DIR [--split split_tr.csv] --stego-methods LSBR --alphas .4 .2 .1 [--simulate] --out spam_fld.npz
    python -m ws_unet_amd.spam score --data DIR [--split split_te.csv] --model spam_fld.npz --stego-methods LSBR --alphas .1 [--simulate] --out spam.csv
    python -m ws_unet_amd.spam features --data DIR --stego-methods LSBR --alphas .1 --out F.npz
    python -m ws_unet_amd.ws.roc --data DIR --out-dir OUT --scores spam.csv B0_SPAM

`score` writes the schema of results/detection/b0.csv, which `ws.roc --scores FILE NAME` takes unchanged.  NAME must contain 'B0' (that is
how ws.roc.produce_roc tells a detector's score from a WS estimate), hence the spelling B0_SPAM.

The package's pattern for per-image statistics: the device counts exact integers (ops.spam_counts, K36: the co-occurrences of order + 1
clipped differences of neighbouring pixels along four steps), the host does a few float64 operations on them.

  * `opposite` derives the counts of the four opposite steps: the same runs walked backwards, C_opp[d_0..d_order] = C[-d_order..-d_0];
  * `features` divides each of the eight tables by its own total ('joint') or each bin by the total of the B bins that share all but the
    last difference ('transition', the paper's conditional probability; 0 where that total is 0), and averages the tables of the four
    axis steps into the first half of the vector and those of the four diagonal steps into the second: 2 B^(order+1) numbers, 686 at
    order 2, T 3 (SPAM-686), 162 at order 1, T 4;
  * `FLD` is Fisher's discriminant with a ridge on the pooled within-class covariance, one float64 solve of the feature dimension;
  * `fit --classifier ensemble --learners L --d-sub D [D ...] --seed S` trains the FLD ensemble of ws_unet_amd.ensemble (`Ensemble`, with
    the tags order, T, normalise) in its place; `load_model` reads either kind of file.  The default stays the FLD.

Not checked: the authors' MATLAB extractor is not at hand.  Clipping differences beyond +-T into the border bins, normalising each
direction's table by its own total and offering 'transition' as the alternative is the convention of the common SPAM-686 code as
remembered, unverified against it.
"""
from __future__ import annotations

import argparse
import logging
import pathlib
import typing

import numpy as np
import torch

from . import ensemble, fabrika

NORMALISE = ("joint", "transition")
SIMULATED = ("LSBR", "HILLR", "LSBM", "HILL")                       # the stego methods `simulate=True` makes on the device
CLASSIFIERS = ("fld", "ensemble")
CSV_COLUMNS = ["name", "height", "width", "output", "prediction", "stego_method", "alpha"]


def bins(order: int = 2, T: int = 3) -> int:
    """B^(order+1), B = 2T + 1: the bins of one direction; ValueError for an (order, T) that K36 does not take."""
    from . import ops
    return ops.spam_bins(order, T)


def opposite(counts, order: int = 2, T: int = 3):
    """The counts of the opposite steps (left, up, up-left, up-right for right, down, down-right, down-left) from counts (..., B^(order+1)),
    a numpy array or a torch tensor: C_opp[d_0, .., d_order] = C[-d_order, .., -d_0], an index permutation."""
    nb, B, k = bins(order, T), 2 * T + 1, order + 1
    if counts.shape[-1] != nb:
        raise ValueError(f"opposite: last dimension {counts.shape[-1]}, expected {nb} bins for order {order}, T {T}")
    lead = tuple(counts.shape[:-1])
    nl = len(lead)
    digits = tuple(range(nl, nl + k))
    t = counts.reshape(lead + (B,) * k)
    perm = tuple(range(nl)) + digits[::-1]
    if isinstance(counts, torch.Tensor):
        return t.flip(digits).permute(perm).reshape(lead + (nb,))
    return np.ascontiguousarray(np.transpose(np.flip(t, digits), perm)).reshape(lead + (nb,))


def features(counts, order: int = 2, T: int = 3, normalise: str = "joint") -> np.ndarray:
    """counts (N,4,B^(order+1)) of ops.spam_counts (a numpy array or a torch tensor) -> (N, 2 B^(order+1)) float64: every one of the eight
    direction tables normalised on its own, then the mean of the tables of right, left, down, up and the mean of those of the four
    diagonal steps.  ValueError when an image has a direction without a counted position (h or w below order + 2)."""
    if normalise not in NORMALISE:
        raise ValueError(f"unknown normalise {normalise!r}; choose from {NORMALISE}")
    nb, B = bins(order, T), 2 * T + 1
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    if c.ndim != 3 or c.shape[1:] != (4, nb):
        raise ValueError(f"features: counts of shape {c.shape}, expected (N, 4, {nb}) for order {order}, T {T}")
    tables = np.concatenate([c, opposite(c, order, T)], axis=1).astype(np.float64)          # right, down, down-right, down-left, then their opposites
    totals = tables.sum(axis=2, keepdims=True)
    if (totals == 0).any():
        raise ValueError(f"features: image {int(np.argwhere(totals[:, :, 0] == 0)[0, 0])} has a direction with no run of {order + 2} pixels")
    if normalise == "joint":
        p = tables / totals
    else:
        rows = tables.reshape(tables.shape[0], 8, nb // B, B)
        den = rows.sum(axis=3, keepdims=True)
        p = np.divide(rows, den, out=np.zeros_like(rows), where=den != 0).reshape(tables.shape)
    axis = (p[:, 0] + p[:, 4] + p[:, 1] + p[:, 5]) / 4.
    diag = (p[:, 2] + p[:, 6] + p[:, 3] + p[:, 7]) / 4.
    return np.concatenate([axis, diag], axis=1)


class FLD:
    """Fisher's linear discriminant with a ridge, in float64: S the pooled within-class covariance of the two classes, lambda =
    ridge trace(S) / d, w = (S + lambda I)^-1 (mu1 - mu0), b = w.(mu0 + mu1) / 2.  `log_odds(F)` = F.w - b; `output(F)` =
    1 / (1 + exp(-log_odds)), the posterior of linear discriminant analysis under equal priors: in 0..1, the range ws.roc sweeps, with
    0.5 as the decision.  The default ridge 0.1 comes from one check on 64 x 64 crops of the five fixture covers (held-out AUC 0.925 at
    0.1, 0.811 at 1e-3 with full-payload LSBR twins); it is not tuned on any real data set."""

    dual = False            # True (srm's larger feature sets): with fewer rows than features and ridge > 0, `fit` solves the n x n dual system

    def __init__(self, ridge: float = 0.1, order: int = 2, T: int = 3, normalise: str = "joint"):
        if not ridge >= 0:
            raise ValueError(f"ridge {ridge!r} must not be negative")
        if normalise not in NORMALISE:
            raise ValueError(f"unknown normalise {normalise!r}; choose from {NORMALISE}")
        bins(order, T)
        self.ridge, self.order, self.T, self.normalise = float(ridge), int(order), int(T), normalise
        self.w, self.b = None, None
        self.stego_methods, self.alphas = [], []

    def fit(self, X0, X1, ridge: typing.Optional[float] = None) -> "FLD":
        """X0: the cover class (n0, d), X1: the stego class (n1, d)."""
        if ridge is not None:
            if not ridge >= 0:
                raise ValueError(f"ridge {ridge!r} must not be negative")
            self.ridge = float(ridge)
        X0, X1 = np.asarray(X0, dtype=np.float64), np.asarray(X1, dtype=np.float64)
        if X0.ndim != 2 or X1.ndim != 2 or X0.shape[1] != X1.shape[1] or len(X0) + len(X1) < 3 or not len(X0) or not len(X1):
            raise ValueError(f"fit: classes of shape {X0.shape} and {X1.shape}: two (n, d) matrices of one d and at least 3 rows in all")
        d = X0.shape[1]
        mu0, mu1 = X0.mean(axis=0), X1.mean(axis=0)
        A0, A1 = X0 - mu0, X1 - mu1
        if self.dual and len(X0) + len(X1) < d and self.ridge > 0:
            # fewer rows than features: S = A^T A with A the centred rows over sqrt(n - 2), and by Woodbury
            # (A^T A + lambda I)^-1 = (I - A^T (A A^T + lambda I)^-1 A) / lambda: an n x n system in place of the d x d one
            A = np.concatenate([A0, A1]) / np.sqrt(len(X0) + len(X1) - 2.)
            lam = self.ridge * float(np.einsum("ij,ij->", A, A)) / d             # trace(S) = ||A||_F^2
            if not lam > 0:
                raise ValueError("fit: the classes have no within-class variance")
            delta = mu1 - mu0
            self.w = (delta - A.T @ np.linalg.solve(A @ A.T + lam * np.eye(len(A)), A @ delta)) / lam
            self.b = float(self.w @ (mu0 + mu1) / 2.)
            return self
        S = (A0.T @ A0 + A1.T @ A1) / (len(X0) + len(X1) - 2)
        lam = self.ridge * np.trace(S) / d
        self.w = np.linalg.solve(S + lam * np.eye(d), mu1 - mu0)
        self.b = float(self.w @ (mu0 + mu1) / 2.)
        return self

    def log_odds(self, F) -> np.ndarray:
        if self.w is None:
            raise ValueError("this FLD is not fitted")
        return np.asarray(F, dtype=np.float64) @ self.w - self.b

    def output(self, F) -> np.ndarray:
        with np.errstate(over="ignore"):
            return 1. / (1. + np.exp(-self.log_odds(F)))

    def save(self, path) -> None:
        """An .npz of arrays only: w, b, ridge, order, T, normalise and the stego methods and alphas of the training set."""
        if self.w is None:
            raise ValueError("this FLD is not fitted")
        with open(path, "wb") as f:
            np.savez(f, w=self.w, b=np.float64(self.b), ridge=np.float64(self.ridge), order=np.int64(self.order), T=np.int64(self.T),
                     normalise=np.array(self.normalise), stego_methods=np.array(list(self.stego_methods), dtype=str),
                     alphas=np.array(list(self.alphas), dtype=np.float64))

    @classmethod
    def load(cls, path) -> "FLD":
        with np.load(path, allow_pickle=False) as z:
            ensemble.refuse_ensemble(z, path, "spam")
            m = cls(float(z["ridge"]), int(z["order"]), int(z["T"]), str(z["normalise"]))
            m.w, m.b = np.array(z["w"], dtype=np.float64), float(z["b"])
            m.stego_methods, m.alphas = [str(s) for s in z["stego_methods"]], [float(a) for a in z["alphas"]]
        if m.w.shape != (2 * bins(m.order, m.T),):
            raise ValueError(f"{path}: {m.w.shape[0]} weights for order {m.order}, T {m.T}")
        return m


class Ensemble(ensemble.Ensemble):
    """ensemble.Ensemble (its fit, votes, output) on the features of this module; the file carries FLD's tags order, T, normalise."""

    def __init__(self, learners: int = 51, d_sub=None, ridge: float = 0.1, seed: int = 0, order: int = 2, T: int = 3, normalise: str = "joint"):
        super().__init__(learners, d_sub, ridge, seed)
        if normalise not in NORMALISE:
            raise ValueError(f"unknown normalise {normalise!r}; choose from {NORMALISE}")
        bins(order, T)
        self.order, self.T, self.normalise = int(order), int(T), normalise

    def _tags(self) -> dict:
        return dict(order=np.int64(self.order), T=np.int64(self.T), normalise=np.array(self.normalise))

    @classmethod
    def load(cls, path) -> "Ensemble":
        with np.load(path, allow_pickle=False) as z:
            cls._require(z, path)
            m = cls(int(z["learners"]), [int(v) for v in z["d_sub_candidates"]], float(z["ridge"]), int(z["seed"]), int(z["order"]), int(z["T"]),
                    str(z["normalise"]))._read(z, path)
        if m.mean.shape != (2 * bins(m.order, m.T),):
            raise ValueError(f"{path}: {m.mean.shape[0]} features for order {m.order}, T {m.T}")
        return m


def load_model(path):
    """The model of `fit` at `path`, an FLD or an Ensemble as the file's `classifier` entry says (an FLD file has none)."""
    return Ensemble.load(path) if ensemble.is_ensemble_file(path) else FLD.load(path)


# ---- features of a data set ----------------------------------------------------------------------------------------------------------

def _prefetch(fnames, kws):
    from .planes import load_planes_u8
    return (load_planes_u8(fnames),)


def device_planes(fnames, twin=None, prefetched=None):
    """The chunk's Y planes on the device, uploaded once: one (x, names) per group of files of one shape.  twin = (method, alpha, stream):
    their twins instead, made on the device with the seeds embed.image_seed(file, stream) ('HILLR' takes none); a fourth entry is the
    path order of 'LSBRS'.  Nothing waits for the GPU.  (Shared with ws_unet_amd.histogram.)"""
    from . import embed, embed_pm1
    from .planes import plane_groups, upload_planes
    for planes, names in plane_groups(fnames, prefetched):
        x = upload_planes(planes, "cuda")
        if twin is not None:
            method, alpha, stream, *path = twin
            seeds = [embed.image_seed(f, stream) for f in names]
            if method in embed_pm1.METHODS:
                x = embed_pm1.simulate(x, method, alpha, seeds)[0]
            else:
                x = embed.simulate(x, method, alpha, seeds if method != "HILLR" else None, **({"order": path[0]} if path else {}))[0]
        yield x, names


def _submit(fnames, clean, *, order, T, twin=None, prefetched=None):
    """Upload the chunk's Y planes once, make their twins when asked (twin = (method, alpha, stream)), queue K36; nothing waits for the GPU."""
    from . import ops
    return clean, [ops.spam_counts(x, order, T) for x, _ in device_planes(fnames, twin, prefetched)]


def _collect(handle):
    clean, counts = handle
    c = np.concatenate([t.cpu().numpy() for t in counts])
    return [{**kw, "counts": c[i]} for i, kw in enumerate(clean)]


def _count_chunk(fnames, kws, prefetched=None, **shared):
    return _collect(_submit(fnames, kws, prefetched=prefetched, **shared))


_count_chunk.submit, _count_chunk.collect = _submit, _collect
_count_chunk = fabrika.shared_kwargs(_count_chunk, ("order", "T", "twin"), _prefetch)


def _iterators(batch_size: int):
    kw = dict(iterator="batched", convert_to=None, ignore_missing=True, batch_size=batch_size)
    return fabrika.precovers(**kw)(_count_chunk), fabrika.stego_spatial(**kw)(_count_chunk)


def file_set(covers, stegos, data_dir, stego_method, alpha, simulate, stream, *, simulated=SIMULATED, twin_order=None, **shared):
    """The rows of one image set from a pair of fabrika iterators over one chunk function: the covers (stego_method None), the files of one
    stego folder, or with simulate=True the covers again with twin=(method, alpha, stream) for the chunk function and their rows named as
    the simulator's write_dataset would name the files.  simulated: the methods simulate=True may make; twin_order: the path order of
    'LSBRS' twins, a fourth entry of `twin`.  (Shared with ws_unet_amd.histogram.)"""
    from . import embed, embed_pm1
    if stego_method is None:
        return covers(data_dir, **shared)
    if simulate:
        maker = embed_pm1 if str(stego_method).upper() in embed_pm1.METHODS else embed
        method = maker.method_name(stego_method)
        if method not in simulated:
            raise ValueError(f"simulate=True makes {' / '.join(simulated)} twins only, not {stego_method!r}")
        path = () if twin_order is None else (twin_order,)
        folder = maker.folder_name(method, alpha, *path)
        return [{**r, "name": f"{folder}/{pathlib.Path(r['name']).stem}.png", "stego_method": method, "alpha": float(alpha)}
                for r in covers(data_dir, twin=(method, float(alpha), int(stream), *path), **shared)]
    try:
        return stegos(data_dir, stego_method=stego_method, alpha=alpha, **shared)
    except KeyError as e:
        raise ValueError(f"split {shared.get('split')!r} lists no stego rows (no {e.args[0]!r} column): use simulate=True or a split that names them") from e


def file_rows(res, drop=()):
    """the frame name, height, width, stego_method, alpha of the rows `res` without their `drop` entries (covers: NaN in the last two)"""
    import pandas as pd
    rows = pd.DataFrame([{k: v for k, v in r.items() if k not in drop} for r in res])
    for col in ("stego_method", "alpha"):
        if col not in rows:
            rows[col] = np.nan
    return rows[["name", "height", "width", "stego_method", "alpha"]]


def extract(data_dir, stego_method: typing.Optional[str] = None, alpha: typing.Optional[float] = None, split: typing.Optional[str] = None,
            order: int = 2, T: int = 3, normalise: str = "joint", simulate: bool = False, stream: int = 0, batch_size: int = 32,
            progress_on: bool = False, **kw):
    """(rows, F): the file rows (a frame with name, height, width, stego_method, alpha) and the (N, 2 B^(order+1)) float64 feature matrix of
    the covers of `data_dir` (stego_method None) or of one stego folder (stego_method, alpha), from the Y plane of every image, decoded a
    chunk ahead and uploaded a chunk at a time.  simulate=True makes the twins of the uploaded covers on the device instead of reading stego
    files ('LSBR' with embed.image_seed(file, stream), 'HILLR'; 'LSBM' and 'HILL' of embed_pm1 with the same seeds); their rows are named as
    embed.write_dataset / embed_pm1.write_dataset would name the files.
    Other keywords go to the fabrika iterators (take_num_images, shuffle_seed, ...)."""
    bins(order, T)
    if normalise not in NORMALISE:
        raise ValueError(f"unknown normalise {normalise!r}; choose from {NORMALISE}")
    if (stego_method is None) != (alpha is None):
        raise ValueError("extract: give both stego_method and alpha, or neither (the covers)")
    shared = dict(order=order, T=T, split=split, progress_on=progress_on, **kw)
    res = file_set(*_iterators(batch_size), data_dir, stego_method, alpha, simulate, stream, **shared)
    rows = file_rows(res, ("counts",))
    return rows, features(np.stack([r["counts"] for r in res]), order, T, normalise)


def _sets(a):
    return [(m, al) for m in a.stego_methods for al in a.alphas]


def check_classifier(classifier: str, d_sub) -> str:
    """'fld' or 'ensemble'; ValueError for another name and for an ensemble without d_sub"""
    if classifier not in CLASSIFIERS:
        raise ValueError(f"unknown classifier {classifier!r}; choose from {CLASSIFIERS}")
    if classifier == "ensemble" and not d_sub:
        raise ValueError("classifier 'ensemble' needs d_sub (--d-sub D [D ...]): the features of a base learner, or candidates to choose from")
    return classifier


def fit(data_dir, stego_methods, alphas, *, split=None, simulate=False, order=2, T=3, normalise="joint", ridge=0.1, classifier="fld",
        learners=51, d_sub=None, seed=0, **kw):
    """An FLD on the covers of `data_dir` against its stegos of every listed (method, alpha), pooled into one class.  classifier='ensemble':
    an Ensemble(learners, d_sub, ridge, seed) instead, whose bootstrap keeps the rows of one file stem (a cover and its twins) together."""
    check_classifier(classifier, d_sub)
    opts = dict(split=split, order=order, T=T, normalise=normalise, **kw)
    rows0, F0 = extract(data_dir, **opts)
    parts = [extract(data_dir, m, al, simulate=simulate, **opts) for m in stego_methods for al in alphas]
    F1 = np.concatenate([p[1] for p in parts])
    if classifier == "ensemble":
        groups = ensemble.stem_groups(rows0["name"], np.concatenate([p[0]["name"].to_numpy(str) for p in parts]))
        model = Ensemble(learners, d_sub, ridge, seed, order, T, normalise).fit(F0, F1, *groups)
    else:
        model = FLD(ridge, order, T, normalise).fit(F0, F1)
    model.stego_methods, model.alphas = [str(m) for m in stego_methods], [float(al) for al in alphas]
    return model


def score(data_dir, model, stego_methods, alphas, *, split=None, simulate=False, **kw):
    """The frame of results/detection/b0.csv: the covers (empty stego_method and alpha), then the stegos method by method and alpha by
    alpha; output = model.output of the image's features, prediction = output > 0.5."""
    import pandas as pd
    opts = dict(split=split, order=model.order, T=model.T, normalise=model.normalise, **kw)
    frames = []
    for m, al in [(None, None)] + [(m, al) for m in stego_methods for al in alphas]:
        rows, F = extract(data_dir, m, al, simulate=simulate and m is not None, **opts)
        out = model.output(F)
        frames.append(rows.assign(output=out, prediction=out > 0.5))
    return pd.concat(frames).reset_index(drop=True)[CSV_COLUMNS]


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------

def add_classifier_options(p) -> None:
    """the options of `fit` that choose and shape the classifier (shared with ws_unet_amd.srm)"""
    p.add_argument("--classifier", choices=CLASSIFIERS, default="fld",
                   help="fld: one ridge-regularised Fisher discriminant (the default); ensemble: the FLD ensemble of ws_unet_amd.ensemble")
    p.add_argument("--learners", type=int, default=51, help="--classifier ensemble: base learners (odd, so that a vote cannot tie)")
    p.add_argument("--d-sub", type=int, nargs="+", default=None,
                   help="--classifier ensemble (required): features per base learner; several values: the one with the least out-of-bag error")
    p.add_argument("--seed", type=int, default=0, help="--classifier ensemble: the seed of its draws")


def classifier_keywords(ap, a) -> dict:
    """the keywords of `fit` from the parsed options; the parser's error when `ensemble` comes without --d-sub"""
    if a.classifier == "ensemble" and not a.d_sub:
        ap.error("--classifier ensemble requires --d-sub D [D ...]")
    return dict(classifier=a.classifier, learners=a.learners, d_sub=a.d_sub, seed=a.seed) if a.classifier == "ensemble" else {}


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="SPAM features and a Fisher linear discriminant: a detector trained in the package, whose "
                                             "scores `python -m ws_unet_amd.ws.roc --scores FILE B0_SPAM` reads.")
    sub = ap.add_subparsers(dest="command", required=True)

    def common(p, model_options: bool):
        p.add_argument("--data", required=True, help="data set directory (images*/files.csv, stego*/files.csv)")
        p.add_argument("--split", default=None, help="a split CSV of the data set instead of every file")
        p.add_argument("--stego-methods", nargs="+", default=["LSBR"])
        p.add_argument("--alphas", nargs="+", type=float, required=True)
        p.add_argument("--simulate", action="store_true",
                       help=f"make the twins of the covers on the device ({' / '.join(SIMULATED)}) instead of reading stego files")
        p.add_argument("--stream", type=int, default=0, help="--simulate: LSBR realisation number (embed.image_seed)")
        p.add_argument("--batch-size", type=int, default=32)
        p.add_argument("--progress", action="store_true")
        p.add_argument("--out", required=True)
        if model_options:
            p.add_argument("--order", type=int, choices=(1, 2), default=2)
            p.add_argument("--T", type=int, default=3, help="differences are clipped to -T..T: 1..8 at order 1, 1..4 at order 2")
            p.add_argument("--normalise", choices=NORMALISE, default="joint")

    p = sub.add_parser("fit", help="train on the covers against every listed (method, alpha), pooled; writes the model .npz")
    common(p, True)
    p.add_argument("--ridge", type=float, default=0.1)
    add_classifier_options(p)
    p = sub.add_parser("score", help="write detector scores in the schema of results/detection/b0.csv")
    common(p, False)
    p.add_argument("--model", required=True, help="the .npz of `fit`")
    p = sub.add_parser("features", help="write the raw feature matrices as an .npz")
    common(p, True)
    a = ap.parse_args(argv)
    a.classifier_kw = classifier_keywords(ap, a) if a.command == "fit" else {}
    return a


def main(argv=None) -> None:
    a = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    run = dict(split=a.split, simulate=a.simulate, stream=a.stream, batch_size=a.batch_size, progress_on=a.progress)
    if a.command == "fit":
        model = fit(a.data, a.stego_methods, a.alphas, order=a.order, T=a.T, normalise=a.normalise, ridge=a.ridge, **a.classifier_kw, **run)
        model.save(a.out)
    elif a.command == "score":
        score(a.data, load_model(a.model), a.stego_methods, a.alphas, **run).to_csv(a.out, index=False)
    else:
        opts = dict(order=a.order, T=a.T, normalise=a.normalise, **run)
        rows, F = extract(a.data, **{**opts, "simulate": False})
        arrays = {"cover_names": rows["name"].to_numpy(str), "cover": F}
        for m, al in _sets(a):
            rows, F = extract(a.data, m, al, **opts)
            arrays[f"{m}_{al}_names"], arrays[f"{m}_{al}"] = rows["name"].to_numpy(str), F
        with open(a.out, "wb") as f:
            np.savez(f, order=np.int64(a.order), T=np.int64(a.T), normalise=np.array(a.normalise), **arrays)
    logging.info(f"output saved to {a.out}")


if __name__ == "__main__":
    main()
