"""The FLD ensemble classifier of J. Kodovsky, J. Fridrich, V. Holub, "Ensemble classifiers for steganalysis of digital media", IEEE TIFS
7(2), 2012: L Fisher discriminants, each on a random subset of d_sub features and a bootstrap sample of the training images, a
threshold per learner, a majority vote, and an out-of-bag (OOB) error estimate that chooses d_sub without a validation set.  Not part of
the reference.  It is independent of any feature set; ws_unet_amd.spam and ws_unet_amd.srm subclass it with their feature tags.

The algorithm is the paper's, made deterministic (tests/ensemble_np.py restates it in numpy, draw for draw):

 1. Centring.  Z = the rows of both classes (X0 first), less the mean of all rows, float64, on the host.  zt = Z.T on the device.
    Non-finite features raise.
 2. Groups.  groups0 / groups1 give an integer per row, the image a row comes from.  Default: row i of X0 with rows i, i + n0, ... of X1
    when len(X1) is a multiple of len(X0); otherwise every row is its own group.  The group labels of both classes are renumbered
    0 .. n_groups-1 in ascending order of label.  The bootstrap draws groups: a cover and its stego twins enter or leave a bag together.
 3. Draws.  rng = numpy.random.Generator(numpy.random.Philox(key=seed)).  For each candidate d_sub in the order given, for each learner
    l = 0 .. L-1:  idx_l = sorted(rng.permutation(d)[:d_sub]);  c_l = bincount(rng.integers(0, n_groups, n_groups), minlength=n_groups).
    When either class has total weight 0 under c_l, the learner's whole draw (idx_l, then c_l) is made again from the same stream.
    A row's weight is its group's count.
 4. Scatter and solve, on the device.  G_l = sum_i w_i z_i z_i^T on the learner's features (ops.subspace_gram, K53).  The weighted class
    sums are one float64 matmul of the (L, n) weight matrix with Z per class, gathered to idx_l afterwards; n0, n1 the class's total
    weights, m0, m1 its weighted means.  S_l = (G_l - n0 m0 m0^T - n1 m1 m1^T) / (n0 + n1 - 2), lambda = ridge trace(S_l) / d_sub,
    w_l = (S_l + lambda I)^-1 (m1 - m0) by torch's batched float64 Cholesky (torch.linalg.cholesky_ex) and torch.cholesky_solve learner by
    learner: torch's, not kernels of this library.  A factorisation that fails raises ValueError naming the learner.
 5. Projection.  w_l scattered into a dense (d, L) matrix; P = Z W, one float64 matmul on the device.
 6. Threshold, on the host.  b_l minimises the weighted (P_FA + P_MD) / 2 of the learner's bag (rows of weight > 0) over the midpoints of
    consecutive distinct projections of the bag, a candidate b calling p > b stego; ties to the lowest candidate; the two rates are
    compared as exact integers (FA n1 + MD n0).  A bag with one distinct projection takes it as b.  A learner votes stego when z.w_l > b_l.
 7. Out-of-bag error.  Each training row is judged by the learners whose bag leaves its group out: the majority, a tie half an error;
    rows with no such learner are left out.  oob_error = (P_FA + P_MD) / 2 over the judged rows; a class without a judged row counts 1/2.
 8. With several candidates the one with the least oob_error is kept, ties to the first listed; `oob_errors` has them all.

NOT built: the paper's automatic stopping rule for L and its search schedule for d_sub (both are given by the caller here); no comparison
with the authors' MATLAB, which is not at hand.
"""
from __future__ import annotations

import time
import typing

import numpy as np

CLASSIFIER = "ensemble"


def default_groups(n0: int, n1: int) -> typing.Tuple[np.ndarray, np.ndarray]:
    """step 2's default: (groups0, groups1)"""
    if n0 > 0 and n1 % n0 == 0:
        return np.arange(n0, dtype=np.int64), np.arange(n1, dtype=np.int64) % n0
    return np.arange(n0, dtype=np.int64), n0 + np.arange(n1, dtype=np.int64)


def row_groups(n0: int, n1: int, groups0=None, groups1=None) -> typing.Tuple[np.ndarray, int]:
    """(group, n_groups): per row of [X0; X1] its group renumbered 0 .. n_groups-1 in ascending order of the labels given"""
    if (groups0 is None) != (groups1 is None):
        raise ValueError("fit: give groups0 and groups1, or neither")
    if groups0 is None:
        groups0, groups1 = default_groups(n0, n1)
    g0, g1 = np.asarray(groups0), np.asarray(groups1)
    if g0.shape != (n0,) or g1.shape != (n1,) or g0.dtype.kind not in "iu" or g1.dtype.kind not in "iu":
        raise ValueError(f"fit: groups of shape {g0.shape} {g0.dtype} and {g1.shape} {g1.dtype}: one integer per row, ({n0},) and ({n1},)")
    uniq, inverse = np.unique(np.concatenate([g0, g1]).astype(np.int64), return_inverse=True)
    return inverse.astype(np.int64), len(uniq)


def draw(rng: np.random.Generator, d: int, d_sub: int, group: np.ndarray, n_groups: int, n0: int) -> typing.Tuple[np.ndarray, np.ndarray]:
    """step 3 for one learner: (idx (d_sub,) int64 sorted, c (n_groups,) int64), redrawn while a class has no weight"""
    while True:
        idx = np.sort(rng.permutation(d)[:d_sub])
        c = np.bincount(rng.integers(0, n_groups, n_groups), minlength=n_groups)
        wt = c[group]
        if wt[:n0].sum() > 0 and wt[n0:].sum() > 0:
            return idx.astype(np.int64), c.astype(np.int64)


def draws(seed: int, d: int, d_subs: typing.Sequence[int], learners: int, group: np.ndarray, n_groups: int, n0: int):
    """step 3 for the whole fit: per candidate d_sub (idx (L, d_sub) int64, c (L, n_groups) int64), from one stream"""
    rng = np.random.Generator(np.random.Philox(key=int(seed)))
    out = []
    for ds in d_subs:
        pairs = [draw(rng, d, ds, group, n_groups, n0) for _ in range(learners)]
        out.append((np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])))
    return out


def threshold(p: np.ndarray, y: np.ndarray, wt: np.ndarray) -> float:
    """step 6: p (n,) float64 projections, y (n,) 0 / 1, wt (n,) integer weights of the learner's bag -> b"""
    p, y, wt = np.asarray(p, dtype=np.float64), np.asarray(y), np.asarray(wt).astype(np.int64)
    keep = wt > 0
    p, y, wt = p[keep], y[keep], wt[keep]
    n0, n1 = int(wt[y == 0].sum()), int(wt[y == 1].sum())
    if not n0 or not n1:
        raise ValueError("threshold: a class has no weight in the bag")
    v, inv = np.unique(p, return_inverse=True)
    if len(v) == 1:
        return float(v[0])
    below0 = np.cumsum(np.bincount(inv[y == 0], weights=wt[y == 0], minlength=len(v)).astype(np.int64))    # weights sum exactly in float64
    below1 = np.cumsum(np.bincount(inv[y == 1], weights=wt[y == 1], minlength=len(v)).astype(np.int64))
    cost = (n0 - below0[:-1]) * n1 + below1[:-1] * n0                    # candidate k lies between v[k] and v[k + 1]: FA n1 + MD n0
    k = int(np.argmin(cost))                                            # the first of the smallest: the lowest candidate
    return float((v[k] + v[k + 1]) / 2.)


def oob_error(stego_votes: np.ndarray, in_bag: np.ndarray, y: np.ndarray) -> float:
    """step 7: stego_votes (n, L) bool, in_bag (n, L) bool (the learner's bag holds the row's group), y (n,) 0 / 1"""
    out = ~np.asarray(in_bag, dtype=bool)
    judges = out.sum(axis=1)
    s = (np.asarray(stego_votes, dtype=bool) & out).sum(axis=1)
    y = np.asarray(y)
    err = np.where(2 * s == judges, 0.5, np.where((2 * s > judges) != (y == 1), 1.0, 0.0))
    rates = []
    for cls in (0, 1):
        rows = (judges > 0) & (y == cls)
        rates.append(float(err[rows].mean()) if rows.any() else 0.5)
    return (rates[0] + rates[1]) / 2.


def dense(idx: np.ndarray, w: np.ndarray, d: int) -> np.ndarray:
    """step 5: idx, w (L, d_sub) -> the (d, L) matrix with w[l] at the rows idx[l] of column l"""
    W = np.zeros((d, len(idx)), dtype=np.float64)
    W[idx, np.arange(len(idx))[:, None]] = w
    return W


class Ensemble:
    """Ensemble(learners=51, d_sub, ridge=0.1, seed=0): d_sub an int or a list of ints in 1..d (several: the one with the least OOB error
    is kept); ridge has spam.FLD's meaning and default, untuned as there; 51 learners are odd so that a vote cannot tie, not tuned.
    After `fit`: idx (L, d_sub_chosen) int32, w (L, d_sub_chosen), b (L,), mean (d,), d_sub_chosen, oob_error, oob_errors (one per candidate),
    timings (seconds in 'gram', 'solve', 'projection', 'threshold' of the last fit; device stages are synchronised only when
    `profile` is set).  `votes(F)`: the number of learners voting stego; `output(F)` = votes / L, in 0..1 with 0.5 as the decision."""

    profile = False

    def __init__(self, learners: int = 51, d_sub: typing.Union[int, typing.Sequence[int], None] = None, ridge: float = 0.1, seed: int = 0):
        if isinstance(learners, bool) or int(learners) != learners or learners < 1:
            raise ValueError(f"learners {learners!r} must be a positive integer")
        if not ridge >= 0:
            raise ValueError(f"ridge {ridge!r} must not be negative")
        if d_sub is None:
            raise ValueError("d_sub is required: an int or a list of ints, the features of a base learner")
        cand = [d_sub] if np.ndim(d_sub) == 0 else list(d_sub)
        if not cand or any(isinstance(v, bool) or int(v) != v or v < 1 for v in cand):
            raise ValueError(f"d_sub {d_sub!r}: positive integers expected")
        self.learners, self.d_sub, self.ridge, self.seed = int(learners), [int(v) for v in cand], float(ridge), int(seed)
        self.idx = self.w = self.b = self.mean = None
        self.d_sub_chosen, self.oob_error, self.oob_errors = None, None, []
        self.stego_methods, self.alphas = [], []
        self.timings = dict(gram=0., solve=0., projection=0., threshold=0.)

    # ---- fit ---------------------------------------------------------------------------------------------------------------------------
    def fit(self, X0, X1, groups0=None, groups1=None) -> "Ensemble":
        """X0: the cover class (n0, d), X1: the stego class (n1, d); groups: see the module docstring."""
        import torch
        X0, X1 = np.asarray(X0, dtype=np.float64), np.asarray(X1, dtype=np.float64)
        if X0.ndim != 2 or X1.ndim != 2 or X0.shape[1] != X1.shape[1] or len(X0) + len(X1) < 3 or not len(X0) or not len(X1):
            raise ValueError(f"fit: classes of shape {X0.shape} and {X1.shape}: two (n, d) matrices of one d and at least 3 rows in all")
        n0, n1, d = len(X0), len(X1), X0.shape[1]
        if max(self.d_sub) > d:
            raise ValueError(f"fit: d_sub {max(self.d_sub)} above the {d} features")
        X = np.concatenate([X0, X1])
        if not np.isfinite(X).all():
            raise ValueError("fit: the features hold non-finite values")
        group, n_groups = row_groups(n0, n1, groups0, groups1)
        mean = X.mean(axis=0)
        Z = X - mean
        y = np.concatenate([np.zeros(n0, dtype=np.int64), np.ones(n1, dtype=np.int64)])
        if not torch.cuda.is_available():
            raise RuntimeError("Ensemble.fit runs on the GPU (ops.subspace_gram, K53): no CPU fallback exists")
        Zd = torch.from_numpy(Z).cuda()
        zt = Zd.T.contiguous()
        self.timings = dict(gram=0., solve=0., projection=0., threshold=0.)
        best = None
        self.oob_errors = []
        for ds, (idx, c) in zip(self.d_sub, draws(self.seed, d, self.d_sub, self.learners, group, n_groups, n0)):
            wt = c[:, group]                                                 # (L, n) the rows' weights
            w = self._solve(Zd, zt, idx, wt, n0)
            t0 = self._clock()
            P = (Zd @ torch.from_numpy(dense(idx, w, d)).cuda()).cpu().numpy()      # (n, L)
            self.timings["projection"] += self._clock() - t0
            t0 = time.perf_counter()
            b = np.array([threshold(P[:, l], y, wt[l]) for l in range(self.learners)])
            err = oob_error(P > b[None, :], wt.T > 0, y)
            self.timings["threshold"] += time.perf_counter() - t0
            self.oob_errors.append(err)
            if best is None or err < best[0]:
                best = (err, ds, idx, w, b)
        self.oob_error, self.d_sub_chosen, idx, self.w, self.b = best
        self.idx, self.mean = idx.astype(np.int32), mean
        return self

    def _clock(self) -> float:
        if self.profile:
            import torch
            torch.cuda.synchronize()
        return time.perf_counter()

    def _solve(self, Zd, zt, idx: np.ndarray, wt: np.ndarray, n0: int, max_bytes: typing.Optional[int] = None) -> np.ndarray:
        """step 4: idx (L, d_sub), wt (L, n) -> w (L, d_sub) float64 on the host"""
        import torch
        from . import ops
        L, ds = idx.shape
        dev = Zd.device
        idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
        wt_d = torch.from_numpy(np.ascontiguousarray(wt, dtype=np.int32)).to(dev)
        max_bytes = ops.SUBSPACE_GRAM_MAX_BYTES if max_bytes is None else max_bytes
        per = max(1, max_bytes // (8 * ds * ds))
        wf = wt_d.double()
        N0, N1 = wf[:, :n0].sum(dim=1), wf[:, n0:].sum(dim=1)                # (L,) the classes' total weights
        gather = idx_d.long()
        m0 = torch.gather(wf[:, :n0] @ Zd[:n0], 1, gather) / N0[:, None]    # (L, d_sub) the weighted class means on the learner's features
        m1 = torch.gather(wf[:, n0:] @ Zd[n0:], 1, gather) / N1[:, None]
        out = torch.empty((L, ds), dtype=torch.float64, device=dev)
        eye = torch.eye(ds, dtype=torch.float64, device=dev)
        for l0 in range(0, L, per):
            sl = slice(l0, min(l0 + per, L))
            t0 = self._clock()
            G = ops.subspace_gram(zt, idx_d[sl], wt_d[sl], max_bytes=max_bytes)
            t1 = self._clock()
            a, bb = m0[sl], m1[sl]
            S = G.sub_(N0[sl, None, None] * a[:, :, None] * a[:, None, :]).sub_(N1[sl, None, None] * bb[:, :, None] * bb[:, None, :])
            S.div_((N0[sl] + N1[sl] - 2.)[:, None, None])
            lam = self.ridge * torch.diagonal(S, dim1=1, dim2=2).sum(dim=1) / ds
            S.add_(lam[:, None, None] * eye)
            chol, info = torch.linalg.cholesky_ex(S)
            bad = torch.nonzero(info).flatten().tolist()
            if bad:
                raise ValueError(f"fit: the regularised scatter of learner {l0 + bad[0]} (d_sub {ds}) is not positive definite: "
                                 f"use a ridge above 0 (it is {self.ridge})")
            # the two triangular solves learner by learner: torch's BATCHED cholesky_solve ended with a HIP launch failure on a
            # (51, 200, 200) batch with one right-hand side on gfx950 (torch 2.x for ROCm); the single-matrix call takes another path
            rhs = (bb - a)[:, :, None]
            for k in range(len(chol)):
                out[l0 + k] = torch.cholesky_solve(rhs[k], chol[k])[:, 0]
            self.timings["gram"] += t1 - t0
            self.timings["solve"] += self._clock() - t1
        return out.cpu().numpy()

    # ---- use ---------------------------------------------------------------------------------------------------------------------------
    def _fitted(self):
        if self.w is None:
            raise ValueError("this Ensemble is not fitted")

    def votes(self, F) -> np.ndarray:
        """(N,) int64: the learners voting stego, z.w_l > b_l with z = F - mean"""
        self._fitted()
        F = np.asarray(F, dtype=np.float64)
        if F.ndim != 2 or F.shape[1] != len(self.mean):
            raise ValueError(f"votes: features of shape {F.shape}, expected (N, {len(self.mean)})")
        return (((F - self.mean) @ dense(self.idx, self.w, len(self.mean))) > self.b[None, :]).sum(axis=1).astype(np.int64)

    def output(self, F) -> np.ndarray:
        return self.votes(F) / float(self.learners)

    # ---- files -------------------------------------------------------------------------------------------------------------------------
    def _tags(self) -> dict:
        """the arrays a subclass adds to the file: its feature tags"""
        return {}

    def save(self, path) -> None:
        """An .npz of arrays only: classifier = 'ensemble', idx, w, b, mean, d_sub (the chosen one), d_sub_candidates, oob_error,
        oob_errors, learners, ridge, seed, the stego methods and alphas of the training set, and the subclass's feature tags."""
        self._fitted()
        with open(path, "wb") as f:
            np.savez(f, classifier=np.array(CLASSIFIER), idx=self.idx, w=self.w, b=self.b, mean=self.mean, d_sub=np.int64(self.d_sub_chosen),
                     d_sub_candidates=np.array(self.d_sub, dtype=np.int64), oob_error=np.float64(self.oob_error),
                     oob_errors=np.array(self.oob_errors, dtype=np.float64), learners=np.int64(self.learners), ridge=np.float64(self.ridge),
                     seed=np.int64(self.seed), stego_methods=np.array(list(self.stego_methods), dtype=str),
                     alphas=np.array(list(self.alphas), dtype=np.float64), **self._tags())

    def _read(self, z, path) -> "Ensemble":
        """fill a constructed model from the open file `z`"""
        self.idx, self.w = np.array(z["idx"], dtype=np.int32), np.array(z["w"], dtype=np.float64)
        self.b, self.mean = np.array(z["b"], dtype=np.float64), np.array(z["mean"], dtype=np.float64)
        self.d_sub_chosen, self.oob_error = int(z["d_sub"]), float(z["oob_error"])
        self.oob_errors = [float(v) for v in z["oob_errors"]]
        self.stego_methods, self.alphas = [str(s) for s in z["stego_methods"]], [float(a) for a in z["alphas"]]
        L, ds, d = self.learners, self.d_sub_chosen, len(self.mean)
        if self.idx.shape != (L, ds) or self.w.shape != (L, ds) or self.b.shape != (L,) or self.mean.ndim != 1 or (
                self.idx.size and (self.idx.min() < 0 or self.idx.max() >= d)):
            raise ValueError(f"{path}: idx {self.idx.shape}, w {self.w.shape}, b {self.b.shape} do not fit {L} learners of {ds} out of {d} features")
        return self

    @staticmethod
    def _require(z, path) -> None:
        if "classifier" not in z.files or str(z["classifier"]) != CLASSIFIER:
            raise ValueError(f"{path}: not an ensemble model (no classifier = {CLASSIFIER!r} entry); an FLD file is read by FLD.load or load_model")

    @classmethod
    def load(cls, path) -> "Ensemble":
        with np.load(path, allow_pickle=False) as z:
            cls._require(z, path)
            return cls(int(z["learners"]), [int(v) for v in z["d_sub_candidates"]], float(z["ridge"]), int(z["seed"]))._read(z, path)


def is_ensemble_file(path) -> bool:
    """whether the .npz at `path` has classifier = 'ensemble'"""
    with np.load(path, allow_pickle=False) as z:
        return "classifier" in z.files and str(z["classifier"]) == CLASSIFIER


def refuse_ensemble(z, path, who: str) -> None:
    """the one check FLD.load adds: ValueError when the open file `z` is an ensemble's"""
    if "classifier" in z.files and str(z["classifier"]) == CLASSIFIER:
        raise ValueError(f"{path}: an ensemble model (classifier = {CLASSIFIER!r}), not an FLD: {who}.load_model reads both kinds")


def stem_groups(names0, names1) -> typing.Tuple[np.ndarray, np.ndarray]:
    """(groups0, groups1) for the drivers: rows whose file names have the same stem are one group (a cover and its stego twins)"""
    import pathlib
    s0, s1 = [pathlib.Path(str(n)).stem for n in names0], [pathlib.Path(str(n)).stem for n in names1]
    number = {s: i for i, s in enumerate(sorted(set(s0) | set(s1)))}
    return np.array([number[s] for s in s0], dtype=np.int64), np.array([number[s] for s in s1], dtype=np.int64)
