"""Detection ROC and AUC tables of the reference, results/detection/auc_<alpha>.csv and roc_<alpha>.csv (src/ws/roc.py):

    python -m ws_unet_amd.ws.roc --data DATA --out-dir DIR [--model-dir DIR] [--scores b0.csv B0_0.01 ...]

How well does a WS payload estimate, made with each pixel predictor (AVG, KB, UNet), separate covers from stegos, next to a CNN
detector's score?  Per (stego method, model) the covers and that method's stegos of every alpha are pooled into one curve, swept over
the 501 thresholds of linspace(0, 1, 501) from 1 down to 0.  `produce_roc` restates roc.py:198-283 without fixing it:

  * groups in groupby(['stego_method', 'model_name']) order, 'Cover' skipped; a group uses the model's rows of its method and 'Cover';
  * 'B0' in the model name: y_hat = score, y = alpha; otherwise y_hat = clip(beta_hat, 0), y = alpha / 2; positive means y > 0;
  * tpr = TP / (TP + FN), fpr = FP / (FP + TN) (0/0 = NaN); bins = diff(fpr, prepend=fpr[0]) / its sum, auc = sum(bins * tpr);
  * p_e, tau0, fpr_tau0, tpr_tau0 at the first argmin of (1 - tpr + fpr) / 2 in descending-tau order (the first NaN if there is one);
  * fpr_50 / tpr_50 at tau = 0.5 with the reference's stale FN: tpr_50 = TP_0.5 / (TP_0.5 + FN at tau = 0), because roc.py:247-251
    never recomputes FN after the loop (when every positive scores in (0, 0.5] this is 0/0 = NaN, not 0).

The confusion counts of every group and threshold come from ONE call of K19 (wsu_roc_counts, exact integer counts of s > tau in
float64); the host forms the rates and the table in fp64 with numpy, in the reference's array order.  The B0 detector itself is out of
scope: its scores enter as files in the schema of results/detection/b0.csv (`load_scores`, `--scores`).  The structural estimators of
ws/structural.py ('SPA', 'RS') are further curves: rows like a predictor's (beta_hat = the estimated change rate), labelled by their own names.

`collect_ws_scores` is the reference main's WS half (roc.py:372-395): ws.estimate.run per (image set, predictor), unweighted, without
bias correction, on the Y plane -- but every image is decoded and uploaded once and all predictors score the device batch.
"""
from __future__ import annotations

import argparse
import logging
import pathlib
import typing

import numpy as np

from .. import fabrika
from .. import filters as filters_lib
from ..imread import imread4_u8
from ..planes import load_planes_u8, upload_planes
from ..unet_run import model_device
from . import adaptive, predictors, sequential, structural

TAUS = np.linspace(0, 1, 501, endpoint=True)       # ascending; the reference walks them reversed
AUC_COLUMNS = ["stego_method", "model_name", "auc", "p_e", "tau0", "fpr_tau0", "tpr_tau0", "fpr_50", "tpr_50"]
STEGO_METHODS = ("LSBR",)
ALPHAS = (.1, .05, .01)
WS_FILTERS = ("AVG", "KB")


# ---- produce_roc --------------------------------------------------------------------------------------------------------------

def _groups(df_ws) -> typing.List[typing.Tuple[str, str, np.ndarray, np.ndarray]]:
    """(stego_method, model_name, y_hat float64, labels int8) per curve, in the reference's group and row order.  labels: 1 where
    y > 0, 0 where y <= 0, -1 where y is NaN (in neither class, as numpy's comparisons leave it)."""
    out = []
    for (stego_method, model_name), _ in df_ws.groupby(["stego_method", "model_name"]):
        if stego_method == "Cover":
            continue
        d = df_ws[df_ws["model_name"] == model_name]
        d = d[d["stego_method"].isin([stego_method, "Cover"])]
        if "B0" in model_name:
            y_hat = np.asarray(d["score"].to_numpy(), dtype=np.float64)
            y = np.asarray(d["alpha"].to_numpy(), dtype=np.float64)
        else:
            # a float32 estimate widened exactly: NumPy 2 compares it with an np.float64 tau in float64 (NEP 50)
            y_hat = np.clip(np.asarray(d["beta_hat"].to_numpy(), dtype=np.float64), 0, None)
            y = np.asarray(d["alpha"].to_numpy(), dtype=np.float64) / 2
        labels = np.where(y > 0., 1, np.where(y <= 0., 0, -1)).astype(np.int8)
        out.append((stego_method, model_name, y_hat, labels))
    return out


def _kernel_taus(taus: np.ndarray) -> typing.Tuple[np.ndarray, np.ndarray, int]:
    """The ascending thresholds handed to K19 (the grid and 0.5), the grid's positions in them and the position of 0.5."""
    k = np.union1d(taus, [.5])
    return k, np.searchsorted(k, taus), int(np.searchsorted(k, .5))


def _device_counts(groups, ktaus: np.ndarray) -> np.ndarray:
    """(G, len(ktaus), 4) int64 {TP, FP, TN, FN} of every group in one K19 call."""
    import torch
    from .. import ops
    offsets = np.concatenate([[0], np.cumsum([len(g[2]) for g in groups])]).astype(np.int64)
    scores = torch.from_numpy(np.ascontiguousarray(np.concatenate([g[2] for g in groups]))).cuda()
    labels = torch.from_numpy(np.ascontiguousarray(np.concatenate([g[3] for g in groups]))).cuda()
    return ops.roc_counts(scores, labels, offsets, ktaus).cpu().numpy()


def roc_rows(stego_method: str, model_name: str, taus_desc: np.ndarray, counts: np.ndarray, counts_50: np.ndarray):
    """One group's frame of roc.py:232-280 from its confusion counts: counts (T, 4) int64 {TP, FP, TN, FN} at taus_desc (the
    reference's loop order, tau descending), counts_50 (4,) at tau = 0.5.  fp64 numpy in the reference's order of operations."""
    import pandas as pd
    TP, FP, TN, FN = (np.asarray(counts[:, c], dtype=np.int64) for c in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        tpr = TP / (TP + FN)
        fpr = FP / (FP + TN)
        bins = np.diff(fpr, prepend=fpr[0])
        bins /= bins.sum()
        auc = np.sum(bins * tpr)
        tau0_idx = np.argmin((1 - tpr + fpr) / 2)
        p_e = ((1 - tpr + fpr) / 2)[tau0_idx]
        tp50, fp50, tn50 = (np.int64(counts_50[c]) for c in range(3))
        fn_stale = np.int64(FN[-1])                           # FN of the loop's last tau, not of 0.5 (roc.py:247-251)
        fpr50, tpr50 = fp50 / (fp50 + tn50), tp50 / (tp50 + fn_stale)
    label = model_name if "B0" in model_name or model_name in structural.NAMES else f"WS-{model_name}"
    return pd.DataFrame({
        "stego_method": stego_method,
        "model_name": model_name,
        "tau": taus_desc,
        "tpr": tpr,
        "fpr": fpr,
        "p_e": p_e,
        "tau0": taus_desc[tau0_idx],
        "fpr_tau0": fpr[tau0_idx],
        "tpr_tau0": tpr[tau0_idx],
        "auc": auc,
        "fpr_50": fpr50,
        "tpr_50": tpr50,
        "label": label,
    })


def _roc_frame(groups, counts: np.ndarray, taus: np.ndarray = TAUS):
    """produce_roc's frame from the groups (_groups) and their counts at the ascending thresholds of _kernel_taus(taus)."""
    import pandas as pd
    _, at_grid, at_50 = _kernel_taus(taus)
    taus_desc = np.array(list(reversed(taus)))
    frames = [roc_rows(sm, mn, taus_desc, counts[g][at_grid][::-1], counts[g][at_50]) for g, (sm, mn, _, _) in enumerate(groups)]
    return pd.concat(frames)


def produce_roc(df_ws):
    """roc.py:198-283 `produce_roc` (without the progress print): per (stego_method, model_name) the ROC over TAUS and its summary
    columns, one frame of 501 rows per group, concatenated.  df_ws: WS rows (model_name, stego_method, alpha, beta_hat) and
    detector rows (a model_name containing 'B0', score), covers marked stego_method 'Cover'."""
    import pandas as pd
    groups = _groups(df_ws)
    if not groups:
        return pd.concat([])                                  # the reference's "No objects to concatenate"
    ktaus, _, _ = _kernel_taus(TAUS)
    return _roc_frame(groups, _device_counts(groups, ktaus), TAUS)


def auc_table(df_roc):
    """results/detection/auc_<alpha>.csv (roc.py:456-457), written with index=False."""
    return df_roc[AUC_COLUMNS].drop_duplicates()


def roc_table(df_roc):
    """results/detection/roc_<alpha>.csv (roc.py:460-466): tau ascending, the tpr_<method>_<model> columns, then the fpr_ ones;
    written with index=False."""
    df = df_roc.pivot(index=["tau"], columns=["stego_method", "model_name"], values=["tpr", "fpr"])
    df.columns = ["_".join(col).strip() for col in df.columns.values]
    return df


# ---- WS scores of every predictor from one decode ------------------------------------------------------------------------------

def _prefetch(fnames, kws):
    return (load_planes_u8(fnames),)


def _submit(fnames, clean, *, predictors, placement="random", order="rows", criterion="hill", flip_rate=1.0, prefetched=None):
    """Upload the chunk once and queue every predictor's statistic (ws.estimate._stat) on it; nothing waits for the GPU.  A ragged
    chunk goes through ws.estimate.attack image by image, as ws.estimate.attack_batch does."""
    from . import estimate
    planes = prefetched[0] if prefetched is not None else load_planes_u8(fnames)
    if planes is None:
        proc = filters_lib.get_processor_2d((3,))
        return "host", [[estimate.attack(f, (3,), est, estimate.NAMED_FILTERS["AVG"], False, 0, imread4_u8, proc, placement, order,
                                        criterion, flip_rate, **{**kw, "model_name": name})
                         for name, est in predictors] for f, kw in zip(fnames, clean)]
    x = upload_planes(planes, model_device(estimate.unet_model_of(predictors[-1][1])))
    betas = []
    for _, est in predictors:
        try:
            betas.append(estimate._stat(x, est, estimate.NAMED_FILTERS["AVG"], 0, False, placement=placement, order=order, criterion=criterion,
                                        flip_rate=flip_rate))
        except ValueError:                                   # ws.estimate.attack_batch: no estimate for this chunk
            betas.append(None)
    return "device", (clean, [name for name, _ in predictors], betas, estimate._placement_tail(placement, order, criterion, flip_rate))


def _collect(handle):
    """Per row of the chunk: the row dict of ws.estimate.attack_batch for every predictor."""
    kind, val = handle
    if kind == "host":
        return val
    clean, names, betas, placed = val
    betas = [b.cpu().numpy() if b is not None else [None] * len(clean) for b in betas]
    tail = {"channels": "3", "weighted": 0, "correct_bias": False} | placed
    return [[{**kw, "model_name": name, "beta_hat": betas[p][i], **tail} for p, name in enumerate(names)] for i, kw in enumerate(clean)]


def _score_chunk(fnames, kws, prefetched=None, **shared):
    return _collect(_submit(fnames, kws, prefetched=prefetched, **shared))


_score_chunk.submit, _score_chunk.collect = _submit, _collect
_score_chunk = fabrika.shared_kwargs(_score_chunk, ("predictors", "placement", "order", "criterion", "flip_rate"), _prefetch)
_score_covers = fabrika.precovers(iterator="batched", convert_to=None, ignore_missing=True)(_score_chunk)
_score_stegos = fabrika.stego_spatial(iterator="batched", convert_to=None, ignore_missing=True)(_score_chunk)


def collect_ws_scores(input_dir, stego_methods: typing.Sequence[str] = STEGO_METHODS, alphas: typing.Sequence[float] = ALPHAS,
                      filters: typing.Sequence[str] = WS_FILTERS, unet=None, mode: str = None, progress_on: bool = False,
                      placement: str = "random", order: str = "rows", criterion: str = "hill", flip_rate: float = 1.0, **kw):
    """The WS rows the reference's main concatenates (roc.py:372-395): for the cover set, then each stego method x alpha, the rows of
    ws.estimate.run(..., weighted=0, correct_bias=False, channels=(3,), batched=True) of each named filter (or structural estimator,
    'SPA' / 'RS', whose curves are labelled with their own names, not 'WS-<name>') and then of the UNet
    (model_name 'UNet'), concatenated, index reset, stego_method NaN -> 'Cover', alpha NaN -> 0.  The same frame, but each image is
    decoded (native PNG reader, one chunk ahead) and uploaded once, and every predictor's statistic runs on that device batch.
    unet: None (no UNet rows), a ws.estimate.UNetEstimator, a model, or (model_path, model_name) of a trained run loaded in
    inference `mode`.  placement='sequential' (with `order`) scores every image with the changepoint estimator of ws/sequential.py instead
    (pixel predictors only); the rows then also carry `placement` and `order`.  placement='adaptive' (with `criterion` and `flip_rate`) scores
    with the estimator of ws/adaptive.py along the recomputed cost order; the rows then carry `placement`, `criterion` and `flip_rate`.
    Other keywords go to the fabrika iterators (take_num_images, split, ...)."""
    import pandas as pd
    from . import estimate
    preds = [(name, predictors.require(name)) for name in filters]
    est = estimate.as_unet_estimator(unet, mode)
    if est is not None:
        preds.append(("UNet", est))
    if not preds:
        raise ValueError("no predictor: give filters and / or a UNet")
    for _, p in preds:                                       # an option a predictor does not have is an error up front, not an empty curve
        estimate._check_options(p, 0, False, placement, order, criterion, flip_rate)
    placed = dict(placement=placement, order=order) if placement != "random" else {}
    if placement == "adaptive":
        placed = dict(placement=placement, criterion=criterion, flip_rate=flip_rate)
    frames = []
    for stego_method, alpha in [(None, None)] + [(sm, al) for sm in stego_methods for al in alphas]:
        if stego_method:
            rows = _score_stegos(input_dir, inbayer=None, stego_method=stego_method, alpha=alpha, model_name=None, predictors=preds,
                                 progress_on=progress_on, **placed, **kw)
        else:
            rows = _score_covers(input_dir, inbayer=None, model_name=None, predictors=preds, progress_on=progress_on, **placed, **kw)
        for p in range(len(preds)):                          # ws.estimate.run's frame of predictor p on this set
            res = pd.DataFrame([r[p] for r in rows])
            res["channels"] = "3"
            frames.append(res[~res.beta_hat.isna()])
    res = pd.concat(frames).reset_index(drop=True)
    res["stego_method"] = res["stego_method"].fillna("Cover") if "stego_method" in res else "Cover"
    res["alpha"] = res["alpha"].fillna(0.) if "alpha" in res else 0.
    return res



# ---- detector scores (results/detection/b0.csv) ---------------------------------------------------------------------------------

def load_scores(path, name: str, stego_methods: typing.Sequence[str] = STEGO_METHODS, alphas: typing.Sequence[float] = ALPHAS):
    """Detector outputs in the schema of results/detection/b0.csv (name, ..., output, stego_method, alpha) as produce_roc rows
    {..., model_name=name, score=output}: the cover rows (empty stego_method) and the rows of the given stego methods and alphas,
    covers first, then method by method and alpha by alpha (the reference's run order).  `name` must contain 'B0': that is how
    produce_roc tells a detector score from a WS estimate."""
    import pandas as pd
    if "B0" not in name:
        raise ValueError(f"scores name {name!r} must contain 'B0' (produce_roc reads a model without it as a WS estimate)")
    df = pd.read_csv(path, float_precision="round_trip")
    for col in ("output", "stego_method", "alpha"):
        if col not in df.columns:
            raise ValueError(f"{path}: no {col!r} column (expected the schema of results/detection/b0.csv)")
    parts = [df[df["stego_method"].isna()]]
    parts += [df[(df["stego_method"] == sm) & (df["alpha"] == al)] for sm in stego_methods for al in alphas]
    res = pd.concat(parts).assign(model_name=name)
    res["score"] = res["output"].astype(np.float64)
    return res


# ---- CLI ------------------------------------------------------------------------------------------------------------------------

def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(
        description="WS detection ROC / AUC tables (results/detection/auc_<alpha>.csv, roc_<alpha>.csv).  All alphas of a stego method "
                    "are pooled into one curve; the files are named after the LAST alpha, as the reference names them.")
    ap.add_argument("--data", required=True, help="dataset root with images*/ and stego*/ files.csv (the reference's ../data)")
    ap.add_argument("--out-dir", required=True, help="output directory (the reference writes results/detection/)")
    ap.add_argument("--model-dir", default=None, help="trained UNets in the reference's layout <dir>/<train method>/<run>/"
                                                      "{config.json,model/best_model.pt.tar}; no UNet rows without it")
    ap.add_argument("--train-method", default="LSBR", help="stego method the UNet was trained on (its run under --model-dir)")
    ap.add_argument("--stego-methods", nargs="*", default=list(STEGO_METHODS))
    ap.add_argument("--alphas", nargs="+", type=float, default=list(ALPHAS),
                    help="pooled into one curve per stego method; the LAST one names the output files")
    ap.add_argument("--filters", nargs="*", default=list(WS_FILTERS), help=predictors.filters_help(structural=True))
    ap.add_argument("--scores", nargs=2, action="append", default=[], metavar=("FILE", "NAME"),
                    help="detector scores in the schema of results/detection/b0.csv (the `output` column; covers have an empty "
                         "stego_method) added as model NAME, which must contain 'B0'; repeatable")
    ap.add_argument("--mode", default=None, help="UNet inference mode (default: the package default)")
    ap.add_argument("--progress", action="store_true")
    ap.add_argument("--placement", choices=sequential.PLACEMENTS, default="random",
                    help="where the payload is assumed to lie: spread uniformly (the WS statistic), in the first pixels of the file order, or "
                         "in the pixels of lowest cost under --criterion, recomputed from each image under attack")
    ap.add_argument("--order", choices=sequential.ORDERS, default="rows", help="sequential placement: rows from the top, or from the bottom")
    ap.add_argument("--criterion", choices=adaptive.CRITERIA, default="hill", help="adaptive placement: the cost that orders the pixels")
    ap.add_argument("--flip-rate", type=float, default=1.0,
                    help="adaptive placement: the probability that a used pixel was flipped (1: HILLR flips every used pixel; 0.5: a real message)")
    predictors.add_arguments(ap)
    return ap.parse_args(argv)


def main(argv=None) -> None:
    import pandas as pd
    a = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    predictors.register_from_args(a)
    detectors = [load_scores(path, name, a.stego_methods, a.alphas) for path, name in a.scores]      # input errors before GPU work
    unet = None
    if a.model_dir:
        from ..evaluate import trained_runs
        (method, model_name, _), = trained_runs(a.model_dir, [a.train_method])
        unet = (pathlib.Path(a.model_dir) / method, model_name)
    res = collect_ws_scores(a.data, a.stego_methods, a.alphas, a.filters, unet=unet, mode=a.mode, progress_on=a.progress, placement=a.placement,
                            order=a.order, criterion=a.criterion, flip_rate=a.flip_rate)
    res = pd.concat([res] + detectors).reset_index(drop=True)
    res["stego_method"] = res["stego_method"].fillna("Cover")
    res["alpha"] = res["alpha"].fillna(0.)
    df_roc = produce_roc(res)
    out = pathlib.Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    alpha = a.alphas[-1]
    auc_table(df_roc).to_csv(out / f"auc_{alpha}.csv", index=False)
    roc_table(df_roc).to_csv(out / f"roc_{alpha}.csv", index=False)
    logging.info(f"output saved to {out / f'auc_{alpha}.csv'} and {out / f'roc_{alpha}.csv'}")


if __name__ == "__main__":
    main()
