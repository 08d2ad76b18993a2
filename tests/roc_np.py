"""numpy restatement of the reference's threshold sweep (src/ws/roc.py:198-283 `produce_roc`): the yardstick of K19 and of the host
side of ws_unet_amd.ws.roc.  Plain loops over tau with numpy's comparisons, as the reference writes them."""
import numpy as np
import pandas as pd

TAUS = np.linspace(0, 1, 501, endpoint=True)


def counts(y_hat, labels, taus) -> np.ndarray:
    """(len(taus), 4) int64 {TP, FP, TN, FN} at each tau, in the order given: the reference's four np.sum of masks, with y > 0 / y <= 0
    written as labels 1 / 0 (-1: y is NaN, in neither)."""
    y_hat = np.asarray(y_hat)
    pos, neg = np.asarray(labels) == 1, np.asarray(labels) == 0
    out = np.empty((len(taus), 4), dtype=np.int64)
    for j, tau in enumerate(taus):
        out[j] = (np.sum((y_hat > tau) & pos), np.sum((y_hat > tau) & neg), np.sum((y_hat <= tau) & neg), np.sum((y_hat <= tau) & pos))
    return out


def group_counts(y_hats, labels, taus) -> np.ndarray:
    """(G, T, 4) counts of several groups (what one K19 call returns for them)."""
    return np.stack([counts(s, lab, taus) for s, lab in zip(y_hats, labels)]) if len(y_hats) else np.zeros((0, len(taus), 4), np.int64)


def roc_group(stego_method, model_name, y_hat, y, taus=TAUS) -> pd.DataFrame:
    """The reference's loop body for one group (roc.py:218-280), print and plot left out."""
    tpr, fpr, taus_out = [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for tau in reversed(taus):
            TP = np.sum((y_hat > tau) & (y > 0.))
            FP = np.sum((y_hat > tau) & (y <= 0.))
            TN = np.sum((y_hat <= tau) & (y <= 0.))
            FN = np.sum((y_hat <= tau) & (y > 0.))
            taus_out.append(tau)
            tpr.append(TP / (TP + FN))
            fpr.append(FP / (FP + TN))
        tpr, fpr = np.array(tpr), np.array(fpr)
        taus_out = np.array(taus_out)
        bins = np.diff(fpr, prepend=fpr[0])
        bins /= bins.sum()
        auc = np.sum(bins * tpr)
        tau0_idx = np.argmin((1 - tpr + fpr) / 2)
        p_e = ((1 - tpr + fpr) / 2)[tau0_idx]
        TP = np.sum((y_hat > .5) & (y > 0.))
        FP = np.sum((y_hat > .5) & (y <= 0.))
        TN = np.sum((y_hat <= .5) & (y <= 0.))
        fpr50, tpr50 = FP / (FP + TN), TP / (TP + FN)
    label = model_name if "B0" in model_name else f"WS-{model_name}"
    return pd.DataFrame({"stego_method": stego_method, "model_name": model_name, "tau": taus_out, "tpr": tpr, "fpr": fpr, "p_e": p_e,
                         "tau0": taus_out[tau0_idx], "fpr_tau0": fpr[tau0_idx], "tpr_tau0": tpr[tau0_idx], "auc": auc, "fpr_50": fpr50,
                         "tpr_50": tpr50, "label": label})


def produce_roc(df_ws: pd.DataFrame) -> pd.DataFrame:
    """roc.py:198-283 as written."""
    df = []
    for (stego_method, model_name), _ in df_ws.groupby(["stego_method", "model_name"]):
        if stego_method == "Cover":
            continue
        d = df_ws[df_ws["model_name"] == model_name]
        d = d[d["stego_method"].isin([stego_method, "Cover"])]
        if "B0" in model_name:
            y_hat = d["score"].to_numpy()
            y = d["alpha"].to_numpy()
        else:
            y_hat = np.clip(d["beta_hat"].to_numpy(), 0, None)
            y = d["alpha"].to_numpy() / 2
        df.append(roc_group(stego_method, model_name, y_hat, y))
    return pd.concat(df)
