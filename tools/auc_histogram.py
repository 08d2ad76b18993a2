"""The detection record of the five histogram detectors (ws_unet_amd.histogram) on the five fixture covers against LSBM and LSBR twins
simulated at alpha 1.0 and 0.5: `histogram score --simulate` writes each score file, and the functions behind `ws.roc --scores`
(load_scores, produce_roc, auc_table, with the covers' alpha filled with 0 as ws.roc's main does) make the AUC and p_e of its sweep over
the thresholds 0..1.  Beside them the rank AUC of the same ten scores (the share of (twin, cover) pairs with the twin above, which needs
no threshold grid) and the number of twins that score above their own cover.  Prints one JSON object.
Usage: python tools/auc_histogram.py > auc_hist.json"""
import json, shutil, sys, tempfile
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
from ws_unet_amd import histogram
from ws_unet_amd.ws import roc

gold = ROOT / "tests" / "golden"
root = Path(tempfile.mkdtemp())
(root / "images").mkdir()
for k in (6, 7, 8, 9, 10):
    shutil.copy(gold / f"cover_{k}.png", root / "images" / f"{k}.png")
(root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in (6, 7, 8, 9, 10)))
out = {}
for det in histogram.DETECTORS:
    for method in ("LSBM", "LSBR"):
        for alpha in (1.0, 0.5):
            csv = root / f"{det}_{method}_{alpha}.csv"
            histogram.main(["score", "--data", str(root), "--detector", det, "--stego-methods", method, "--alphas", str(alpha), "--simulate", "--out", str(csv)])
            s = roc.load_scores(csv, f"B0_{det}", [method], [alpha])
            s["stego_method"] = s["stego_method"].fillna("Cover")
            s["alpha"] = s["alpha"].fillna(0.)                      # as ws.roc's main does
            auc = roc.auc_table(roc.produce_roc(s))
            c, t = s["score"].to_numpy()[:5], s["score"].to_numpy()[5:]
            rank = float(((t[:, None] > c[None, :]).sum() + 0.5 * (t[:, None] == c[None, :]).sum()) / 25.)
            paired = int((t > c).sum())
            out[f"{det} {method} {alpha}"] = {"roc_auc": float(auc["auc"].iloc[0]), "p_e": float(auc["p_e"].iloc[0]), "rank_auc": rank,
                                               "twin_above_its_cover": paired, "covers": c.tolist(), "twins": t.tolist()}
shutil.rmtree(root)
print(json.dumps(out, indent=1))
