"""Prediction-error table of the reference, results/prediction/filters.csv (src/filters/evaluate.py:182-205 `__main__`):

    python -m ws_unet_amd.prediction_error --data DATA --out filters.csv [--model-path DIR --model-name NAME]

One row per cover image and filter (AVG, KB on the Y plane) with `fname`, `mae_3_<filter>`, `wmae_3_<filter>` and fabrika's
name / height / width, in the reference's row order and layout.  With --model-path / --model-name, rows of the UNet
(src/predictor_error.py:19-76 `attack`: filter='UNet', mae, wmae) follow.  Everything is computed on the GPU.
"""
from __future__ import annotations

import argparse
import logging
import pathlib


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--data", required=True, help="dataset root with images*/files.csv (the reference's ../data)")
    ap.add_argument("--out", required=True, help="output CSV (the reference writes results/prediction/filters.csv)")
    ap.add_argument("--filters", nargs="*", default=["AVG", "KB"])
    ap.add_argument("--per-image", action="store_true", help="one launch chain per image instead of one per chunk of 32")
    ap.add_argument("--model-path", default=None, help="directory holding <model-name>/config.json and model/best_model.pt.tar")
    ap.add_argument("--model-name", default=None)
    ap.add_argument("--mode", default=None, help="UNet inference mode (default: the package default)")
    ap.add_argument("--progress", action="store_true")
    from .ols import add_kernels_argument
    add_kernels_argument(ap)
    return ap


def parse_args(argv=None) -> argparse.Namespace:
    return _parser().parse_args(argv)


def main(argv=None) -> None:
    ap = _parser()
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)

    import pandas as pd
    from . import evaluate, filters, ols
    ols.register_from_args(a)
    data = pathlib.Path(a.data)
    iterator = "python" if a.per_image else "batched"
    res = filters.run(data, filter_names=a.filters, channels=[[3]] * len(a.filters), iterator=iterator, progress_on=a.progress)
    if a.model_path or a.model_name:
        if not (a.model_path and a.model_name):
            ap.error("--model-path and --model-name go together")
        model = evaluate.get_pretrained(a.model_path, (3,), model_name=a.model_name, mode=a.mode)
        fn = evaluate.predict_unet_error_cover if a.per_image else evaluate.predict_unet_error_cover_batched
        res = pd.concat([res, fn(data, model=model, progress_on=a.progress)])
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res.to_csv(out, index=False)
    logging.info(f"output saved to {out}")


if __name__ == "__main__":
    main()
