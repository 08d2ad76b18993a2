"""Training driver for the UNet runs: `python -m ws_unet_amd.train ...` or, data-parallel on one node,
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 -m ws_unet_amd.train ...`.

The reference publishes no UNet driver; this follows the structure of its detector driver
(src/detector/train.py:143-304: run directory naming, config.json dump, log/ + model/ sub-directories, optional weight-only
resume, epoch loop with reshuffle / validate / checkpoint / best copy / patience) and takes the keys of the published run configs
(models/unet/*/config.json) under the same names, so a published config replays with `--config <file> --dataset <dir>`.

`batch_size` is the GLOBAL batch as in the published configs (16); with N ranks every rank runs batch_size / N samples per step and
the flat gradient bucket is sum-all-reduced over RCCL (parallel.allreduce_flat_).  The UniformDropout mask stream is seeded per
rank (seed * world + rank) and advances with the call counter, so replicas draw different masks and a run is reproducible.
"""
from __future__ import annotations

import argparse
import json
import pathlib
import time
import typing

import torch

from . import parallel
from .data.pairs import PairLoader
from .model import get_model
from .trainer import Trainer, create_run_name, resume

DEFAULTS: typing.Dict[str, typing.Any] = {
    "SLURM_JOB_ID": "0", "alpha": None, "batch_size": 16, "channel": [0], "covers_only": False, "dataset": None,
    "demosaic": None, "demosaic_oracle": False, "drop_rate": 0.0, "experiment_dir_suffix": None, "grayscale": True,
    "learning_rate": 1e-4, "loss": "l1ws", "loss_lambda": 0.25, "network": "unet_2", "num_epochs": 300, "output_dir": "runs",
    "patience": 10, "resume": None, "resume_dir": None, "seed": None, "stego_method": None, "tr_csv": "split_tr.csv",
    "va_csv": "split_va.csv", "take_num_images": None, "mode": None, "train_mode": None,
    "simulate_stego": False,         # make the stego samples on the device from the covers (data/pairs.py simulate=True): no stego_* folders needed
    # the published configs' augmentation and payload keys (data/pairs.py): random flips / rot90 per training pair; a list of payloads and / or
    # methods of which every pair draws one per epoch.  A list that is not null overrides `alpha` / `stego_method`.
    "post_flip": False, "post_rotate": False, "alphas": None, "stego_methods": None,
    # side-information planes behind the image (data/pairs.py; the reference's ParityOracle; `demosaic_oracle` above is its DemosaicOracle)
    "parity_oracle": False,
}
# written to config.json only when set, so that the config file of every run that does not use them is what it was
OPTIONAL_KEYS = ("simulate_stego", "post_flip", "post_rotate", "alphas", "stego_methods", "parity_oracle")
LIST_FLAGS = {"alphas": float, "stego_methods": str}
# Whether a model with side-information planes trains on the planar path (UNet.train_planes_planar) or on the fp32-storage fallback.
# Rule: True only if, with the two alternating three times in one process (tools/bench_side_planes.py: unet_2, batch 16 at 512x512, 5 planes,
# L1WS, windows of 20 steps), the slowest planar window beats the fastest fallback window.
# Measured on one MI355X (profiles/r19/README.md): planar 20.11 / 20.18 / 20.15 ms per step, fallback 32.28 / 32.35 / 32.49 ms -> True.
PLANES_PLANAR = True


def run_config(args: typing.Dict[str, typing.Any]) -> typing.Dict[str, typing.Any]:
    """The dict a run writes to its config.json: the merged arguments without the keys that are this package's own switches, and with the
    OPTIONAL_KEYS only where they are set."""
    return {k: v for k, v in args.items() if k not in ("mode", "train_mode", "take_num_images")
            and (k not in OPTIONAL_KEYS or v)}


def payload_args(args: typing.Dict[str, typing.Any]):
    """(stego method(s), alpha(s)) for the loaders: `stego_methods` / `alphas` where given, else the scalar keys; (None, None) for covers only."""
    for key in ("stego_methods", "alphas"):                              # a list that is not null overrides its scalar key; an empty one is a mistake
        if args.get(key) is not None and len(args[key]) == 0:
            raise ValueError(f"{key} is an empty list: give at least one value, or null to use the scalar key")
    if args["covers_only"]:
        return None, None
    methods = list(args["stego_methods"]) if args.get("stego_methods") is not None else args["stego_method"]
    if args.get("alphas") is not None:
        return methods, [float(a) for a in args["alphas"]]
    return methods, None if args["alpha"] is None else float(args["alpha"])


def input_planes(args: typing.Dict[str, typing.Any]) -> int:
    """Planes of the network input a run's config asks for: the image, + 1 with `parity_oracle`, + 3 with `demosaic_oracle`."""
    return 1 + int(bool(args.get("parity_oracle"))) + 3 * int(bool(args.get("demosaic_oracle")))


def train(args: typing.Dict[str, typing.Any]) -> float:
    """One run; returns the best validation loss.  `args`: DEFAULTS overridden by the caller (published config keys)."""
    args = {**DEFAULTS, **args}
    rank, world = parallel.init_from_env()
    if not torch.cuda.is_available():
        raise RuntimeError("ws_unet_amd.train needs a GPU: the train step is libwsu kernels only (no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    if args["batch_size"] % world:
        raise ValueError(f"global batch_size {args['batch_size']} is not divisible by {world} ranks")

    # run directory: <output_dir>/<stego_method>/<yymmddHHMMSS>-<job>-<run name>[_suffix]   (detector/train.py:146-159)
    # (a list of payloads has no place in the name: the `alpha_...` part is left out)
    name = time.strftime("%y%m%d%H%M%S") + "-" + str(args["SLURM_JOB_ID"]) + "-" + create_run_name(
        {**args, "alpha": None} if args["alphas"] is not None else args)
    if args["experiment_dir_suffix"]:
        name += "_" + args["experiment_dir_suffix"]
    stego, alpha = payload_args(args)
    method_dir = (args["stego_methods"][0] if args["stego_methods"] is not None else args["stego_method"]) or "dropout"
    out_dir = pathlib.Path(args["output_dir"]) / method_dir / name
    if world > 1:                                                        # every rank must agree on the timestamped name
        box = [str(out_dir)]
        torch.distributed.broadcast_object_list(box, src=0)
        out_dir = pathlib.Path(box[0])

    if args["seed"]:
        torch.manual_seed(int(args["seed"]))
    sides = (bool(args["parity_oracle"]), bool(args["demosaic_oracle"]))
    model = get_model(args["network"], in_channels=input_planes(args), out_channels=1, channel=args["channel"],
                      drop_rate=args["drop_rate"], mode=args["mode"]).to(dev)    # 0.0 still builds the (identity) dropout, like the reference
    model.side_planes = sides
    model.train_planes_planar = PLANES_PLANAR and any(sides)
    if args["train_mode"]:
        model.train_mode = args["train_mode"]
    if model.input_dropout is not None:
        model.input_dropout.seed = int(args["seed"] or 0) * world + rank
    if args["resume"]:                                                   # weights only, from another run's best model (:235-249)
        resume_dir = pathlib.Path(args["resume_dir"] or args["output_dir"]) / method_dir / args["resume"]
        if not (resume_dir / "model" / "best_model.pt.tar").exists():
            raise Exception(f"no checkpoint found at '{args['resume']}'")
        resume(model, resume_dir, dev)

    kw = dict(covers_only=bool(args["covers_only"]), rank=rank, world=world, device=dev, take_num_images=args["take_num_images"],
              simulate=bool(args["simulate_stego"]), parity_oracle=sides[0], demosaic_oracle=sides[1])
    per_rank = args["batch_size"] // world
    # augmentation: the training loader only (the validation loader is never reshuffled either: its payload draw is the same every epoch)
    tr_loader = PairLoader(args["dataset"], args["tr_csv"], stego, alpha, per_rank, shuffle=True, seed=int(args["seed"] or 0),
                           post_flip=bool(args["post_flip"]), post_rotate=bool(args["post_rotate"]), **kw)
    va_loader = PairLoader(args["dataset"], args["va_csv"], stego, alpha, per_rank, shuffle=False, **kw)

    trainer = Trainer(model, loss=args["loss"], lr=args["learning_rate"], out_dir=out_dir, config=run_config(args), patience=args["patience"])
    best = trainer.fit(tr_loader, va_loader, args["num_epochs"])
    if rank == 0:
        print(f"[train] {out_dir}: best val loss {best:.6f} after {len({e for e, _, _ in trainer.scalars})} epochs")
    return best


def parse_args(argv=None) -> typing.Dict[str, typing.Any]:
    """The command line (and the config file it names) as the dict `train` takes: the keys of DEFAULTS that were given."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", help="a published run's config.json; explicit flags override its keys")
    for key, val in DEFAULTS.items():
        flag = "--" + key
        if key in LIST_FLAGS:
            ap.add_argument(flag, type=LIST_FLAGS[key], nargs="+", default=None)
        elif isinstance(val, bool):
            ap.add_argument(flag, type=lambda s: s.lower() in ("1", "true", "yes"), default=None)
        elif isinstance(val, list):
            ap.add_argument(flag, type=int, nargs="+", default=None)
        elif isinstance(val, (int, float)) and not isinstance(val, bool):
            ap.add_argument(flag, type=type(val), default=None)
        else:
            ap.add_argument(flag, default=None)
    ns = vars(ap.parse_args(argv))
    args = {}
    cfg_path = ns.pop("config")
    if cfg_path:
        with open(cfg_path) as f:
            args.update({k: v for k, v in json.load(f).items() if k in DEFAULTS})
    args.update({k: v for k, v in ns.items() if v is not None})
    for key in ("num_epochs", "patience", "batch_size", "take_num_images"):
        if args.get(key) is not None:
            args[key] = int(args[key])
    if not args.get("dataset"):
        ap.error("--dataset is required (directory with images*/files.csv, stego*/files.csv and the split CSVs)")
    return args


def main(argv=None) -> None:
    train(parse_args(argv))


if __name__ == "__main__":
    main()
