"""A UNet on the device: what every table driver needs to run this package's UNet over uint8 planes.

  * `model_device`: where a model's planes go;
  * the range flag of the planar modes: `range_fallback` (one synchronising look, switch to 'bf16x3s') and `range_retry` (compute, look, recompute);
  * `unet_plane` (u8 -> /255 -> forward -> first output plane) and `check_unet_geometry`;
  * the WS statistics of a batch (`predict_u8_batch`), their one-copy read-back (`predict_u8_one_readback`) and the prediction-error pair
    (`predict_u8_error_batch`).
"""
from __future__ import annotations

import logging

import numpy as np
import torch

from . import ops

DEVICE = torch.device("cuda")


def model_device(model) -> torch.device:
    try:
        return next(model.parameters()).device
    except (StopIteration, AttributeError):
        return DEVICE


PLANAR_MODES = ("f16f8p", "f16f8q", "f16f4p", "f16p")         # the modes whose forward sets UNet's range flag


def range_fallback(model, collective: bool = False) -> bool:
    """One synchronising look at a planar model's range flag (UNet.range_exceeded: an activation beyond +-448 was stored since the last
    look -- the format's e4m3 residual saturates there and that value keeps only f16 accuracy, MAE ~1e-4, AT the gate; mode 'f16p': beyond
    +-65504, where the stored f16 value overflows).  If set: warn,
    switch the model to 'bf16x3s' (fp32-range storage) and return True -- the caller recomputes what it computed since the last look.
    The evaluate drivers call this once per data-set pass (one sync per pass), the per-image functions once per image (they synchronise
    on their result anyway).  `collective`: OR the flag over the ranks first (every rank of a sharded pass takes the same decision)."""
    planar = getattr(model, "mode", None) in PLANAR_MODES and hasattr(model, "range_exceeded")
    if collective:
        # EVERY rank enters the all-reduce, whatever its local state (a rank that skipped it while the others entered would hang the job
        # or pair with a later collective).  A rank whose model already left the planar modes by a look of its OWN that the other ranks
        # have not seen yet (UNet.forward_features' first-forward look, a per-image call before the pass: `_range_switched` without
        # `_range_switch_synced`) contributes 1: the others follow and everybody recomputes, in the same arithmetic.
        from . import parallel
        if not hasattr(model, "_range_flag_tensor"):
            return False
        rf = model._range_flag_tensor(model_device(model))
        unsynced = (not planar) and getattr(model, "_range_switched", False) and not getattr(model, "_range_switch_synced", False)
        hit = parallel.any_rank_flag(torch.ones_like(rf) if unsynced else rf)
        rf.zero_()
        if hit:
            model._range_switch_synced = True
        if not planar:
            return hit
    else:
        if not planar:
            return False
        hit = model.range_exceeded()
    if hit:
        if model.mode == "f16p":
            logging.warning("ws_unet_amd.evaluate: activations beyond +-65504 in mode 'f16p' (not a finite f16: the planar H format overflows); "
                            "switching this model to mode 'bf16x3s' and recomputing")
        else:
            logging.warning("ws_unet_amd.evaluate: activations beyond +-448 in mode '%s' (the planar format's e4m3 residual saturates there); "
                            "switching this model to mode 'bf16x3s' and recomputing", model.mode)
        model.mode = "bf16x3s"
        model._range_switched = True
    return hit


def range_retry(model, compute, **look):
    """compute(), ONE look at the model's range flag (range_fallback(model, **look)), and compute() once more -- now in 'bf16x3s' -- if the
    look switched the model.  WHEN a driver looks is its own (measured) decision: what it wraps is what it recomputes."""
    res = compute()
    if range_fallback(model, **look):
        res = compute()
    return res


def unet_plane(model, x_u8: torch.Tensor) -> torch.Tensor:
    """(N,H,W) uint8 device planes -> the network's first output plane for x / 255 (wsu_u8_to_unit_f32 -> forward), a contiguous (N,H,W)
    float32 tensor in [0,1]; no autograd graph.  A model trained with side-information planes (`model.side_planes`, set by get_pretrained from
    the run's config) gets them behind the image: one launch builds the whole input (ops.side_planes)."""
    parity, demosaic = getattr(model, "side_planes", (False, False))
    with torch.no_grad():
        if parity or demosaic:
            return model(ops.side_planes(x_u8, parity, demosaic))[:, 0].contiguous()
        return model(ops.u8_to_unit(x_u8)[:, None])[:, 0].contiguous()


def check_unet_geometry(hw, who: str) -> None:
    """The batched device paths feed the UNet whole planes: ValueError unless they are 512x512."""
    if tuple(hw) != (512, 512):
        raise ValueError(f"{who} works on 512x512 planes, got {hw[0]}x{hw[1]} (the reference's CenterCrop(512) would change the geometry)")


def predict_u8_batch(x_u8: torch.Tensor, model: torch.nn.Module):
    """x_u8: (N,H,W) uint8 on the model's device -> (beta_hat[N], l1[N]) fp32 device tensors.
    u8 -> /255 (wsu_u8_to_unit_f32) -> UNet forward -> WS residual statistics (wsu_ws_residual_stats)."""
    return ops.ws_residual_stats(x_u8, unet_plane(model, x_u8))


def _pack_stats(beta: torch.Tensor, l1: torch.Tensor, model):
    """(beta_hat[n], l1[n]) and, for a planar mode, the model's range flag as ONE float32 device vector (one copy brings all of it to the
    host) -> (vector, whether the flag rides along)."""
    rf = getattr(model, "_range_flag", None)
    planar = rf is not None and getattr(model, "mode", None) in PLANAR_MODES
    return torch.cat([beta.reshape(-1), l1.reshape(-1)] + ([rf.reshape(-1).view(torch.float32)] if planar else [])), planar


def _unpack_stats(v: np.ndarray, n: int, planar: bool):
    """_pack_stats' vector on the host -> (beta_hat[n], l1[n], flag set)."""
    return v[:n], v[n:2 * n], bool(planar and v[2 * n:].view(np.int32)[0] != 0)


# ---- the per-image API with ONE read-back (round 4).  The reference's call pattern is one image per call
# (src/unet/evaluate.py:48,109-139).  Round 3 synchronised three times per image (the range flag, beta_hat, l1: three blocking 4-byte copies);
# now the three words leave the device as one 12-byte copy.  Measured on one MI355X box (profiles/r04/evaluate_loop.json.log): 1 079 -> 1 256
# images/s through predict_unet_cover.  (Also measured and NOT kept: the same chain as one hipGraph replay over static buffers -- 0.62 ms per
# call against 0.57 ms for the eagerly launched kernels, whose launches overlap the GPU's work on the previous ones.)
def predict_u8_one_readback(x_u8: torch.Tensor, model: torch.nn.Module):
    """predict_u8_batch + the model's range flag, brought to the host in ONE copy: (beta_hat[N], l1[N], flag_set) as numpy / bool."""
    v, planar = _pack_stats(*predict_u8_batch(x_u8, model), model)
    return _unpack_stats(v.cpu().numpy(), x_u8.shape[0], planar)


def predict_u8_error_batch(x_u8: torch.Tensor, model: torch.nn.Module, quantile: float = 0.1):
    """x_u8: (N,H,W) uint8 on the model's device -> (mae[N], wmae[N]) fp64 device tensors.  mae is K10's l1 (same float32 residual
    x - y*255, fp64 sums in another fixed order; see tests/test_gpu_prediction_error.py), wmae its mean over the interior pixels whose
    HILL cost is at most the per-image `quantile` of the costs."""
    return ops.prediction_error(x_u8, unet_plane(model, x_u8), hat_scale=255., quantile=quantile)
