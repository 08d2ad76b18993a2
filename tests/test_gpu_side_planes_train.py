"""GPU: side-information planes (parity_oracle / demosaic_oracle) through training and evaluation: the planar training path on a 5-plane
input against the exact path, the loader on the device against its host-logic mode, and the driver end to end -- train, checkpoint,
get_pretrained, the evaluation input and the WS estimator."""
import json
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
from ws_unet_amd import evaluate, formula, ops, planes, unet_run
from ws_unet_amd.data.pairs import PairLoader
from ws_unet_amd.model import get_model

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)


def rel_l2(got, ref) -> float:
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def _model5(nsteps, mode="f16f8p"):
    m = get_model(f"unet_{nsteps}", in_channels=5, out_channels=1, channel=[0], drop_rate=None, mode=mode)
    sd = formula.formula_state_dict(nsteps, "he", in_channels=5)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def _grads(model, x, tgt):
    model.zero_grad()
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        ((model(x) - tgt) ** 2).mean().backward()
        torch.cuda.synchronize()
    finally:
        ops.set_timer(None)
    return {k: p.grad.detach().double().cpu() for k, p in model.named_parameters()}, set(timer.summary())


@pytest.mark.parametrize("ns,n,h,w", [(2, 2, 64, 96), (0, 1, 2, 4), (1, 1, 4, 8)])
def test_planar_path_takes_five_planes(ns, n, h, w):
    """train_planes_planar=True, train_mode 'f16f8p' against 'f32' under a smooth (L2) loss: every parameter gradient within relative L2 2e-3
    (the band of test_gpu_planar_train.py::test_planar_vs_fp32_storage_gradients_smooth_loss: ReLU-mask flips on rounding noise are the
    floor).  unet_0 / unet_1 at their smallest legal size, H = 2 * 2^ns, W = 4 * 2^ns."""
    assert model_default_is_off()
    model = _model5(ns)
    u8 = torch.from_numpy(np.random.default_rng(ns).integers(0, 256, (n, h, w), dtype=np.uint8)).to(DEV)
    x = ops.side_planes(u8, True, True)
    tgt = torch.rand((n, 1, h, w), generator=torch.Generator().manual_seed(4)).to(DEV)
    model.train_mode = "f32"
    exact, _ = _grads(model, x, tgt)
    model.train_mode = "f16f8p"
    fallback, used = _grads(model, x, tgt)                                        # the attribute left False: fp32 storage
    assert "conv3x3_bwd_data" in used and "conv3x3_first_pl_bwd_weight_planes" not in used
    model.train_planes_planar = True
    planar, used = _grads(model, x, tgt)
    assert "conv3x3_first_pl_bwd_weight_planes" in used and "conv3x3_pl_bwd_data" in used and "conv3x3_bwd_data" not in used
    assert tuple(planar["e11.weight"].shape) == (64, 5, 3, 3)
    worst = max(rel_l2(planar[k], exact[k]) for k in exact)
    print(f"unet_{ns} {n}x5x{h}x{w}: worst relative L2 of a parameter gradient, planar against f32: {worst:.2e}")
    for k in exact:
        assert rel_l2(planar[k], exact[k]) < 2e-3, (k, rel_l2(planar[k], exact[k]))


def model_default_is_off() -> bool:
    m = get_model("unet_0", in_channels=3, out_channels=1, channel=[0], drop_rate=None, mode="f16f8p")
    return m.train_planes_planar is False and m.side_planes == (False, False)


def _golden_dataset(root):
    (root / "images").mkdir(parents=True)
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    return root


def test_loader_on_the_device_equals_host_logic(tmp_path):
    """Both oracles, flips and rotations on: the file route and simulate=True (a bare data set, HILLR twins made on the device) against the
    host-logic loader over the twins the simulator wrote; covers and alphas are those of the same loader without oracles."""
    from ws_unet_amd import embed
    data, bare = _golden_dataset(tmp_path / "data"), _golden_dataset(tmp_path / "bare")
    kw = dict(batch_size=4, seed=11, post_flip=True, post_rotate=True)
    embed.write_dataset(data, "HILLR", [0.4])
    host = PairLoader(data, None, "HILLR", 0.4, parity_oracle=True, demosaic_oracle=True, **kw)
    plain = PairLoader(data, None, "HILLR", 0.4, device=torch.device(DEV), **kw)
    loaders = {"files": PairLoader(data, None, "HILLR", 0.4, device=torch.device(DEV), parity_oracle=True, demosaic_oracle=True, **kw),
               "simulate": PairLoader(bare, None, "HILLR", 0.4, simulate=True, device=torch.device(DEV), parity_oracle=True,
                                      demosaic_oracle=True, **kw)}
    assert host.aug_ops().max() >= 4
    want, base = list(host), list(plain)
    assert len(want) == len(base) == 2
    for name, loader in loaders.items():
        got = list(loader)
        assert len(got) == 2, name
        for (x, (c, a)), (xh, (ch, ah)), (x0, (c0, a0)) in zip(got, want, base):
            assert x.is_cuda and x.shape == (4, 5, 512, 512) and x.dtype == torch.float32 and tuple(xh.shape) == (4, 5, 512, 512)
            assert xh.dtype == torch.uint8
            hx = xh.numpy()
            assert np.array_equal(x[:, 0].cpu().numpy(), hx[:, 0].astype(np.float32) / np.float32(255)), name
            assert np.array_equal(x[:, 1:].cpu().numpy(), hx[:, 1:].astype(np.float32)), name
            assert set(np.unique(hx[:, 1:])) == {0, 1}
            assert torch.equal(c, c0) and torch.equal(a, a0) and torch.equal(x[:, :1], x0), name
            assert np.array_equal(c.cpu().numpy()[:, 0], ch.numpy().astype(np.float32) / np.float32(255)) and torch.equal(a.cpu(), ah)


def test_driver_trains_checkpoints_and_evaluates_with_both_oracles(tmp_path):
    from ws_unet_amd import train as train_mod
    from ws_unet_amd import filters
    from ws_unet_amd.imread import imread4_u8
    from ws_unet_amd.ws import estimate
    data = _golden_dataset(tmp_path / "data")
    rows = "name,height,width,stego_method,alpha\n" + "".join(f"images/{k}.png,512,512,,\n" for k in COVERS)
    for name in ("split_tr.csv", "split_va.csv"):
        (data / name).write_text(rows)
    cfg = {"dataset": str(data), "output_dir": str(tmp_path / "runs"), "network": "unet_1", "stego_method": "LSBR", "alpha": "0.400",
           "simulate_stego": True, "parity_oracle": True, "demosaic_oracle": True, "post_flip": True, "post_rotate": True, "loss": "l1ws",
           "batch_size": 2, "num_epochs": 1, "take_num_images": 4, "learning_rate": 1e-3, "drop_rate": 0.0, "seed": 7, "SLURM_JOB_ID": "44"}
    best = train_mod.train(cfg)
    assert np.isfinite(best)
    runs = list((tmp_path / "runs" / "LSBR").iterdir())
    assert len(runs) == 1 and "oracle_" in runs[0].name and "parity" not in runs[0].name
    saved = json.loads((runs[0] / "config.json").read_text())
    assert saved["parity_oracle"] is True and saved["demosaic_oracle"] is True
    ckpt = torch.load(runs[0] / "model" / "best_model.pt.tar", map_location="cpu", weights_only=True)
    assert tuple(ckpt["state_dict"]["e11.weight"].shape) == (64, 5, 3, 3)
    model = evaluate.get_pretrained(tmp_path / "runs" / "LSBR", (3,), model_name=runs[0].name)
    assert model.side_planes == (True, True) and model.e11.in_channels == 5
    files = [str(data / "images" / f"{k}.png") for k in COVERS[:3]]
    x_u8 = planes.load_planes_u8(files).to(DEV)
    with torch.no_grad():
        want = model(ops.side_planes(x_u8, True, True))[:, 0]
    assert torch.equal(unet_run.unet_plane(model, x_u8), want)
    est = estimate.UNetEstimator(model)
    batch = estimate.attack_batch(files, [{} for _ in files], channels=(3,), pixel_estimator=est)
    host_kw = dict(imread=imread4_u8, process_image=filters.get_processor_2d((3,)))
    single = [estimate.attack(f, (3,), est, **host_kw) for f in files]
    betas = [r["beta_hat"] for r in batch]
    assert np.all(np.isfinite(betas)) and betas == [r["beta_hat"] for r in single]
    with pytest.raises(NotImplementedError, match="parity of that difference image"):
        estimate.attack(files[0], (3,), est, correct_bias=True, **host_kw)
