"""GPU: wsu_pair_batch_f32 (gather + D4 transform + u8 -> unit fp32 in one launch) against numpy, exactly, and the pair loader's
augmentation / mixed payloads on the device against its host-logic mode."""
import json
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
from ws_unet_amd import _lib, embed, formula, ops
from ws_unet_amd.data.pairs import PairLoader
from ws_unet_amd.imread import imread4_u8

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)


def _planes(files, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (files, h, w), dtype=np.uint8)


def apply_op(x, op):
    """The op table of include/wsu.h restated in numpy: bit 0 mirrors the columns, bit 1 the rows, bit 2 transposes last."""
    x = x[:, ::-1] if op & 1 else x
    x = x[::-1, :] if op & 2 else x
    return x.T if op & 4 else x


def _expect(planes, idx, op):
    """np.float32(D(op)(plane)) / np.float32(255), per sample"""
    return np.stack([apply_op(planes[i], o).astype(np.float32) / np.float32(255) for i, o in zip(idx, op)])[:, None]


def _check(planes, idx_in, idx_cov, op):
    x, c = ops.pair_batch(torch.from_numpy(planes).to(DEV), idx_in, idx_cov, op)
    torch.cuda.synchronize()
    n, (h, w) = len(op), planes.shape[1:]
    assert x.shape == c.shape == (n, 1, h, w) and x.dtype == c.dtype == torch.float32
    want_x, want_c = _expect(planes, idx_in, op), _expect(planes, idx_cov, op)
    for s in range(n):                                                          # `==` on fp32, sample by sample for a readable failure
        assert np.array_equal(x[s].cpu().numpy(), want_x[s]), f"inputs[{s}]: plane {idx_in[s]} op {op[s]} at {h}x{w}"
        assert np.array_equal(c[s].cpu().numpy(), want_c[s]), f"covers[{s}]: plane {idx_cov[s]} op {op[s]} at {h}x{w}"


def test_every_op_with_repeated_and_crossed_indices():
    planes = _planes(3, 64, 64, 1)
    op = list(range(8)) * 2
    idx_in = [0, 1, 2, 0, 1, 2, 0, 1, 2, 2, 1, 0, 2, 1, 0, 1]
    idx_cov = [0, 0, 2, 1, 1, 0, 0, 2, 1, 2, 0, 0, 1, 1, 2, 1]                 # equal (cover samples) and different, in every op
    assert {(o, a == b) for o, a, b in zip(op, idx_in, idx_cov)} == {(o, e) for o in range(8) for e in (True, False)}
    _check(planes, idx_in, idx_cov, op)
    # op 0 is today's assembly, bit for bit: wsu_u8_to_unit_f32, then two gathers
    d = torch.from_numpy(planes).to(DEV)
    unit = ops.u8_to_unit(d)[:, None]
    x, c = ops.pair_batch(d, idx_in, idx_cov, [0] * 16)
    assert torch.equal(x, unit[torch.tensor(idx_in, device=DEV)]) and torch.equal(c, unit[torch.tensor(idx_cov, device=DEV)])


@pytest.mark.parametrize("size", [1, 2, 66, 68, 129])
def test_square_edges_all_ops(size):
    """1, 2: less than one word; 66 / 129: partial tiles in both directions, w % 4 = 2 / 1, rows start unaligned (the byte-wise kernel);
    68: partial tiles in the 4-byte / 16-byte kernel."""
    planes = _planes(2, size, size, size)
    _check(planes, [0, 1] * 4, [0, 0, 1, 1, 1, 1, 0, 0], list(range(8)))


@pytest.mark.parametrize("h,w", [(5, 7), (130, 34), (6, 72)])
def test_non_square_planes_take_the_mirrors(h, w):
    """w not a multiple of 4 (5x7, 130x34: three row tiles) and a word-aligned non-square shape with a partial column tile (6x72)"""
    planes = _planes(2, h, w, h * w)
    _check(planes, [0, 1, 1, 0], [0, 0, 1, 1], [0, 1, 2, 3])


def test_workload_plane_size_once():
    planes = _planes(2, 512, 512, 512)
    _check(planes, [0, 1, 0, 1, 1, 0, 1, 0], [0, 0, 0, 0, 1, 1, 1, 1], list(range(8)))


def test_empty_batch_and_argument_errors():
    d = torch.from_numpy(_planes(3, 5, 7, 0)).to(DEV)
    x, c = ops.pair_batch(d, [], [], [])
    assert x.shape == c.shape == (0, 1, 5, 7) and x.dtype == torch.float32 and x.is_cuda
    for bad in (([3], [0], [0]), ([0], [-1], [0]), ([0], [0], [8]), ([0], [0], [4])):       # index `files`, index -1, op 8, op 4 on 5x7
        with pytest.raises(ValueError):
            ops.pair_batch(d, *bad)
    sq = torch.from_numpy(_planes(1, 4, 4, 0)).to(DEV)
    assert ops.pair_batch(sq, [0], [0], [4])[0].shape == (1, 1, 4, 4)                       # ... and fine on square planes
    lib = _lib.load()
    assert lib.wsu_pair_batch_f32(None, 1, 4, 4, None, None, None, 1, 1, None, None, None) == -1 and b"null" in lib.wsu_last_error()
    p = d.data_ptr()
    assert lib.wsu_pair_batch_f32(p, 3, 5, 7, p, p, p, 1, 1, p, p, None) == -1 and b"square" in lib.wsu_last_error()
    assert lib.wsu_pair_batch_f32(p, 3, 0, 7, p, p, p, 1, 0, p, p, None) == -1 and b"h=0" in lib.wsu_last_error()
    assert lib.wsu_pair_batch_f32(p, 3, 5, 7, p, p, p, -1, 0, p, p, None) == -1
    assert lib.wsu_pair_batch_f32(p, 3, 5, 7, p, p, p, 0, 0, p, p, None) == 0               # n == 0: nothing to do


def test_out_of_range_samples_write_nothing():
    """The raw entry point with what the wrapper refuses: such a sample's outputs keep their bytes, its neighbours are assembled."""
    planes = _planes(2, 8, 8, 3)
    d = torch.from_numpy(planes).to(DEV)
    n = 5
    idx_in = torch.tensor([0, 2, 1, -1, 1], dtype=torch.int32, device=DEV)                  # sample 1: index `files`; sample 3: -1
    idx_cov = torch.tensor([0, 0, 1, 0, 0], dtype=torch.int32, device=DEV)
    op = torch.tensor([1, 0, 9, 0, 6], dtype=torch.uint8, device=DEV)                       # sample 2: op 9
    x = torch.full((n, 1, 8, 8), -1.0, device=DEV)
    c = torch.full((n, 1, 8, 8), -1.0, device=DEV)
    rc = _lib.load().wsu_pair_batch_f32(d.data_ptr(), 2, 8, 8, idx_in.data_ptr(), idx_cov.data_ptr(), op.data_ptr(), n, 1, x.data_ptr(),
                                       c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for s in (1, 2, 3):
        assert (x[s] == -1).all() and (c[s] == -1).all()
    assert np.array_equal(x[0].cpu().numpy(), _expect(planes, [0], [1])[0]) and np.array_equal(c[4].cpu().numpy(), _expect(planes, [0], [6])[0])
    assert np.array_equal(x[4].cpu().numpy(), _expect(planes, [1], [6])[0])
    # allow_transpose = 0: ops 4..7 are not admitted either
    x.fill_(-1.0)
    op4 = torch.tensor([4, 0, 0, 0, 0], dtype=torch.uint8, device=DEV)
    ok = torch.zeros(n, dtype=torch.int32, device=DEV)
    assert _lib.load().wsu_pair_batch_f32(d.data_ptr(), 2, 8, 8, ok.data_ptr(), ok.data_ptr(), op4.data_ptr(), n, 0, x.data_ptr(), c.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert (x[0] == -1).all() and np.array_equal(x[1].cpu().numpy(), _expect(planes, [0], [0])[0])


# ---- the loader on the device ------------------------------------------------------------------------------------------------------

METHODS, ALPHAS = ["LSBR", "HILLR"], [0.4, 0.1]


def _unit(u8: torch.Tensor) -> np.ndarray:
    return u8.numpy().astype(np.float32)[:, None] / np.float32(255)


def test_loader_on_the_device_equals_host_logic(tmp_path):
    """Five golden covers, LSBR / HILLR x 0.4 / 0.1, flips and rotations on: the file route and simulate=True on the device against the
    host-logic loader over the files the simulators wrote."""
    data, bare = tmp_path / "data", tmp_path / "bare"
    for root in (data, bare):
        (root / "images").mkdir(parents=True)
        for k in COVERS:
            shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
        (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    kw = dict(batch_size=4, seed=11, post_flip=True, post_rotate=True)
    sim = PairLoader(bare, None, METHODS, ALPHAS, simulate=True, device=torch.device(DEV), **kw)
    for m in METHODS:
        embed.write_dataset(data, m, ALPHAS, stream=sim.lsbr_stream(0))
    host = PairLoader(data, None, METHODS, ALPHAS, **kw)
    files = PairLoader(data, None, METHODS, ALPHAS, device=torch.device(DEV), **kw)
    assert host.covers == sim.covers == files.covers and host.payload_plan() == sim.payload_plan() == files.payload_plan()
    assert host.combos == [("LSBR", 0.4), ("LSBR", 0.1), ("HILLR", 0.4), ("HILLR", 0.1)]
    plan, aug, order = host.payload_plan(), host.aug_ops(), host.pair_order()
    assert len(set(plan)) > 1 and aug.max() >= 4
    want = list(host)
    assert len(want) == 2
    covers_u8 = {c: imread4_u8(data / c)[..., 3] for c in host.covers}
    for name, loader in (("files", files), ("simulate", sim)):
        got = list(loader)
        assert len(got) == 2, name
        for (x, (c, a)), (xh, (ch, ah)), pairs in zip(got, want, order):
            assert x.is_cuda and x.shape == (4, 1, 512, 512) and x.dtype == torch.float32
            assert np.array_equal(x.cpu().numpy(), _unit(xh)), name
            assert np.array_equal(c.cpu().numpy(), _unit(ch)), name
            assert torch.equal(a.cpu(), ah) and a.cpu().tolist() == pytest.approx([v for p in pairs for v in (0.0, plan[p][1])])
            if name == "simulate":                                               # the HILLR samples: D(op) of embed.simulate at the drawn alpha
                for k, p in enumerate(pairs):
                    if plan[p][0] != "HILLR":
                        continue
                    cover = torch.from_numpy(covers_u8[host.covers[p]]).to(DEV)[None]
                    twin = embed.simulate(cover, "HILLR", plan[p][1])[0][0].cpu().numpy()
                    assert np.array_equal(x[2 * k + 1, 0].cpu().numpy(), apply_op(twin, aug[p]).astype(np.float32) / np.float32(255))
    assert any(plan[p][0] == "HILLR" for p in order.ravel())


def test_driver_trains_with_flags_and_an_alpha_list(tmp_path):
    from PIL import Image
    from ws_unet_amd import train as train_mod
    data = tmp_path / "data"
    (data / "images").mkdir(parents=True)
    u8 = formula.synthetic_images(6, 64, 64, seed=77)
    for i in range(6):
        Image.fromarray(u8[i]).save(data / "images" / f"{i}.png")
    rows = "".join(f"images/{i}.png,64,64,,\n" for i in range(6))
    for a in (0.4, 0.2):
        sd = data / f"stego_LSBR_alpha_{a}"
        sd.mkdir()
        for i in range(6):
            Image.fromarray(formula.lsbr_embed(u8[i], a, seed=10 * i + int(10 * a))).save(sd / f"{i}.png")
        rows += "".join(f"{sd.name}/{i}.png,64,64,LSBR,{a}\n" for i in range(6))
    for name in ("split_tr.csv", "split_va.csv"):
        (data / name).write_text("name,height,width,stego_method,alpha\n" + rows)
    cfg = {"dataset": str(data), "output_dir": str(tmp_path / "runs"), "network": "unet_1", "stego_methods": ["LSBR"], "alphas": [0.4, 0.2],
           "post_flip": True, "post_rotate": True, "loss": "l1ws", "batch_size": 4, "num_epochs": 2, "patience": 5, "learning_rate": 1e-3,
           "drop_rate": 0.0, "seed": 7, "SLURM_JOB_ID": "43", "mode": "f32"}
    best = train_mod.train(cfg)
    assert np.isfinite(best)
    runs = list((tmp_path / "runs" / "LSBR").iterdir())
    assert len(runs) == 1 and "alpha_" not in runs[0].name
    saved = json.loads((runs[0] / "config.json").read_text())
    assert saved["post_flip"] is True and saved["post_rotate"] is True and saved["alphas"] == [0.4, 0.2] and saved["stego_methods"] == ["LSBR"]
    scalars = (runs[0] / "log" / "scalars.csv").read_text().splitlines()
    losses = [float(ln.split(",")[2]) for ln in scalars if ",train/loss," in ln]
    assert len(losses) == 2 and all(np.isfinite(losses))
