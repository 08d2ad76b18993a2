"""CPU: the side-information planes (parity_oracle / demosaic_oracle) in the loader's host-logic mode and in the training driver's
configuration handling."""
import json
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
from ws_unet_amd.data import get_timm_transform
from ws_unet_amd.data.pairs import PairLoader, apply_op, side_planes_u8
from ws_unet_amd.imread import imread4_u8

COVERS = (6, 7, 8, 9, 10)


def _dataset(root):
    (root / "images").mkdir(parents=True)
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    sd = root / "stego_LSBR_alpha_0.1"
    sd.mkdir()
    for k in COVERS:
        shutil.copy(GOLDEN / f"stego_LSBR_0.1_{k}.png", sd / f"{k}.png")
    (sd / "files.csv").write_text("name,height,width,stego_method,alpha\n" + "".join(f"{sd.name}/{k}.png,512,512,LSBR,0.1\n" for k in COVERS))
    return root


def test_host_logic_batches_equal_the_reference_transform(tmp_path):
    data = _dataset(tmp_path)
    kw = dict(batch_size=4, seed=5, post_flip=True, post_rotate=True)
    loader = PairLoader(data, None, "LSBR", 0.1, parity_oracle=True, demosaic_oracle=True, **kw)
    plain = PairLoader(data, None, "LSBR", 0.1, **kw)
    transform = get_timm_transform(mean=None, std=None, grayscale=True, parity_oracle=True, demosaic_oracle=True)
    codes, order = loader.aug_ops(), loader.pair_order()
    assert len(set(codes.tolist())) > 1 and codes.max() >= 4
    batches, base = list(loader), list(plain)
    assert len(batches) == len(order) == 2
    for (x, (c, a)), (x0, (c0, a0)), pairs in zip(batches, base, order):
        assert tuple(x.shape) == (4, 5, 512, 512) and x.dtype.is_floating_point is False and tuple(c.shape) == (4, 512, 512)
        assert np.array_equal(x[:, 0].numpy(), x0.numpy()) and np.array_equal(c.numpy(), c0.numpy()) and a.tolist() == a0.tolist()
        for k, f in enumerate(f for p in pairs for f in (loader.covers[p], loader.stegos[p])):    # cover, then its twin: own pixels, own parity
            want = apply_op(transform(imread4_u8(data / f)).numpy(), codes[pairs[k // 2]])
            got = x[k].numpy()
            assert np.array_equal(got[0].astype(np.float32) / np.float32(255), want[0])
            assert np.array_equal(got[1:].astype(np.float32), want[1:])


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (4, 4), (5, 5), (2, 3), (3, 5), (6, 8)])
def test_plane_rule_in_source_coordinates(h, w):
    """The rule of include/wsu.h evaluated at the source coordinate of every output pixel equals "append the planes, then transform";
    and round((v / 255) * 255) & 1 == v & 1 in fp32 for all 256 values (the reference's ParityOracle sees v / 255)."""
    u8 = np.random.default_rng(h * 16 + w).integers(0, 256, (h, w), dtype=np.uint8)
    for op in range(8 if h == w else 4):
        got = apply_op(side_planes_u8(u8, True, True), op)
        oh, ow = got.shape[1:]
        for i in range(oh):
            for j in range(ow):
                r, c = (j, i) if op & 4 else (i, j)
                r = h - 1 - r if op & 2 else r
                c = w - 1 - c if op & 1 else c
                v = int(u8[r, c])
                rule = [v, v & 1, int(r % 2 == 0 and c % 2 == 0), int((r + c) % 2 == 1), int(r % 2 == 1 and c % 2 == 1)]
                assert got[:, i, j].tolist() == rule, (op, i, j)
    v = np.arange(256, dtype=np.float32)
    assert np.array_equal(np.round((v / np.float32(255)) * np.float32(255)).astype(np.int32) & 1, np.arange(256) & 1)


def test_driver_configuration(tmp_path, monkeypatch):
    from ws_unet_amd import train as train_mod
    assert train_mod.DEFAULTS["parity_oracle"] is False and "parity_oracle" in train_mod.OPTIONAL_KEYS
    plain = train_mod.run_config({**train_mod.DEFAULTS, "dataset": "d", "stego_method": "LSBR", "alpha": "0.4"})
    assert "parity_oracle" not in plain and plain["demosaic_oracle"] is False          # the config of such a run is what it always was
    assert train_mod.run_config({**train_mod.DEFAULTS, "parity_oracle": True})["parity_oracle"] is True
    f = tmp_path / "config.json"
    f.write_text(json.dumps({"network": "unet_2", "stego_method": "LSBR", "alpha": "0.400", "parity_oracle": True, "demosaic_oracle": True,
                             "num_workers": 8}))
    args = train_mod.parse_args(["--config", str(f), "--dataset", str(tmp_path)])
    assert args["parity_oracle"] is True and args["demosaic_oracle"] is True and "num_workers" not in args
    seen = {}
    monkeypatch.setattr(train_mod, "train", lambda a: seen.update(a) or 0.0)
    train_mod.main(["--dataset", str(tmp_path), "--parity_oracle", "true"])
    assert seen["parity_oracle"] is True and "demosaic_oracle" not in seen
    want = {(False, False): 1, (True, False): 2, (False, True): 4, (True, True): 5}
    for (parity, demosaic), planes in want.items():
        assert train_mod.input_planes({"parity_oracle": parity, "demosaic_oracle": demosaic}) == planes
    assert train_mod.input_planes({}) == 1
    # run name as the reference's create_run_name: a part for the demosaic oracle, none for parity
    from ws_unet_amd.trainer import create_run_name
    base = {**train_mod.DEFAULTS, "alpha": "0.4"}
    assert create_run_name({**base, "parity_oracle": True}) == create_run_name(base)
    assert "oracle_" in create_run_name({**base, "demosaic_oracle": True}) and "oracle_" not in create_run_name(base)
