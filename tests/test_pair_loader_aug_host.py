"""CPU: the pair loader's D4 augmentation and mixed payloads in host-logic mode (device=None: uint8 planes, numpy transforms) on PNGs
written to tmp_path, and the training driver's four new keys."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

from ws_unet_amd import formula
from ws_unet_amd.data.pairs import FLIP_ROT_OP, PairLoader, apply_op

ALPHAS = (0.4, 0.2)


def _dataset(root, h=64, w=64, n=6, alphas=(0.4,), missing=()):
    """n covers and, per alpha, an LSBR folder of twins; `missing` = (alpha, cover) twins that are left out."""
    (root / "images").mkdir(parents=True)
    u8 = formula.synthetic_images(n, h, w, seed=31)
    for i in range(n):
        Image.fromarray(u8[i]).save(root / "images" / f"{i}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{i}.png,{h},{w}\n" for i in range(n)))
    st = {}
    for a in alphas:
        sd = root / f"stego_LSBR_alpha_{a}"
        sd.mkdir()
        ids = [i for i in range(n) if (a, i) not in missing]
        for i in ids:
            st[a, i] = formula.lsbr_embed(u8[i], a, seed=100 * i + int(10 * a))
            Image.fromarray(st[a, i]).save(sd / f"{i}.png")
        (sd / "files.csv").write_text("name,height,width,stego_method,alpha\n" + "".join(f"{sd.name}/{i}.png,{h},{w},LSBR,{a}\n" for i in ids))
    return u8, st


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = tmp_path_factory.mktemp("pairs64")
    return (root,) + _dataset(root)


def _batches(loader):
    return [(x.numpy(), c.numpy(), a.numpy()) for x, (c, a) in loader]


def test_flip_rot_table_and_op_decoder_against_numpy():
    ramp = np.arange(16).reshape(4, 4)
    assert FLIP_ROT_OP.shape == (16,) and FLIP_ROT_OP.dtype == np.uint8
    for k in range(4):
        for vflip in (0, 1):
            for hflip in (0, 1):
                y = ramp[:, ::-1] if hflip else ramp
                y = y[::-1, :] if vflip else y
                np.testing.assert_array_equal(apply_op(ramp, FLIP_ROT_OP[hflip + 2 * vflip + 4 * k]), np.rot90(y, k), err_msg=f"{hflip} {vflip} {k}")
    assert FLIP_ROT_OP.tolist() == [0, 1, 2, 3, 5, 4, 7, 6, 3, 2, 1, 0, 6, 7, 4, 5]
    assert [int(FLIP_ROT_OP[4 * k]) for k in range(4)] == [0, 5, 3, 6]                       # rot90(x, k) alone
    assert len({apply_op(ramp, o).tobytes() for o in range(8)}) == 8
    # the decoder against the (r, c) formula of include/wsu.h, on a non-square ramp
    x = np.arange(12).reshape(3, 4)
    h, w = x.shape
    for o in range(8):
        y = apply_op(x, o)
        assert y.shape == ((w, h) if o & 4 else (h, w))
        for i in range(y.shape[0]):
            for j in range(y.shape[1]):
                r, c = (j, i) if o & 4 else (i, j)
                r = h - 1 - r if o & 2 else r
                c = w - 1 - c if o & 1 else c
                assert y[i, j] == x[r, c], (o, i, j)
    with pytest.raises(ValueError):
        apply_op(x, 8)


def test_augmented_batches_are_the_plain_batches_transformed(data):
    root = data[0]
    kw = dict(batch_size=4, seed=7)
    plain = PairLoader(root, None, "LSBR", 0.4, **kw)
    aug = PairLoader(root, None, "LSBR", 0.4, post_flip=True, post_rotate=True, **kw)
    ops = aug.aug_ops()
    assert ops.shape == (6,) and ops.max() <= 7 and len(set(ops.tolist())) > 1
    pairs = plain.pair_order()
    assert np.array_equal(pairs, aug.pair_order())
    for (x, c, a), (xp, cp, ap), batch_pairs in zip(_batches(aug), _batches(plain), pairs):
        assert x.dtype == np.uint8 and np.array_equal(a, ap)
        for s in range(4):
            o = ops[batch_pairs[s // 2]]                                             # cover and stego sample of a pair share the op
            np.testing.assert_array_equal(x[s], apply_op(xp[s], o))
            np.testing.assert_array_equal(c[s], apply_op(cp[s], o))                  # ... and so does the target
    # same seed and epoch: same ops; the next epoch draws again
    again = PairLoader(root, None, "LSBR", 0.4, post_flip=True, post_rotate=True, **kw)
    assert np.array_equal(again.aug_ops(), ops) and np.array_equal(aug.aug_ops(0), ops)
    aug.reshuffle()
    assert not np.array_equal(aug.aug_ops(), ops) and np.array_equal(aug.aug_ops(), again.aug_ops(1))
    # flips alone stay among ops 0..3, rotations alone among rot90's codes
    assert set(PairLoader(root, None, "LSBR", 0.4, post_flip=True, **kw).aug_ops(3).tolist()) <= {0, 1, 2, 3}
    assert set(PairLoader(root, None, "LSBR", 0.4, post_rotate=True, **kw).aug_ops(3).tolist()) <= {0, 5, 3, 6}


def test_ranks_split_the_augmented_epoch(data):
    root = data[0]
    kw = dict(seed=5, post_flip=True, post_rotate=True)
    full = _batches(PairLoader(root, None, "LSBR", 0.4, batch_size=4, **kw))
    r0 = _batches(PairLoader(root, None, "LSBR", 0.4, batch_size=2, rank=0, world=2, **kw))
    r1 = _batches(PairLoader(root, None, "LSBR", 0.4, batch_size=2, rank=1, world=2, **kw))
    assert len(full) == len(r0) == len(r1) == 3
    for f, a, b in zip(full, r0, r1):
        for k in range(3):                                                           # pairs r, r + world, ...: rank 0's pair, then rank 1's
            np.testing.assert_array_equal(f[k], np.concatenate([a[k], b[k]]))


def test_flags_off_give_todays_batches(data):
    root, u8, st = data
    old = _batches(PairLoader(root, None, "LSBR", 0.4, batch_size=4, seed=2))
    new = PairLoader(root, None, "LSBR", 0.4, batch_size=4, seed=2, post_flip=False, post_rotate=False)
    assert not new.aug_ops().any() and new.payload_plan() == [("LSBR", 0.4)] * 6
    pairs = new.pair_order()
    for (x, c, a), (xo, co, ao), bp in zip(_batches(new), old, pairs):
        assert np.array_equal(x, xo) and np.array_equal(c, co) and np.array_equal(a, ao)
        np.testing.assert_array_equal(x, np.stack([u8[bp[0]], st[0.4, bp[0]], u8[bp[1]], st[0.4, bp[1]]]))     # fabrika's order = 0..5 here
        np.testing.assert_array_equal(c, np.stack([u8[bp[0]], u8[bp[0]], u8[bp[1]], u8[bp[1]]]))
        assert a.tolist() == pytest.approx([0.0, 0.4, 0.0, 0.4])
    # a one-element list is the scalar route
    one = PairLoader(root, None, ["LSBR"], [0.4], batch_size=4, seed=2)
    assert one.combos is None and all(np.array_equal(p, q) for b, bo in zip(_batches(one), old) for p, q in zip(b, bo))


def test_rotation_needs_square_images(tmp_path):
    u8, st = _dataset(tmp_path, h=48, w=64, n=4)
    with pytest.raises(ValueError, match="square"):
        next(iter(PairLoader(tmp_path, None, "LSBR", 0.4, batch_size=4, post_rotate=True)))
    ld = PairLoader(tmp_path, None, "LSBR", 0.4, batch_size=4, shuffle=False, seed=1, post_flip=True)
    ops = ld.aug_ops()
    assert set(ops.tolist()) <= {0, 1, 2, 3}
    (x, c, a), = _batches(ld)[:1]
    assert x.shape == (4, 48, 64)
    for s in range(4):
        np.testing.assert_array_equal(x[s], apply_op(st[0.4, s // 2] if s % 2 else u8[s // 2], ops[s // 2]))
        np.testing.assert_array_equal(c[s], apply_op(u8[s // 2], ops[s // 2]))


def test_payload_lists_draw_one_twin_per_pair(tmp_path):
    u8, st = _dataset(tmp_path, n=7, alphas=ALPHAS, missing={(0.2, 3)})
    kw = dict(batch_size=4, seed=9)
    ld = PairLoader(tmp_path, None, "LSBR", list(ALPHAS), **kw)
    assert ld.combos == [("LSBR", 0.4), ("LSBR", 0.2)]
    assert ld.covers == [f"images/{i}.png" for i in (0, 1, 2, 4, 5, 6)]                      # cover 3 lacks its 0.2 twin: dropped
    ids = [0, 1, 2, 4, 5, 6]
    plan = ld.payload_plan()
    assert len(plan) == 6 and set(plan) <= set(ld.combos)
    assert len({a for e in range(4) for _, a in ld.payload_plan(e)}) == 2                    # both payloads are drawn
    for (x, c, a), bp in zip(_batches(ld), ld.pair_order()):
        for k, p in enumerate(bp):
            alpha = plan[p][1]
            np.testing.assert_array_equal(x[2 * k], u8[ids[p]])
            np.testing.assert_array_equal(x[2 * k + 1], st[alpha, ids[p]])                  # the file of the drawn combination, byte for byte
            np.testing.assert_array_equal(c[2 * k + 1], u8[ids[p]])
            assert a[2 * k] == 0.0 and a[2 * k + 1] == np.float32(alpha)
    r0 = PairLoader(tmp_path, None, "LSBR", list(ALPHAS), rank=0, world=2, **kw)
    r1 = PairLoader(tmp_path, None, "LSBR", list(ALPHAS), rank=1, world=2, **kw)
    assert r0.payload_plan() == r1.payload_plan() == plan
    ld.reshuffle()
    assert ld.payload_plan() != plan or ld.payload_plan(2) != plan
    with pytest.raises(ValueError, match="no cover"):
        PairLoader(tmp_path, None, "LSBR", [0.4, 0.1], **kw)                                 # no 0.1 folder: no pair has every combination


def test_train_driver_takes_the_four_new_keys(tmp_path, monkeypatch):
    from ws_unet_amd import train as train_mod
    seen = {}
    monkeypatch.setattr(train_mod, "train", lambda args: seen.update(args) or 0.0)
    cfg = {"network": "unet_2", "alpha": "0.400", "stego_method": "LSBR", "post_flip": True, "post_rotate": True, "alphas": [0.4, 0.2],
           "stego_methods": ["LSBR", "HILLR"], "num_workers": 8}
    f = tmp_path / "config.json"
    f.write_text(json.dumps(cfg))
    train_mod.main(["--config", str(f), "--dataset", str(tmp_path)])
    assert seen["post_flip"] is True and seen["post_rotate"] is True and seen["alphas"] == [0.4, 0.2] and seen["stego_methods"] == ["LSBR", "HILLR"]
    seen.clear()
    train_mod.main(["--dataset", str(tmp_path), "--post_flip", "true", "--post_rotate", "true", "--alphas", ".4", ".2", ".1",
                    "--stego_methods", "LSBR", "HILLR"])
    assert seen["post_flip"] is True and seen["post_rotate"] is True and seen["alphas"] == [0.4, 0.2, 0.1] and seen["stego_methods"] == ["LSBR", "HILLR"]
    merged = {**train_mod.DEFAULTS, **seen}
    assert train_mod.payload_args(merged) == (["LSBR", "HILLR"], [0.4, 0.2, 0.1])
    written = train_mod.run_config(merged)
    assert written["post_flip"] is True and written["post_rotate"] is True and written["alphas"] == [0.4, 0.2, 0.1]
    assert written["stego_methods"] == ["LSBR", "HILLR"] and "mode" not in written and "simulate_stego" not in written
    # a run that sets none of them writes the config it always wrote
    plain = train_mod.run_config({**train_mod.DEFAULTS, "dataset": "d", "stego_method": "LSBR", "alpha": "0.4"})
    assert not {"post_flip", "post_rotate", "alphas", "stego_methods", "simulate_stego"} & set(plain)
    assert train_mod.payload_args({**train_mod.DEFAULTS, "stego_method": "LSBR", "alpha": "0.4"}) == ("LSBR", 0.4)
    assert train_mod.payload_args({**train_mod.DEFAULTS, "stego_method": "LSBR", "alpha": "0.4", "covers_only": True}) == (None, None)
    for key in ("stego_methods", "alphas"):                                                   # not null overrides; an empty list is refused, for both keys alike
        with pytest.raises(ValueError, match=key):
            train_mod.payload_args({**train_mod.DEFAULTS, "stego_method": "LSBR", "alpha": "0.4", key: []})
    assert train_mod.payload_args({**train_mod.DEFAULTS, "stego_method": "LSBR", "alpha": "0.4", "stego_methods": ["HILLR"]}) == (["HILLR"], 0.4)
    # the run name leaves the alpha part out when a list is given
    from ws_unet_amd.trainer import create_run_name
    assert "alpha_" in create_run_name({**train_mod.DEFAULTS, "alpha": "0.4"})
    assert "alpha_" not in create_run_name({**train_mod.DEFAULTS, "alpha": None})
