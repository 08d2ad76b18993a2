"""GPU: the ternary two-layer syndrome-trellis embedder (K45-K47 over K43 / K44, ops.stc_layer_high / _low / _compose, ws_unet_amd.stc_ml)
against the numpy restatement (stc_ml_np) on its fixture grid.  The integer planes, the low layer's costs, the stego, the counts and the
layer lengths bit for bit; the high layer's costs and the two float sums to the roundings of the library functions and of a reordered
sum.  The restatement takes the device's multiplier, and each Viterbi pass is compared by giving stc_np.viterbi the DEVICE's cost plane,
so that one unit in the last place of exp or log1p cannot flip a tie.  Then the round trip, batch independence, stego over cover, the
strict errors and the drivers (`write_dataset`, both CLI commands, `spam fit` on the written folder)."""
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import stc_ml_np
import stc_np
from ws_unet_amd import embed, ops, spam, stc, stc_ml
from ws_unet_amd.imread import read_luma_batch

pytestmark = pytest.mark.gpu

SEED = stc_ml_np.SEED
EPS = 2.0 ** -52
GRID = [(s, a, h) for s in stc_ml_np.SHAPES for a in stc_ml_np.ALPHAS for h in stc_ml_np.heights(s)]
CONTENTS = stc_ml_np.CONTENTS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _batch(shape):
    x, rho = zip(*(stc_ml_np.case(c, shape) for c in CONTENTS))
    return _dev(np.stack(x)), _dev(np.stack(rho))


def _close(got, want, rel, what):
    """|got - want| <= rel |want| where want is finite; the same infinities elsewhere; returns the largest relative error seen"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), what
    err = np.abs(got[fin] - want[fin])
    worst = float((err / np.where(want[fin] != 0, np.abs(want[fin]), 1.0)).max()) if fin.any() else 0.0
    assert (err <= rel * np.abs(want[fin])).all(), (what, worst, rel)
    return worst


@pytest.mark.parametrize("shape,alpha,h", GRID)
def test_every_stage_equals_the_restatement(shape, alpha, h):
    n, hw = len(CONTENTS), shape[0] * shape[1]
    k = stc_ml_np.bits_of(shape, alpha)
    cover, rho = _batch(shape)
    m_np = stc_ml_np.message(shape, alpha)
    seeds = [SEED] * n
    msg = stc.random_message(seeds, k, DEV)
    np.testing.assert_array_equal(msg[0].cpu().numpy(), m_np)
    s = embed.seeds_tensor("test", seeds, n, DEV)
    path = stc.key_path(s, *shape, DEV)
    path_np = stc_np.key_path(SEED, hw)
    lam, _, fits = ops.ternary_lambda(cover, rho, torch.full((n,), float(k), dtype=torch.float64, device=DEV))
    assert fits.all()
    # K45
    u1, rho1, ent = ops.stc_layer_high(cover, rho, lam)
    assert u1.dtype == torch.uint8 and rho1.dtype == torch.float64 and ent.dtype == torch.float64 and ent.shape == (n,)
    k1 = torch.clamp(torch.floor(ent), 0, k - 1).to(torch.int32)
    k0 = k - k1
    cols = stc_ml._columns_for(h, hw, torch.cat([k1, k0]), 0, DEV)
    # K43 over the high layer, K46, K43 over the low layer, K47
    y1, _, _, ok1 = ops.stc_embed_ragged(u1, rho1, msg, cols, s, ks=k1, h=h, path=path)
    u0, rho0 = ops.stc_layer_low(cover, rho, lam, y1, k1)
    y0, _, _, ok0 = ops.stc_embed_ragged(u0, rho0, msg, cols, s, ks=k0, first=k1, h=h, path=path)
    stego, changes, dist, ok = ops.stc_layer_compose(cover, rho, y1, y0, k1, ok1, ok0)
    worst1 = 0.0
    for i, c in enumerate(CONTENTS):
        what = f"{c} {shape} alpha {alpha} h {h}"
        x, r = stc_ml_np.case(c, shape)
        lam_i = lam[i].item()
        ref_u1, ref_rho1, ref_h1 = stc_ml_np.high_planes(x, r, lam_i)
        np.testing.assert_array_equal(u1[i].cpu().numpy(), ref_u1, err_msg=what)
        worst1 = max(worst1, _close(rho1[i].cpu().numpy(), ref_rho1, 8 * EPS, what + " rho1"))
        H1 = stc_ml_np.high_entropy(ref_h1)
        assert abs(ent[i].item() - H1) <= (hw + 64) * EPS * H1, (what, ent[i].item(), H1)
        assert abs(H1 - round(H1)) > (hw + 64) * EPS * H1 or H1 == 0.0, (what, H1)          # (so both floors are the same)
        ref_k1 = int(min(np.floor(H1), k - 1))
        assert (k1[i].item(), k0[i].item()) == (ref_k1, k - ref_k1), what
        if c == "ends":
            assert ref_k1 == 0
        shortest = min(v for v in (ref_k1, k - ref_k1) if v > 0)
        ref_y1, ref_ok1 = stc_ml_np.layer(ref_u1, rho1[i].cpu().numpy(), m_np[:ref_k1], h, path_np, hw, shortest)
        np.testing.assert_array_equal(y1[i].cpu().numpy(), ref_y1, err_msg=what + " y1")
        ref_u0, ref_rho0 = stc_ml_np.low_planes(x, r, lam_i, ref_y1, ref_k1)
        np.testing.assert_array_equal(u0[i].cpu().numpy(), ref_u0, err_msg=what + " u0")
        assert np.array_equal(rho0[i].cpu().numpy().view(np.uint64), ref_rho0.view(np.uint64)), what + " rho0"
        ref_y0, ref_ok0 = stc_ml_np.layer(ref_u0, ref_rho0, m_np[ref_k1:], h, path_np, hw, shortest)
        np.testing.assert_array_equal(y0[i].cpu().numpy(), ref_y0, err_msg=what + " y0")
        assert (bool(ok1[i]), bool(ok0[i]), bool(ok[i])) == (ref_ok1, ref_ok0, ref_ok1 and ref_ok0), what
        ref_stego, ref_changes, ref_dist = stc_ml_np.compose(x, r, ref_y1, ref_y0, ref_k1, ref_ok1 and ref_ok0)
        np.testing.assert_array_equal(stego[i].cpu().numpy(), ref_stego, err_msg=what + " stego")
        assert changes[i].item() == ref_changes and abs(dist[i].item() - ref_dist) <= (hw + 64) * EPS * ref_dist, what
        if alpha <= 0.4:
            assert ref_ok1 and ref_ok0, what
        if ref_ok1 and ref_ok0:
            np.testing.assert_array_equal(stc_ml_np.extract(ref_stego, ref_k1, k - ref_k1, h), m_np, err_msg=what)
            d = ref_stego.astype(np.int64) - x
            assert set(np.unique(d)) <= {-1, 0, 1} and not d[np.isinf(r)].any()
        else:
            assert np.array_equal(ref_stego, x) and ref_changes == 0
    print(f"{shape} alpha {alpha} h {h}: largest relative error of rho1 {worst1 / EPS:.2f} x 2^-52 (bound 8); k1 {k1.tolist()}; ok {ok.tolist()}")
    # the driver is this chain
    got = stc_ml.embed(cover, alpha, seeds=seeds, rho=rho, h=h, strict=False)
    assert got[3].dtype == torch.bool and got[4].dtype == torch.int64 and got[4].shape == (n, 2)
    assert torch.equal(got[0], stego) and torch.equal(got[1], changes) and torch.equal(got[2], dist) and torch.equal(got[3], ok.to(torch.bool))
    assert torch.equal(got[4], torch.stack([k1, k0], dim=1).to(torch.int64))
    assert torch.equal(stc_ml.embed(cover, msg.cpu(), seeds=torch.tensor(seeds, dtype=torch.int64), rho=rho, h=h, strict=False)[0], stego)
    # the receiver
    read, ks = stc_ml.extract(stego, got[4], seeds=seeds, h=h)
    assert read.shape == (n, k) and ks.tolist() == [k] * n
    assert all(torch.equal(read[i], msg[i]) for i in range(n) if ok[i])
    # an image alone is the image in the batch
    if h != 10:
        for i in (1, 3):
            one = stc_ml.embed(cover[i:i + 1], alpha, seeds=seeds[i:i + 1], rho=rho[i:i + 1], h=h, strict=False)
            assert all(torch.equal(a[0], b[i]) for a, b in zip(one, got)), i
            assert torch.equal(ops.stc_layer_high(cover[i:i + 1], rho[i:i + 1], lam[i:i + 1])[2][0], ent[i])


def test_unequal_layers_in_one_call_and_a_wrong_key():
    """images of one batch split their message differently; another seed, raster order or swapped layers do not read it"""
    shape, h = (24, 40), 7
    cover, rho = _batch(shape)
    seeds = [embed.image_seed(f"{i}.png", 1) for i in range(4)]
    stego, changes, dist, ok, layers = stc_ml.embed(cover, 0.1, seeds=seeds, rho=rho, h=h)
    k = stc_ml_np.bits_of(shape, 0.1)
    assert ok.all() and (layers.sum(dim=1) == k).all() and layers[3, 0].item() == 0
    assert layers[:, 0].tolist() == [stc_ml_np.reference(c, shape, 0.1, h)["k1"] for c in CONTENTS] and len(set(layers[:, 0].tolist())) > 2
    d = stego.cpu().numpy().astype(np.int64) - cover.cpu().numpy()
    assert np.abs(d).max() == 1 and changes.tolist() == np.count_nonzero(d, axis=(1, 2)).tolist()
    paid = torch.where(stego != cover, rho, torch.zeros_like(rho)).sum(dim=(1, 2))
    assert torch.allclose(paid, dist, rtol=1e-12, atol=0)
    want = stc.random_message(seeds, k, DEV)
    read, ks = stc_ml.extract(stego, layers, seeds=seeds, h=h)
    assert torch.equal(read, want) and ks.tolist() == [k] * 4
    assert torch.equal(stc_ml.extract(stego, layers.cpu().numpy(), seeds=seeds, h=h)[0], want)
    wrong = stc_ml.extract(stego, layers, seeds=[seeds[0] + 1] + seeds[1:], h=h)[0]
    assert not torch.equal(wrong[0], want[0]) and torch.equal(wrong[1:], want[1:])
    assert not torch.equal(stc_ml.extract(stego, layers, seeds=seeds, h=h, permute=False)[0], want)
    # raster order and a given message of another length per call
    msg = _dev(np.stack([stc_np.message_case(shape, 300, w) for w in ("a", "b", "a", "b")]))
    stego, _, _, _, layers = stc_ml.embed(cover, msg, seeds=seeds, rho=rho, h=6, permute=False)
    assert torch.equal(stc_ml.extract(stego, layers, seeds=seeds, h=6, permute=False)[0], msg)


def test_compose_writes_over_the_cover_and_copies_what_is_not_ok():
    shape, h = (33, 31), 7
    cover, rho = _batch(shape)
    n, hw = 4, 1023
    k = stc_ml_np.bits_of(shape, 0.4)
    s = embed.seeds_tensor("test", [SEED] * n, n, DEV)
    msg = stc.random_message([SEED] * n, k, DEV)
    lam = ops.ternary_lambda(cover, rho, torch.full((n,), float(k), dtype=torch.float64, device=DEV))[0]
    u1, rho1, ent = ops.stc_layer_high(cover, rho, lam)
    k1 = torch.clamp(torch.floor(ent), 0, k - 1).to(torch.int32)
    cols = stc_ml._columns_for(h, hw, torch.cat([k1, k - k1]), 0, DEV)
    path = stc.key_path(s, *shape, DEV)
    y1, _, _, ok1 = ops.stc_embed_ragged(u1, rho1, msg, cols, s, ks=k1, h=h, path=path)
    u0, rho0 = ops.stc_layer_low(cover, rho, lam, y1, k1)
    y0, _, _, ok0 = ops.stc_embed_ragged(u0, rho0, msg, cols, s, ks=k - k1, first=k1, h=h, path=path)
    assert ok1.all() and ok0.all()
    ok0[2] = 0
    ok1[0] = 0
    stego, changes, dist, ok = ops.stc_layer_compose(cover, rho, y1, y0, k1, ok1, ok0)
    assert ok.tolist() == [0, 1, 0, 1] and changes[0].item() == 0 and dist[2].item() == 0.0
    assert torch.equal(stego[0], cover[0]) and torch.equal(stego[2], cover[2]) and (stego[1] != cover[1]).any()
    lib = ops._lib.load()
    over = cover.clone()
    ws = torch.empty(lib.wsu_stc_layer_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    c2, d2, o2 = torch.empty_like(changes), torch.empty_like(dist), torch.empty_like(ok)
    ops.check(lib.wsu_stc_layer_compose(over.data_ptr(), rho.data_ptr(), y1.data_ptr(), y0.data_ptr(), k1.data_ptr(), ok1.data_ptr(), ok0.data_ptr(),
                                        over.data_ptr(), c2.data_ptr(), d2.data_ptr(), o2.data_ptr(), ws.data_ptr(), ws.numel(), n, shape[0], shape[1],
                                        ops._stream()), "wsu_stc_layer_compose")
    assert torch.equal(over, stego) and torch.equal(c2, changes) and torch.equal(d2, dist) and torch.equal(o2, ok)


def test_strict_names_the_images_and_the_reason():
    shape = (33, 31)
    cover, rho = _batch(shape)                                               # noise, photo, flat, ends
    rho = rho.clone()
    rho[2] = float("inf")
    assert not stc_ml_np.reference("photo", shape, 1.0, 6)["ok0"]
    with pytest.raises(ValueError, match=r"image\(s\) 1 \(the low layer has no solution\), 2 \(the payload exceeds the capacity\) of"):
        stc_ml.embed(cover, 1.0, seeds=[SEED] * 4, rho=rho, h=6)
    stego, changes, dist, ok, layers = stc_ml.embed(cover, 1.0, seeds=[SEED] * 4, rho=rho, h=6, strict=False)
    assert ok.tolist() == [True, False, False, True] and torch.equal(stego[1], cover[1]) and torch.equal(stego[2], cover[2])
    assert changes.tolist()[1:3] == [0, 0] and dist.tolist()[1:3] == [0.0, 0.0] and (layers.sum(dim=1) == 1023).all()


def test_layer_argument_errors():
    cover = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    rho = torch.ones((2, 8, 8), dtype=torch.float64, device=DEV)
    lam = torch.ones(2, dtype=torch.float64, device=DEV)
    k1 = torch.ones(2, dtype=torch.int32, device=DEV)
    ok = torch.ones(2, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="rho must be"):
        ops.stc_layer_high(cover, rho.float(), lam)
    with pytest.raises(ValueError, match="lambdas must be"):
        ops.stc_layer_high(cover, rho, lam[:1])
    with pytest.raises(ValueError, match="y1 must be"):
        ops.stc_layer_low(cover, rho, lam, cover[:1], k1)
    with pytest.raises(ValueError, match="k1 must be"):
        ops.stc_layer_low(cover, rho, lam, cover, k1.to(torch.int64))
    with pytest.raises(ValueError, match="y0 must be"):
        ops.stc_layer_compose(cover, rho, cover, cover.float(), k1, ok, ok)
    with pytest.raises(ValueError, match="ok0 must be"):
        ops.stc_layer_compose(cover, rho, cover, cover, k1, ok, ok.to(torch.bool))


def test_write_dataset_cli_and_spam(tmp_path, capsys):
    data = tmp_path / "data"
    (data / "images").mkdir(parents=True)
    covers = (6, 7)
    for c in covers:
        shutil.copy(GOLDEN / f"cover_{c}.png", data / "images" / f"{c}.png")
    (data / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{c}.png,512,512\n" for c in covers))
    x = torch.from_numpy(read_luma_batch([data / "images" / f"{c}.png" for c in covers])).to(DEV)
    seeds = [embed.image_seed(f"{c}.png", 2) for c in covers]
    # random bits at one alpha, h = 7
    folders = stc_ml.write_dataset(data, "stct", 0.1, h=7, stream=2)
    assert folders == [data / "stego_STCT_alpha_0.1_independent_images"]
    stego, changes, dist, ok, layers = stc_ml.embed(x, 0.1, seeds=seeds, h=7)
    k = int(round(0.1 * 512 * 512))
    assert (folders[0] / "files.csv").read_text().splitlines() == ["name,height,width,stego_method,alpha,bits_high,bits_low"] + [
        f"stego_STCT_alpha_0.1_independent_images/{c}.png,512,512,STCT,0.1,{layers[i, 0].item()},{layers[i, 1].item()}" for i, c in enumerate(covers)]
    assert (layers[:, 0] > 0).all() and (layers.sum(dim=1) == k).all()
    files = torch.from_numpy(read_luma_batch([folders[0] / f"{c}.png" for c in covers])).to(DEV)
    assert torch.equal(files, stego)
    assert torch.equal(stc_ml.extract(files, layers, seeds=seeds, h=7)[0], stc.random_message(seeds, k, DEV))
    with capsys.disabled():
        print(f"512 x 512, alpha 0.1, h 7: layers {layers.tolist()} changes {changes.tolist()} distortion {dist.tolist()}")
    capsys.readouterr()
    # a message file through both CLI commands, h = 10
    text = bytes(range(256)) * 2 + b"a message that two layers carry"
    (tmp_path / "message.bin").write_bytes(text)
    alpha = 8 * len(text) / (512 * 512)
    stc_ml.main(["embed", "--data", str(data), "--message", str(tmp_path / "message.bin"), "--stream", "2"])
    folder = data / stc_ml.folder_name("STCT", alpha)
    assert capsys.readouterr().out.split() == [str(folder)]
    files = read_luma_batch([folder / f"{c}.png" for c in covers])
    d = files.astype(np.int64) - x.cpu().numpy()
    assert np.abs(d).max() == 1 and 0 < np.count_nonzero(d) < 8 * len(text)
    stc_ml.main(["extract", "--data", str(data), "--alpha", repr(alpha), "--stream", "2", "--out", str(tmp_path / "read")])
    assert capsys.readouterr().out.split() == [str(tmp_path / "read" / f"{c}.bin") for c in covers]
    for c in covers:
        assert (tmp_path / "read" / f"{c}.bin").read_bytes() == text
    stc_ml.main(["extract", "--data", str(data), "--alpha", repr(alpha), "--stream", "1", "--out", str(tmp_path / "wrong")])
    assert (tmp_path / "wrong" / "6.bin").read_bytes() != text
    # the SPAM detector reads the new folder from its files
    rows, F = spam.extract(data, "STCT", 0.1)
    assert rows["name"].tolist() == [f"stego_STCT_alpha_0.1_independent_images/{c}.png" for c in covers] and (rows["stego_method"] == "STCT").all()
    np.testing.assert_array_equal(F, spam.features(ops.spam_counts(stego)))
    spam.main(["fit", "--data", str(data), "--stego-methods", "STCT", "--alphas", "0.1", "--out", str(tmp_path / "fld.npz")])
    model = spam.FLD.load(tmp_path / "fld.npz")
    assert model.stego_methods == ["STCT"] and model.alphas == [0.1] and np.isfinite(model.w).all()
