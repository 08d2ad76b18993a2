"""GPU: the stego simulators (K20-K23, ws_unet_amd.embed) against the reference's HILLR files, the numpy restatements of
tests/embed_np.py, and end to end through the CLI, fabrika and the pair loader."""
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV, check_span_placements
import embed_np
import hill_np
from ws_unet_amd import embed, fabrika, ops
from ws_unet_amd.data.pairs import PairLoader
from ws_unet_amd.imread import imread4_u8, read_luma_batch

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
SHAPES = [(8, 8), (64, 64), (70, 90), (65, 130)]          # padding wider than the image; one tile; ragged tiles; odd width, 3 x 5 tiles
CONTENTS = ("noise", "crop", "flat_block")
HILLR_ALPHAS = (0.01, 0.1, 0.4, 1.0)


def _hashed(h, w, seed):
    v = (np.arange(h * w, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    v ^= v >> np.uint64(29)
    v *= np.uint64(0xBF58476D1CE4E5B9)
    v ^= v >> np.uint64(32)
    return (v & np.uint64(0xFF)).astype(np.uint8).reshape(h, w)


@pytest.fixture(scope="module")
def covers():
    return np.stack([imread4_u8(GOLDEN / f"cover_{k}.png")[..., 3] for k in COVERS])


@pytest.fixture(scope="module")
def planes(covers):
    """{(h, w): ((3,h,w) uint8 planes in CONTENTS order, their float64 hill_np costs)}: computed once, never written to."""
    out = {}
    for h, w in SHAPES:
        noise = _hashed(h, w, 17 * h + w)
        crop = covers[2][200:200 + h, 100:100 + w].copy()
        flat = _hashed(h, w, 5 * h + w)
        flat[h // 8:h // 8 + max(6, h // 3), w // 8:w // 8 + max(6, w // 3)] = 77             # S == 0 inside: inf -> clamp around it
        x = np.stack([noise, crop, flat])
        cost = np.stack([hill_np.hill_cost(p) for p in x])
        assert (cost[2] == 1e10).any()
        x.setflags(write=False); cost.setflags(write=False)
        out[(h, w)] = (x, cost)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- the reference's files ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha,changes", [(0.01, 1311), (0.4, 52429)])
def test_hillr_equals_the_reference_files(covers, alpha, changes):
    x = torch.from_numpy(covers).to(DEV)
    stego, ch = embed.simulate(x, "HILLr", alpha)
    ref = np.stack([imread4_u8(GOLDEN / f"stego_HILLR_{alpha}_{k}.png")[..., 3] for k in COVERS])
    got = stego.cpu().numpy()
    assert got.dtype == np.uint8 and (got == ref).all()
    assert ch.dtype == torch.int64 and ch.tolist() == [changes] * 5
    again, ch2 = embed.simulate(x, "HILLR", alpha)
    assert torch.equal(again, stego) and torch.equal(ch2, ch)


# ---- K20 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_key_bits_equal_numpy(planes, shape):
    x, cost = planes[shape]
    key = ops.hill_cost_f64(torch.from_numpy(x.copy()).to(DEV))
    assert key.dtype == torch.float64 and tuple(key.shape) == x.shape
    got = key.cpu().numpy()
    for i, name in enumerate(CONTENTS):
        bad = np.flatnonzero(_bits(got[i]) != _bits(cost[i]))
        assert bad.size == 0, (name, bad[:5], got[i].reshape(-1)[bad[:5]], cost[i].reshape(-1)[bad[:5]])
    # an image alone, unaligned in its batch or not, has the bits it has in the batch
    assert torch.equal(ops.hill_cost_f64(torch.from_numpy(x[1:2].copy()).to(DEV))[0], key[1])


def test_key_bits_equal_numpy_on_a_cover(covers):
    """the 16-byte staging path (tiles well inside a 512-wide image) and a relative gap of 9.4e-8 at the alpha 0.4 threshold of cover 8"""
    key = ops.hill_cost_f64(torch.from_numpy(covers[2:3]).to(DEV))[0].cpu().numpy()
    assert (_bits(key) == _bits(hill_np.hill_cost(covers[2]))).all()


# ---- HILLR ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hillr_equals_numpy(planes, shape):
    x, cost = planes[shape]
    xd = torch.from_numpy(x.copy()).to(DEV)
    masks = []
    for alpha in HILLR_ALPHAS:
        stego, ch = embed.simulate(xd, "HILLR", alpha)
        got = stego.cpu().numpy()
        for i in range(3):
            assert (got[i] == embed_np.hillr_np(x[i], alpha, cost[i])).all(), (alpha, CONTENTS[i])
        assert ((got ^ x) <= 1).all()                                              # only LSBs differ
        assert ch.tolist() == [int((got[i] != x[i]).sum()) for i in range(3)]
        assert all(c >= embed_np.hillr_rank(alpha, *shape) + 1 for c in ch.tolist())
        masks.append(got != x)
    for small, large in zip(masks, masks[1:]):                                      # nested across alphas
        assert not (small & ~large).any()
    # one alpha per image, alpha 0 among them
    mixed = (0.4, 0.0, 0.1)
    stego, ch = embed.simulate(xd, "HILLR", mixed)
    for i, a in enumerate(mixed):
        assert (stego[i].cpu().numpy() == embed_np.hillr_np(x[i], a, cost[i])).all()
    assert ch[1].item() == 0
    assert torch.equal(embed.simulate(xd, "HILLR", 0.0)[0], xd)


def test_hillr_flips_every_tie_at_the_threshold():
    """more than half of the keys are the clamp: at alpha 1 the threshold is the clamp and every pixel flips, as in hillr_np"""
    x = _hashed(64, 64, 3)
    x[:48] = 200
    cost = hill_np.hill_cost(x)
    assert (cost == 1e10).mean() > 0.5
    for alpha in (1.0, 0.4, 0.01):
        stego, ch = embed.simulate(torch.from_numpy(x)[None].to(DEV), "HILLR", alpha)
        ref = embed_np.hillr_np(x, alpha, cost)
        assert (stego[0].cpu().numpy() == ref).all() and ch.item() == int((ref != x).sum())
        if alpha == 1.0:
            assert ch.item() == 64 * 64
    flat = torch.full((2, 40, 50), 9, dtype=torch.uint8, device=DEV)                # a flat image is flipped entirely
    stego, ch = embed.simulate(flat, "HILLR", 0.01)
    assert (stego == 8).all() and ch.tolist() == [2000, 2000]


def test_rank_select_edges(planes):
    x, cost = planes[(70, 90)]
    key = ops.hill_cost_f64(torch.from_numpy(x.copy()).to(DEV))
    ranks = [0, 70 * 90 - 1, 3150]
    got = ops.rank_select_f64(key, torch.tensor(ranks, device=DEV)).cpu().numpy().view(np.uint64)
    for i, k in enumerate(ranks):
        assert got[i] == _bits(np.sort(cost[i].reshape(-1))[k:k + 1])[0]
    edge = ops.rank_select_f64(key, torch.tensor([-1, 10 ** 9, -5], device=DEV)).cpu().numpy().view(np.uint64)
    assert edge[0] == 0 and edge[2] == 0 and edge[1] == _bits(cost[1].max(keepdims=True).reshape(1))[0]


# ---- LSBR -------------------------------------------------------------------------------------------------------------------------

SEEDS = (5, (3 << 32) | 0x7654321, 2 ** 64 - 1)


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (64, 64), (70, 90)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lsbr_equals_numpy(shape):
    h, w = shape
    x = np.stack([_hashed(h, w, 100 + i) for i in range(3)])
    xd = torch.from_numpy(x).to(DEV)
    for alpha in (0.0, 0.01, 0.4, 1.0):
        stego, ch = embed.simulate(xd, "lsbr", alpha, SEEDS)
        got = stego.cpu().numpy()
        for i in range(3):
            assert (got[i] == embed_np.lsbr_np(x[i], alpha, SEEDS[i])).all(), (alpha, i)
        assert ch.tolist() == [int((got[i] ^ x[i]).sum()) for i in range(3)]       # the difference is 0 / 1: its sum is its popcount
        assert ((got ^ x) <= 1).all()
        if alpha == 0.0:
            assert (got == x).all()
    # one alpha per image; an image alone equals the same image at batch position 2
    mixed = (0.4, 1.0, 0.01)
    stego, ch = embed.simulate(xd, "LSBR", mixed, torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in SEEDS]))
    for i in range(3):
        assert (stego[i].cpu().numpy() == embed_np.lsbr_np(x[i], mixed[i], SEEDS[i])).all()
    alone, ch1 = embed.simulate(xd[2:3].clone(), "LSBR", mixed[2], [SEEDS[2]])
    assert torch.equal(alone[0], stego[2]) and ch1[0] == ch[2]
    again, ch2 = embed.simulate(xd, "LSBR", mixed, SEEDS)
    assert torch.equal(again, stego) and torch.equal(ch2, ch)


def test_lsbr_where_cover_and_stego_differ_in_alignment():
    """test_lsbr_equals_numpy reaches the pixel loop's paths (a) - (d) (three images of 1x1, 3x5 and 70x90 start off the 16-byte grid);
    (e) needs the raw entry."""
    lib = ops._lib.load()
    seeds = torch.tensor([SEEDS[1]], dtype=torch.int64, device=DEV)
    thr = torch.from_numpy(np.array([ops.lsbr_threshold(0.4)], dtype=np.uint32).view(np.int32)).to(DEV)
    check_span_placements("e", lambda ci, co, ch, h, w: lib.wsu_embed_lsbr(ci, seeds.data_ptr(), thr.data_ptr(), co, ch, 1, h, w, ops._stream()),
                          lambda plane: embed_np.lsbr_np(plane, 0.4, SEEDS[1]))


def test_lsbr_rate_on_a_cover(covers):
    x = torch.from_numpy(covers[:1]).to(DEV)
    stego, ch = embed.simulate(x, "LSBR", 0.4, [embed.image_seed("images/6.png")])
    assert abs(ch.item() / 512 ** 2 - 0.2) < 4 * np.sqrt(0.2 * 0.8) / 512             # 4 sigma of the binomial count
    assert (stego[0].cpu().numpy() == embed_np.lsbr_np(covers[0], 0.4, embed.image_seed("6.png"))).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def _covers_dataset(root):
    (root / "images").mkdir(parents=True)
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    return root


@fabrika.stego_spatial(iterator=None, convert_to=None, ignore_missing=False)
def _stego_rows(df, **kw):
    return df


def _batches(loader):
    return [(i.clone(), c.clone(), a.clone()) for i, (c, a) in loader]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for ba, bb in zip(a, b) for x, y in zip(ba, bb))


def test_cli_fabrika_and_pair_loader(tmp_path, covers, capsys):
    data, bare = _covers_dataset(tmp_path / "data"), _covers_dataset(tmp_path / "covers_only")
    kw = dict(batch_size=4, device=torch.device(DEV), seed=3)
    sim = {m: PairLoader(bare, None, m, 0.4, simulate=True, **kw) for m in ("HILLR", "LSBR")}
    stream = sim["LSBR"].lsbr_stream(0)
    assert stream == sim["LSBR"].lsbr_stream() and stream != sim["LSBR"].lsbr_stream(1)
    embed.main(["--data", str(data), "--stego-method", "hillr", "--alphas", "0.4"])
    embed.main(["--data", str(data), "--stego-method", "LSBR", "--alphas", ".4", "--stream", str(stream)])
    printed = capsys.readouterr().out.split()
    assert printed == [str(data / f"stego_{m}_alpha_0.4_independent_images") for m in ("HILLR", "LSBR")]
    x = torch.from_numpy(covers).to(DEV)
    order = ["10", "6", "7", "8", "9"]                                              # fabrika sorts names lexically
    for m in ("HILLR", "LSBR"):
        folder = f"stego_{m}_alpha_0.4_independent_images"
        assert (data / folder / "files.csv").read_text().splitlines()[:2] == ["name,height,width,stego_method,alpha", f"{folder}/10.png,512,512,{m},0.4"]
        rows = _stego_rows(data, stego_method=m, alpha=0.4)
        assert [str(n) for n in rows["name"]] == [str(data / folder / f"{s}.png") for s in order]
        files = read_luma_batch([data / folder / f"{k}.png" for k in COVERS])
        twins = embed.simulate(x, m, 0.4, [embed.image_seed(f"{k}.png", stream) for k in COVERS])[0]
        assert (files == twins.cpu().numpy()).all()
        # the file route (two decodes per pair) and the simulated route (covers alone) yield the same batches
        from_files = PairLoader(data, None, m, 0.4, **kw)
        assert from_files.covers == sim[m].covers and from_files.alphas == sim[m].alphas and len(from_files) == len(sim[m]) == 2
        a, b = _batches(from_files), _batches(sim[m])
        assert len(a) == 2 and a[0][0].shape == (4, 1, 512, 512) and a[0][2].tolist() == pytest.approx([0.0, 0.4, 0.0, 0.4])
        assert _same(a, b)
    # the next epoch: HILLR twins are the same files' twins, LSBR twins are drawn afresh (shuffle off: the same pairs per batch)
    for m in ("HILLR", "LSBR"):
        loader = PairLoader(bare, None, m, 0.4, simulate=True, shuffle=False, **kw)
        first = _batches(loader)
        assert _same(first, _batches(loader))
        loader.reshuffle()
        second = _batches(loader)
        assert all(torch.equal(p[1], q[1]) and torch.equal(p[0][0::2], q[0][0::2]) for p, q in zip(first, second))      # covers
        assert _same(first, second) == (m == "HILLR")
        if m == "LSBR":
            assert all(not torch.equal(p[0][1], q[0][1]) for p, q in zip(first, second))
