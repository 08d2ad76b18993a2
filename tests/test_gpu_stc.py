"""GPU: the syndrome-trellis code kernels (K40-K42, ops.philox_words / stc_embed / stc_extract, ws_unet_amd.stc) against the numpy
restatement (stc_np) on its shared inputs, bit for bit: stego, cost (as uint64 patterns), changes and ok on both sides of the one-wave /
many-waves boundary; the receiver; the round trip through the keyed path; the +-1 change rule; the workspace cap; and the drivers
(`write_dataset`, both CLI commands, the WS table driver on the new folder)."""
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import stc_np
from ws_unet_amd import embed, fabrika, ops, stc
from ws_unet_amd.imread import read_luma_batch

pytestmark = pytest.mark.gpu

GRID = [(h, s) for h in stc_np.HEIGHTS for s in stc_np.SHAPES]
SEED = stc_np.SEED


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV) if dtype is None else torch.tensor(a, dtype=dtype, device=DEV)


def _cols(h, n, k):
    return _dev(stc_np.columns(h, -(-n // k)).view(np.int32))


def _seeds(n, seed=SEED):
    return _dev(np.full(n, seed, dtype=np.uint64).view(np.int64))


def _batch(shape, names, k):
    covers, rhos = zip(*(stc_np.image_case(shape, w) for w in names))
    msgs = [stc_np.message_case(shape, k, w) for w in names]
    return _dev(np.stack(covers)), _dev(np.stack(rhos)), _dev(np.stack(msgs))


def _same(got, want, what):
    """got: (stego, cost, changes, ok) tensors of one image; want: stc_np.stego's tuple"""
    stego, cost, changes, ok = got
    np.testing.assert_array_equal(stego.cpu().numpy(), want[0], err_msg=what)
    assert cost.cpu().numpy().view(np.uint64) == np.float64(want[1]).view(np.uint64), (what, cost.item(), want[1])
    assert changes.item() == want[2] and bool(ok.item()) == want[3], what


# ---- K41 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,shape", GRID)
def test_embed_equals_the_restatement_bit_for_bit(h, shape):
    """per message length (n / k no integer; k < h; k == n): a batch of image 'b', image 'a' and 'a' with every 7th cost wet; the middle
    image alone; a second call; the identity path against path=None"""
    n = shape[0] * shape[1]
    names = ("b", "a", "wet")
    for k in stc_np.ks_of(shape, h):
        cover, rho, msg = _batch(shape, names, k)
        cols, seeds = _cols(h, n, k), _seeds(3)
        got = ops.stc_embed(cover, rho, msg, cols, seeds, h=h)
        assert got[0].dtype == torch.uint8 and got[1].dtype == torch.float64 and got[2].dtype == torch.int64 and got[3].dtype == torch.uint8
        for i, w in enumerate(names):
            want = stc_np.reference(shape, w, h, k)
            _same([t[i] for t in got], want, f"h {h} k {k} image {w}")
            if want[3]:
                np.testing.assert_array_equal(stc_np.syndrome(want[0].reshape(-1) & 1, k, stc_np.columns(h, -(-n // k)), h),
                                              stc_np.message_case(shape, k, w))
        assert got[2].tolist() == (got[0] != cover).sum(dim=(1, 2)).tolist()
        alone = ops.stc_embed(cover[1:2], rho[1:2], msg[1:2], cols, seeds[1:2], h=h)
        again = ops.stc_embed(cover, rho, msg, cols, seeds, h=h)
        ident = torch.arange(n, dtype=torch.int32, device=DEV).expand(3, -1).contiguous()
        keyed = ops.stc_embed(cover, rho, msg, cols, seeds, h=h, path=ident)
        for j in range(4):
            assert torch.equal(alone[j][0], got[j][1]) and torch.equal(again[j], got[j]) and torch.equal(keyed[j], got[j]), (h, k, j)


@pytest.mark.parametrize("h", stc_np.HEIGHTS)
def test_infeasible_image_keeps_its_cover(h):
    """every cost wet and the cover no solution: ok 0, cost +inf, stego = cover, no change; its neighbour in the batch is embedded"""
    shape = (8, 16)
    k = stc_np.ks_of(shape, h)[0]
    cover, rho, msg = _batch(shape, ("allwet", "a"), k)
    assert torch.equal(msg[0], msg[1])                                       # (message_case: 'allwet' carries the message of 'a')
    stego, cost, changes, ok = ops.stc_embed(cover, rho, msg, _cols(h, 128, k), _seeds(2), h=h)
    assert ok.tolist() == [0, 1] and cost[0].item() == float("inf") and changes[0].item() == 0 and torch.equal(stego[0], cover[0])
    _same((stego[0], cost[0], changes[0], ok[0]), stc_np.reference(shape, "allwet", h, k), f"h {h} all wet")
    _same((stego[1], cost[1], changes[1], ok[1]), stc_np.reference(shape, "a", h, k), f"h {h} beside all wet")


@pytest.mark.parametrize("h,shape", [(6, (24, 40)), (7, (33, 31)), (10, (24, 40))])
def test_keyed_path_and_pm1_equal_the_restatement(h, shape):
    """along the path of the seed: ops.philox_words and stc.key_path are the restatement's; 'flip' and 'pm1' are its stego bit for bit
    (so the sign of a change follows bit 0 of the pixel's restated generator word); both carry the same LSBs; |stego - cover| <= 1"""
    n = shape[0] * shape[1]
    k = stc_np.ks_of(shape, h)[0]
    cover, rho, msg = _batch(shape, ("a",), k)
    seeds = _seeds(1)
    words = ops.philox_words(seeds, *shape)
    assert words.dtype == torch.int32 and words.shape == (1,) + shape
    np.testing.assert_array_equal(words.cpu().numpy().view(np.uint32).reshape(-1), stc_np.words(n, SEED))
    path = stc.key_path([SEED], *shape, DEV)
    assert path.dtype == torch.int32 and path.shape == (1, n)
    np.testing.assert_array_equal(path[0].cpu().numpy(), stc_np.key_path(SEED, n))
    out = {}
    for change in ("flip", "pm1"):
        got = ops.stc_embed(cover, rho, msg, _cols(h, n, k), seeds, h=h, path=path, change=change)
        _same([t[0] for t in got], stc_np.reference(shape, "a", h, k, change, True), f"h {h} {change}")
        out[change] = got[0][0].cpu().numpy().astype(np.int64)
    c = cover[0].cpu().numpy().astype(np.int64)
    assert np.abs(out["pm1"] - c).max() == 1 and np.array_equal(out["pm1"] & 1, out["flip"] & 1)
    assert (out["pm1"] - c > 0).any() and (out["pm1"] - c < 0).any()


def test_pm1_stays_in_range_at_the_ends():
    """a plane of 0 and 255 only: every change goes inwards"""
    shape, h = (24, 40), 7
    k = stc_np.ks_of(shape, h)[0]
    cover, rho = stc_np.image_case(shape, "ends")
    msg = stc_np.message_case(shape, k, "a")
    stego, cost, changes, ok = ops.stc_embed(_dev(cover[None]), _dev(rho[None]), _dev(msg[None]), _cols(h, 960, k), _seeds(1), h=h, change="pm1")
    want = stc_np.stego(cover, rho, msg, stc_np.columns(h, -(-960 // k)), h, change="pm1", seed=SEED)
    _same((stego[0], cost[0], changes[0], ok[0]), want, "ends")
    s = stego[0].cpu().numpy()
    assert set(np.unique(s)) <= {0, 1, 254, 255} and changes.item() > 100
    assert (s[cover == 0] <= 1).all() and (s[cover == 255] >= 254).all()


def test_workspace_cap_slices_the_batch():
    shape, h = (24, 40), 7
    k = stc_np.ks_of(shape, h)[0]
    names = ("a", "b", "wet", "b", "a")
    cover, rho, msg = _batch(shape, names, k)
    cols, seeds = _cols(h, 960, k), _dev(np.arange(5, dtype=np.int64) + 3)
    per = ops.stc_workspace_bytes(960, h)
    assert per == 960 * 16
    whole = ops.stc_embed(cover, rho, msg, cols, seeds, h=h, change="pm1")
    for cap in (2 * per + 5, 1, per):                                        # slices of 2, and of 1 (a cap below one image still holds one)
        cut = ops.stc_embed(cover, rho, msg, cols, seeds, h=h, change="pm1", workspace_cap=cap)
        assert all(torch.equal(a, b) for a, b in zip(cut, whole)), cap
    for i in range(5):
        one = ops.stc_embed(cover[i:i + 1], rho[i:i + 1], msg[i:i + 1], cols, seeds[i:i + 1], h=h, change="pm1")
        assert all(torch.equal(a[0], b[i]) for a, b in zip(one, whole)), i
    # the two phases on the caller's workspace are the call
    ws = torch.empty(5 * per, dtype=torch.uint8, device=DEV)
    fwd = ops.stc_embed(cover, rho, msg, cols, seeds, h=h, change="pm1", phases=1, workspace=ws)
    assert torch.equal(fwd[1], whole[1]) and torch.equal(fwd[3], whole[3])
    # (phase 2 alone takes phase 1's cost and ok as arguments: the C entry)
    lib = ops._lib.load()
    stego, changes = torch.empty_like(cover), torch.empty(5, dtype=torch.int64, device=DEV)
    ops.check(lib.wsu_stc_embed(cover.data_ptr(), rho.data_ptr(), msg.data_ptr(), cols.data_ptr(), None, seeds.data_ptr(), 1, h, k, 2,
                                stego.data_ptr(), fwd[1].data_ptr(), changes.data_ptr(), fwd[3].data_ptr(), ws.data_ptr(), ws.numel(), 5,
                                shape[0], shape[1], ops._stream()), "wsu_stc_embed")
    assert torch.equal(stego, whole[0]) and torch.equal(changes, whole[2])


def test_ops_argument_errors():
    cover = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    rho = torch.ones((2, 8, 8), dtype=torch.float64, device=DEV)
    msg = torch.zeros((2, 20), dtype=torch.uint8, device=DEV)
    cols, seeds = _cols(7, 64, 20), _seeds(2)
    with pytest.raises(ValueError, match="outside 1..10"):
        ops.stc_embed(cover, rho, msg, cols, seeds, h=11)
    with pytest.raises(ValueError, match="rho must be"):
        ops.stc_embed(cover, rho.float(), msg, cols, seeds, h=7)
    with pytest.raises(ValueError, match="message must be"):
        ops.stc_embed(cover, rho, msg[:1], cols, seeds, h=7)
    with pytest.raises(ValueError, match="outside 1..64"):
        ops.stc_embed(cover, rho, torch.zeros((2, 65), dtype=torch.uint8, device=DEV), cols, seeds, h=7)
    with pytest.raises(ValueError, match="cols must be"):
        ops.stc_embed(cover, rho, msg, cols[:3], seeds, h=7)
    with pytest.raises(ValueError, match="path must be"):
        ops.stc_embed(cover, rho, msg, cols, seeds, h=7, path=torch.zeros((2, 63), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="change"):
        ops.stc_embed(cover, rho, msg, cols, seeds, h=7, change="both")
    with pytest.raises(ValueError, match="workspace_cap"):
        ops.stc_embed(cover, rho, msg, cols, seeds, h=7, workspace_cap=0)
    with pytest.raises(ValueError, match="phases"):
        ops.stc_embed(cover, rho, msg, cols, seeds, h=7, phases=1)
    with pytest.raises(ValueError, match="phases"):
        ops.stc_embed(cover, rho, msg, cols, seeds, h=7, phases=2, workspace=torch.empty(2 * 64 * 16, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="outside 1..64"):
        ops.stc_extract(cover, cols, 0, h=7)
    with pytest.raises(ValueError, match="stc_workspace_bytes"):
        ops.stc_workspace_bytes(64, 0)


# ---- K42 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,shape", GRID)
def test_extract_equals_the_restatement(h, shape):
    """the receiver on arbitrary planes (two images, raster and keyed path), and on K41's stego: the message"""
    n = shape[0] * shape[1]
    planes = np.stack([stc_np.image_case(shape, w)[0] for w in ("a", "b")])
    path_np = np.stack([stc_np.key_path(SEED, n), stc_np.key_path(SEED + 1, n)])
    for k in stc_np.ks_of(shape, h):
        cols_np = stc_np.columns(h, -(-n // k))
        cols = _cols(h, n, k)
        got = ops.stc_extract(_dev(planes), cols, k, h=h)
        assert got.dtype == torch.uint8 and got.shape == (2, k)
        keyed = ops.stc_extract(_dev(planes), cols, k, h=h, path=_dev(path_np))
        for i in range(2):
            flat = planes[i].reshape(-1) & 1
            np.testing.assert_array_equal(got[i].cpu().numpy(), stc_np.syndrome(flat, k, cols_np, h), err_msg=f"h {h} k {k}")
            np.testing.assert_array_equal(keyed[i].cpu().numpy(), stc_np.syndrome(flat[path_np[i]], k, cols_np, h), err_msg=f"h {h} k {k} keyed")
        cover, rho, msg = _batch(shape, ("a", "wet"), k)
        stego, _, _, ok = ops.stc_embed(cover, rho, msg, cols, _seeds(2), h=h)
        assert ok.tolist() == [1, stc_np.reference(shape, "wet", h, k)[3]]         # (wet pixels leave no solution where k == n)
        read = ops.stc_extract(stego, cols, k, h=h)
        assert all(torch.equal(read[i], msg[i]) for i in range(2) if ok[i]), (h, k)


# ---- embed / extract ------------------------------------------------------------------------------------------------------------------------

def _golden_crop():
    return read_luma_batch([GOLDEN / "cover_6.png"])[0][192:320, 192:320]


@pytest.mark.parametrize("source", ["noise64", "golden128"])
def test_round_trip_through_the_keyed_path(source):
    """stc.extract(stc.embed(m)) == m at alpha 0.4 and 0.1, h = 10, both change rules, the path and the random message from the seeds; a
    wrong seed does not read it; a given message and raster order work too"""
    plane = np.random.default_rng(64).integers(0, 256, (64, 64)).astype(np.uint8) if source == "noise64" else np.ascontiguousarray(_golden_crop())
    hh, ww = plane.shape
    cover = _dev(np.stack([plane, plane[::-1].copy()]))
    seeds = [embed.image_seed("6.png", 3), embed.image_seed("7.png", 3)]
    rho = ops.hill_cost_f64(cover)
    for alpha in (0.4, 0.1):
        k = int(round(alpha * hh * ww))
        want = stc.random_message(seeds, k, DEV)
        np.testing.assert_array_equal(want[0].cpu().numpy(), stc_np.random_message(seeds[0], k))
        assert 0.4 < want.float().mean().item() < 0.6 and not torch.equal(want[0], want[1])
        for change in ("flip", "pm1"):
            stego, changes, cost, ok = stc.embed(cover, alpha, seeds=seeds, change=change, rho=rho)
            assert ok.dtype == torch.bool and ok.all() and stego.shape == cover.shape
            d = stego.cpu().numpy().astype(np.int64) - cover.cpu().numpy()
            assert np.abs(d).max() == 1 and changes.tolist() == np.count_nonzero(d, axis=(1, 2)).tolist()
            assert (0 < changes).all() and (changes < k / 2).all()           # fewer changes than uncoded embedding's k / 2
            paid = (rho * (stego != cover)).sum(dim=(1, 2))
            assert torch.allclose(paid, cost, rtol=1e-9, atol=0)
            print(f"{source} alpha {alpha} {change}: k {k} changes {changes.tolist()} cost {cost.tolist()}")
            assert torch.equal(stc.extract(stego, k, seeds=seeds), want)
            wrong = stc.extract(stego, k, seeds=[seeds[0] + 1, seeds[1]])
            assert not torch.equal(wrong[0], want[0]) and torch.equal(wrong[1], want[1])
            assert not torch.equal(stc.extract(stego, k, seeds=seeds, permute=False), want)
    msg = _dev(np.stack([stc_np.message_case((hh, ww), 700, w) for w in ("a", "b")]))
    for permute in (True, False):
        stego = stc.embed(cover, msg, seeds=seeds, permute=permute, h=7)[0]
        assert torch.equal(stc.extract(stego, 700, seeds=seeds, permute=permute, h=7), msg)
    assert torch.equal(stc.embed(cover, msg.cpu(), seeds=torch.tensor(seeds), h=7)[0], stc.embed(cover, msg, seeds=seeds, h=7)[0])


def test_embed_names_the_images_without_a_solution():
    cover = _dev(np.stack([stc_np.image_case((8, 16), w)[0] for w in ("a", "b", "a")]))
    rho = torch.ones((3, 8, 16), dtype=torch.float64, device=DEV)
    rho[0] = float("inf")
    rho[2] = float("inf")
    with pytest.raises(ValueError, match=r"image\(s\) \[0, 2\]"):
        stc.embed(cover, 0.4, seeds=[1, 2, 3], rho=rho, h=7)
    stego, changes, cost, ok = stc.embed(cover, 0.4, seeds=[1, 2, 3], rho=rho, h=7, strict=False)
    assert ok.tolist() == [False, True, False] and torch.equal(stego[0], cover[0]) and changes.tolist()[0] == 0


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------

@fabrika.stego_spatial(iterator=None, convert_to=None, ignore_missing=False)
def _stego_rows(df, **kw):
    return df


def test_write_dataset_and_cli(tmp_path, capsys):
    data = tmp_path / "data"
    (data / "images").mkdir(parents=True)
    covers = (6, 7)
    for c in covers:
        shutil.copy(GOLDEN / f"cover_{c}.png", data / "images" / f"{c}.png")
    (data / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{c}.png,512,512\n" for c in covers))
    x = torch.from_numpy(read_luma_batch([data / "images" / f"{c}.png" for c in covers])).to(DEV)
    seeds = [embed.image_seed(f"{c}.png", 2) for c in covers]
    # random bits at one alpha, h = 7
    folders = stc.write_dataset(data, "stcm", 0.1, h=7, stream=2)
    assert folders == [data / "stego_STCM_alpha_0.1_independent_images"]
    assert (folders[0] / "files.csv").read_text().splitlines() == ["name,height,width,stego_method,alpha"] + [
        f"stego_STCM_alpha_0.1_independent_images/{c}.png,512,512,STCM,0.1" for c in covers]
    rows = _stego_rows(data, stego_method="STCM", alpha=0.1)
    assert [str(v) for v in rows["name"]] == [str(folders[0] / f"{c}.png") for c in covers]
    files = torch.from_numpy(read_luma_batch([folders[0] / f"{c}.png" for c in covers])).to(DEV)
    assert torch.equal(files, stc.embed(x, 0.1, seeds=seeds, change="pm1", h=7)[0])
    k = int(round(0.1 * 512 * 512))
    assert torch.equal(stc.extract(files, k, seeds=seeds, h=7), stc.random_message(seeds, k, DEV))
    # a message file through both CLI commands, h = 10
    text = bytes(range(256)) * 2 + b"a message that is really carried"
    (tmp_path / "message.bin").write_bytes(text)
    alpha = 8 * len(text) / (512 * 512)
    stc.main(["embed", "--data", str(data), "--stego-method", "STCR", "--message", str(tmp_path / "message.bin"), "--stream", "2"])
    folder = data / stc.folder_name("STCR", alpha)
    assert capsys.readouterr().out.split() == [str(folder)]
    assert (folder / "files.csv").read_text().splitlines()[1] == f"{folder.name}/6.png,512,512,STCR,{alpha}"
    files = read_luma_batch([folder / f"{c}.png" for c in covers])
    d = files.astype(np.int64) - x.cpu().numpy()
    assert np.abs(d).max() == 1 and ((files ^ x.cpu().numpy()) <= 1).all() and 0 < np.count_nonzero(d) < 8 * len(text)
    stc.main(["extract", "--data", str(data), "--stego-method", "stcr", "--alpha", repr(alpha), "--bits", str(8 * len(text)), "--stream", "2",
              "--out", str(tmp_path / "read")])
    assert capsys.readouterr().out.split() == [str(tmp_path / "read" / f"{c}.bin") for c in covers]
    for c in covers:
        assert (tmp_path / "read" / f"{c}.bin").read_bytes() == text
    # the wrong stream is the wrong key
    stc.main(["extract", "--data", str(data), "--stego-method", "stcr", "--alpha", repr(alpha), "--bits", str(8 * len(text)), "--stream", "1",
              "--out", str(tmp_path / "wrong")])
    assert (tmp_path / "wrong" / "6.bin").read_bytes() != text
    # the WS table driver reads the new folder by its name, unchanged
    from ws_unet_amd.ws import estimate
    res = estimate.run(data, "STCM", 0.1, "KB", None, (3,), batched=True, batch_size=2)
    assert res["name"].tolist() == [f"stego_STCM_alpha_0.1_independent_images/{c}.png" for c in covers] and np.isfinite(res["beta_hat"]).all()
