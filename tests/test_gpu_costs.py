"""GPU: the wavelet cost kernel (K48, ops.wavelet_cost_f64) against the numpy restatement (costs_np), bit for bit as uint64 patterns, on
its shapes and contents, at every placement of the planes and with a sigma and clamps of its own; then ws_unet_amd.costs: the simulated
sender against embed_pm1's and pm1_np's, the round trip of a real message, and the drivers (`write_dataset`, both CLI commands,
`fabrika.stego_spatial` and `spam.extract` on the written folder)."""
import numpy as np
import pytest
import torch

from gpu_util import DEV
import costs_np
import pm1_np
from ws_unet_amd import costs, embed, embed_pm1, fabrika, ops, spam, stc
from ws_unet_amd.imread import read_luma_batch

pytestmark = pytest.mark.gpu

KINDS = ("suniward", "wow")
# costs_np.SHAPES: (3,5) and (8,16) fold several times; 32 = the tile, (33,33) one more in both directions; (80,96) is the smallest plane
# with a tile whose window is copied as 16-byte segments (rows of a multiple of 16 bytes, the tile (1,1) 15 away from every border)
SHAPES = costs_np.SHAPES + ((80, 96),)


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV) if dtype is None else torch.tensor(a, dtype=dtype, device=DEV)


def _same_bits(got: torch.Tensor, want: np.ndarray, what):
    g = got.cpu().numpy()
    assert g.dtype == np.float64 and g.shape == want.shape, what
    bad = np.nonzero(g.view(np.uint64) != want.view(np.uint64))
    assert bad[0].size == 0, (what, bad[0].size, [(int(i), int(j), g[i, j], want[i, j]) for i, j in zip(bad[0][:4], bad[1][:4])])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_k48_equals_the_restatement_bit_for_bit(kind, shape):
    """one batch holds the five contents; again (same bits); three of them, and the middle one alone"""
    cases = [costs_np.case(c, shape, kind) for c in costs_np.CONTENTS]
    x = _dev(np.stack([c[0] for c in cases]))
    rho = ops.wavelet_cost_f64(x, kind)
    assert rho.dtype == torch.float64 and rho.shape == x.shape
    for i, c in enumerate(costs_np.CONTENTS):
        _same_bits(rho[i], cases[i][1], (kind, shape, c))
    clamp = costs_np.CLAMPS[kind]
    assert bool((rho > 0).all()) and bool((rho <= clamp).all())
    assert bool((rho[2] == (clamp if kind == "wow" else rho[2, 0, 0])).all())               # flat
    assert torch.equal(ops.wavelet_cost_f64(x, kind), rho)
    assert torch.equal(ops.wavelet_cost_f64(x[1:4].contiguous(), kind), rho[1:4])
    assert torch.equal(ops.wavelet_cost_f64(x[2:3].contiguous(), kind), rho[2:3])
    assert torch.equal(ops.wavelet_cost_f64(x[1:2].contiguous(), kind)[0], rho[1])


@pytest.mark.parametrize("kind", KINDS)
def test_k48_sigma_and_clamp(kind):
    shape = (33, 31)
    x = costs_np.plane("photo", *shape)
    for sigma, clamp in ((0.25, None), (1.0, 5.0 if kind == "suniward" else 0.3), (3.0, 1e-3)):
        want = costs_np.cost(x, kind, sigma=sigma, clamp=clamp)
        if clamp is not None:
            assert (want == clamp).any() and (clamp == 1e-3 or (want < clamp).any())         # the clamp bites, and not everywhere
        _same_bits(ops.wavelet_cost_f64(_dev(x[None]), kind, sigma=sigma, clamp=clamp)[0], want, (kind, sigma, clamp))
    if kind == "wow":                                                                         # sigma is not read
        assert torch.equal(ops.wavelet_cost_f64(_dev(x[None]), kind, sigma=7.0), ops.wavelet_cost_f64(_dev(x[None]), kind))
    low = 2.0 if kind == "suniward" else 0.25
    assert costs.cost_map(_dev(x[None]), kind.upper(), clamp=low).max().item() == low
    assert torch.equal(costs.cost_map(_dev(x[None]), "hill"), ops.hill_cost_f64(_dev(x[None])))


@pytest.mark.parametrize("kind", KINDS)
def test_k48_at_every_placement_of_its_planes(kind):
    """The window is copied as 16-byte segments only from a 16-byte aligned cover; the cost plane is written as single float64 values.
    A cover at an odd byte offset and a cost plane at an 8-byte but not 16-byte offset give the bits of the aligned call, and no byte
    outside the plane is written."""
    lib = ops._lib.load()
    h, w = 80, 96
    x, want = costs_np.case("noise", (h, w), kind)
    for off_in, off_out in ((0, 0), (1, 0), (0, 1), (3, 1), (16, 2)):
        buf_in = torch.zeros(h * w + 32, dtype=torch.uint8, device=DEV)
        buf_out = torch.full((h * w + 4,), -7.0, dtype=torch.float64, device=DEV)
        assert buf_in.data_ptr() % 16 == 0 and buf_out.data_ptr() % 16 == 0
        cin, cout = buf_in[off_in:off_in + h * w], buf_out[off_out:off_out + h * w]
        cin.copy_(_dev(x.reshape(-1)))
        ops.check(lib.wsu_wavelet_cost_f64(cin.data_ptr(), cout.data_ptr(), ops.WAVELET_COST_KINDS[kind], 1.0, costs_np.CLAMPS[kind], 1, h, w,
                                           ops._stream()), f"{kind} at {off_in} -> {off_out}")
        _same_bits(cout.reshape(h, w), want, (kind, off_in, off_out))
        rest = torch.cat([buf_out[:off_out], buf_out[off_out + h * w:]])
        assert bool((rest == -7.0).all()) and np.array_equal(cin.cpu().numpy(), x.reshape(-1))


def test_k48_argument_errors():
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="kind must be"):
        ops.wavelet_cost_f64(x, "hill")
    with pytest.raises(ValueError, match="uint8"):
        ops.wavelet_cost_f64(x.float(), "wow")
    with pytest.raises(ValueError, match="uint8"):
        ops.wavelet_cost_f64(x[0], "wow")
    with pytest.raises(Exception, match="sigma"):
        ops.wavelet_cost_f64(x, "suniward", sigma=0.0)
    with pytest.raises(Exception, match="clamp"):
        ops.wavelet_cost_f64(x, "wow", clamp=float("inf"))
    with pytest.raises(Exception, match="contiguous"):
        ops.wavelet_cost_f64(torch.zeros((2, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2], "wow")


# ---- the simulated sender ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", costs.SIMULATED)
def test_simulate_is_the_ternary_sender_over_the_cost(method):
    shape = (64, 64)
    names, alphas, seeds = ("noise", "photo", "stripes", "ends"), [0.01, 0.4, 1.0, 0.0], [11, 12, 13, 14]
    xs = [costs_np.plane(c, *shape) for c in names]
    rhos = [costs_np.cost(x, method.lower()) for x in xs]
    cover = _dev(np.stack(xs))
    rho = costs.cost_map(cover, method)
    for i in range(4):
        _same_bits(rho[i], rhos[i], (method, names[i]))
    stego, changes = costs.simulate(cover, method.lower(), alphas, seeds)
    assert stego.dtype == torch.uint8 and changes.dtype == torch.int64
    for again in (costs.simulate(cover, method, alphas, torch.tensor(seeds), rho=rho), embed_pm1.simulate(cover, "HILL", alphas, seeds, rho=rho)):
        assert torch.equal(stego, again[0]) and torch.equal(changes, again[1])
    assert torch.equal(stego[3], cover[3]) and changes[3].item() == 0          # no payload: the cover
    assert not torch.equal(stego[:3], embed_pm1.simulate(cover, "HILL", alphas, seeds)[0][:3])          # (another cost, other twins)
    # pm1_np's sender fed the restated cost, under the device's multiplier (no draw may hang on exp's last bits)
    lam, _, ok = ops.ternary_lambda(cover, rho, _dev(np.array(alphas) * 4096.0))
    assert ok.all()
    for i in range(3):
        lam_i = lam[i].item()
        lo, hi, fits = pm1_np.ternary_lambda(xs[i], rhos[i], alphas[i] * 4096.0)
        assert fits and abs(lam_i / lo - 1) <= 2.0 ** -28, (lam_i, lo, hi)
        assert pm1_np.min_gap(xs[i], *pm1_np.ternary_thresholds(xs[i], rhos[i], lam_i), seeds[i]) > 64
        want, count = pm1_np.ternary_np(xs[i], rhos[i], lam_i, seeds[i])
        np.testing.assert_array_equal(stego[i].cpu().numpy().astype(np.int64), want, err_msg=f"{method} {names[i]}")
        assert changes[i].item() == count and (count > 0 or i == 0)                  # (41 bits may cost no change at all)
    d = stego.cpu().numpy().astype(np.int64) - np.stack(xs)
    assert np.abs(d).max() == 1 and changes.tolist() == np.count_nonzero(d, axis=(1, 2)).tolist()


def test_simulate_capacity_and_method_errors():
    ends = _dev(np.stack([costs_np.plane("ends", 33, 31)] * 3))
    with pytest.raises(ValueError, match=r"'WOW' cannot carry the payload in image\(s\) \[0, 2\]"):
        costs.simulate(ends, "WOW", [1.2, 0.4, 1.3], [1, 2, 3])              # a pixel at 0 or 255 holds one bit
    with pytest.raises(ValueError, match=r"alpha outside \[0, log2 3\) for 'SUNIWARD'"):
        costs.simulate(ends, "SUNIWARD", 1.585, [1, 2, 3])
    with pytest.raises(NotImplementedError, match="use embed"):
        costs.simulate(ends, "WOWT", 0.4, [1, 2, 3])
    with pytest.raises(NotImplementedError, match="use simulate"):
        costs.embed(ends, "WOW", 0.4, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="needs one seed per image"):
        costs.simulate(ends, "WOW", 0.4, None)


# ---- a real message -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", (0.4, 0.1))
@pytest.mark.parametrize("method", ("SUNIWARDT", "WOWT"))
def test_embed_and_extract_round_trip(method, alpha):
    shape, h = (64, 64), 7
    xs = [costs_np.plane(c, *shape) for c in ("noise", "photo")]
    cover = _dev(np.stack(xs))
    seeds = [embed.image_seed(f"{i}.png", 3) for i in range(2)]
    rho = costs.cost_map(cover, costs.method_cost(method))
    stego, changes, dist, ok, layers = costs.embed(cover, method.lower(), alpha, h=h, seeds=seeds)
    k = int(round(alpha * 4096))
    assert ok.all() and (layers.sum(dim=1) == k).all()
    want = stc.random_message(seeds, k, DEV)
    read, ks = costs.extract(stego, layers, h=h, seeds=seeds)
    assert torch.equal(read, want) and ks.tolist() == [k, k]
    d = stego.cpu().numpy().astype(np.int64) - np.stack(xs)
    assert set(np.unique(d)) <= {-1, 0, 1} and changes.tolist() == np.count_nonzero(d, axis=(1, 2)).tolist() and (changes > 0).all()
    paid = torch.where(stego != cover, rho, torch.zeros_like(rho)).sum(dim=(1, 2))
    assert torch.allclose(paid, dist, rtol=1e-12, atol=0)
    given = costs.embed(cover, method, want.cpu(), h=h, seeds=seeds, rho=rho)
    assert all(torch.equal(a, b) for a, b in zip(given, (stego, changes, dist, ok, layers)))
    assert not torch.equal(costs.extract(stego, layers, h=h, seeds=[seeds[0] + 1, seeds[1]])[0][0], want[0])


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------

@fabrika.stego_spatial(iterator=None, convert_to=None, ignore_missing=False)
def _stego_rows(df, **kw):
    return df


def test_write_dataset_cli_and_the_readers(tmp_path, capsys):
    from PIL import Image
    hh, ww = 96, 80
    data = tmp_path / "data"
    (data / "images").mkdir(parents=True)
    big = costs_np.golden_cover(6)
    crops = {"3": big[:hh, :ww], "4": big[200:200 + hh, 300:300 + ww]}
    for name, c in crops.items():
        Image.fromarray(np.ascontiguousarray(c)).save(data / "images" / f"{name}.png")
    (data / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{n}.png,{hh},{ww}\n" for n in crops))
    x = torch.from_numpy(read_luma_batch([data / "images" / f"{n}.png" for n in crops])).to(DEV)
    assert np.array_equal(x.cpu().numpy(), np.stack(list(crops.values())))
    seeds = [embed.image_seed(f"{n}.png", 2) for n in crops]
    # the simulated sender, through write_dataset and through the CLI
    folders = costs.write_dataset(data, "suniward", [0.4, 0.2], stream=2, sigma=0.5)
    assert folders == [data / f"stego_SUNIWARD_alpha_{a}_independent_images" for a in (0.4, 0.2)]
    costs.main(["embed", "--data", str(data), "--stego-method", "wow", "--alphas", ".4", "--stream", "2"])
    assert capsys.readouterr().out.split() == [str(data / "stego_WOW_alpha_0.4_independent_images")]
    for m, a, params in (("SUNIWARD", 0.4, {"sigma": 0.5}), ("SUNIWARD", 0.2, {"sigma": 0.5}), ("WOW", 0.4, {})):
        folder = costs.folder_name(m, a)
        assert (data / folder / "files.csv").read_text().splitlines() == ["name,height,width,stego_method,alpha"] + [
            f"{folder}/{n}.png,{hh},{ww},{m},{a}" for n in crops]
        files = read_luma_batch([data / folder / f"{n}.png" for n in crops])
        twins, changes = costs.simulate(x, m, a, seeds, **params)
        assert (files == twins.cpu().numpy()).all() and (changes > 100).all()
        rows = _stego_rows(data, stego_method=m, alpha=a)
        assert [str(v) for v in rows["name"]] == [str(data / folder / f"{n}.png") for n in crops]
    assert not torch.equal(costs.simulate(x, "SUNIWARD", 0.4, seeds)[0], costs.simulate(x, "SUNIWARD", 0.4, seeds, sigma=0.5)[0])
    # a message file through both CLI commands, h = 10
    text = b"sixty bytes that S-UNIWARD and WOW carry in two layers, each"
    assert len(text) == 60
    (tmp_path / "message.bin").write_bytes(text)
    alpha = 8 * len(text) / (hh * ww)
    for m in ("SUNIWARDT", "WOWT"):
        costs.main(["embed", "--data", str(data), "--stego-method", m.lower(), "--message", str(tmp_path / "message.bin"), "--stream", "2"])
        folder = data / costs.folder_name(m, alpha)
        assert capsys.readouterr().out.split() == [str(folder)]
        table = (folder / "files.csv").read_text().splitlines()
        assert table[0] == "name,height,width,stego_method,alpha,bits_high,bits_low" and len(table) == 3
        assert all(sum(int(v) for v in ln.split(",")[5:]) == 8 * len(text) and ln.split(",")[3] == m for ln in table[1:])
        files = read_luma_batch([folder / f"{n}.png" for n in crops])
        d = files.astype(np.int64) - x.cpu().numpy()
        assert np.abs(d).max() == 1 and 0 < np.count_nonzero(d) < 8 * len(text)
        costs.main(["extract", "--data", str(data), "--stego-method", m, "--alpha", repr(alpha), "--stream", "2", "--out", str(tmp_path / m)])
        assert capsys.readouterr().out.split() == [str(tmp_path / m / f"{n}.bin") for n in crops]
        for n in crops:
            assert (tmp_path / m / f"{n}.bin").read_bytes() == text
    # write_dataset's own message path equals the CLI's files; another stream does not read them
    again = costs.write_dataset(data, "WOWT", message=text, stream=2)
    assert again == [data / costs.folder_name("WOWT", alpha)]
    assert (read_luma_batch([again[0] / f"{n}.png" for n in crops]) == files).all()
    wrong = costs.extract_dataset(data, "WOWT", alpha, tmp_path / "wrong", stream=1)
    assert wrong[0].read_bytes() != text
    # the loaders and the SPAM detector read the new folder from its files
    rows = _stego_rows(data, stego_method="WOWT", alpha=alpha)
    assert [str(v) for v in rows["name"]] == [str(again[0] / f"{n}.png") for n in crops]
    rows, F = spam.extract(data, "WOWT", alpha)
    assert rows["name"].tolist() == [f"{again[0].name}/{n}.png" for n in crops] and (rows["stego_method"] == "WOWT").all()
    np.testing.assert_array_equal(F, spam.features(ops.spam_counts(torch.from_numpy(files).to(DEV))))
