"""GPU: the +-1 simulators (K37-K39, ops.ternary_entropy / ternary_lambda / embed_ternary / embed_lsbm, ws_unet_amd.embed_pm1) against
the numpy restatement (pm1_np) on its shared inputs: the entropy to the rounding of a reordered sum, the draws bit for bit (the CPU test
test_pm1_host asserts that no draw of these cases lies near a threshold), the multiplier search through the restatement's entropy, and
the drivers (`write_dataset`, the CLI, `spam.extract(simulate=True)`)."""
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV, check_span_placements
import pm1_np
import spam_np
from ws_unet_amd import embed, embed_pm1, fabrika, ops, spam
from ws_unet_amd.imread import read_luma_batch

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
INPUTS = [(c, s) for s in pm1_np.SHAPES for c in pm1_np.CONTENTS]
SHORT = {("ends", (70, 90), 1.0), ("ends", (65, 130), 1.0)}                 # as test_pm1_host pins them on the CPU


def _tol(shape):
    """Relative: every term is >= 0, so a reordered sum of n terms moves by at most n - 1 units in the last place; the terms' own
    functions (exp, log2, the division) add a few more."""
    return (shape[0] * shape[1] + 64) * 2.0 ** -52


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.tensor(a, dtype=dtype, device=DEV)


def _lambdas16(content, shape):
    """16 multipliers from a quarter of the smallest to four times the largest the three payloads need"""
    los = [pm1_np.case_lambda(content, shape, a)[0] for a in pm1_np.ALPHAS]
    lo, hi = min(los) / 4, max(los) * 4
    return lo * (hi / lo) ** (np.arange(16) / 15.0)


def _close(got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print(f"max relative difference {np.max(np.abs(got - want) / np.maximum(want, 1e-300)):.3e} (tolerance {tol:.3e})")
    return bool(np.all(np.abs(got - want) <= tol * want))


# ---- K37 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("content,shape", INPUTS)
def test_entropy_equals_the_restatement(content, shape):
    """the image between two others of its shape, 16 multipliers each; again (same bits); alone (same bits); one multiplier (same bits);
    with every 7th cost +inf"""
    names = ("noise", content, "flat")
    xs, rhos = zip(*(pm1_np.case(c, shape) for c in names))
    lams = np.stack([_lambdas16(c, shape) for c in names])
    x, rho, lam = _dev(np.stack(xs)), _dev(np.stack(rhos)), _dev(lams)
    got = ops.ternary_entropy(x, rho, lam)
    assert got.shape == (3, 16) and got.dtype == torch.float64
    want = [pm1_np.entropy(xs[1], rhos[1], v) for v in lams[1]]
    assert want[0] > want[-1] >= 0
    assert _close(got[1].cpu().numpy(), want, _tol(shape))
    assert torch.equal(ops.ternary_entropy(x, rho, lam), got)
    assert torch.equal(ops.ternary_entropy(x[1:2], rho[1:2], lam[1:2]), got[1:2])
    assert torch.equal(ops.ternary_entropy(x, rho, lam[:, 5:6].contiguous()), got[:, 5:6])
    wet = np.array(rhos[1])
    wet.reshape(-1)[::7] = np.inf
    got = ops.ternary_entropy(x[1:2], _dev(wet[None]), lam[1:2])
    assert _close(got[0].cpu().numpy(), [pm1_np.entropy(xs[1], wet, v) for v in lams[1]], _tol(shape))


def test_entropy_argument_errors():
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    rho = torch.ones((2, 8, 8), dtype=torch.float64, device=DEV)
    for lam in (torch.ones((2, 17), dtype=torch.float64, device=DEV), torch.ones((2, 0), dtype=torch.float64, device=DEV),
                torch.ones((3, 4), dtype=torch.float64, device=DEV), torch.ones((2, 4), dtype=torch.float32, device=DEV),
                torch.ones(2, dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError, match="lambdas must be"):
            ops.ternary_entropy(x, rho, lam)
    lam = torch.ones((2, 4), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="rho must be"):
        ops.ternary_entropy(x, rho.float(), lam)
    with pytest.raises(ValueError, match="rho must be"):
        ops.ternary_entropy(x, rho[:1], lam)
    with pytest.raises(Exception, match="contiguous"):
        ops.ternary_entropy(x, rho, torch.ones((2, 8), dtype=torch.float64, device=DEV)[:, ::2])
    with pytest.raises(ValueError, match="message_bits must be"):
        ops.ternary_lambda(x, rho, torch.ones(3, dtype=torch.float64, device=DEV))


# ---- K38, K39 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("content,shape", INPUTS)
def test_draws_equal_the_restatement_bit_for_bit(content, shape):
    """one batch holds the image three times, once per payload, under the seed of the CPU test; the multipliers come from the restatement,
    so nothing here depends on the device search.  Also: the counts, an image alone, and stego written over the cover."""
    x, rho = pm1_np.case(content, shape)
    n = len(pm1_np.ALPHAS)
    lams = [pm1_np.case_lambda(content, shape, a)[0] for a in pm1_np.ALPHAS]
    cover, cost = _dev(np.stack([x] * n)), _dev(np.stack([rho] * n))
    seeds = _dev([pm1_np.SEED] * n, torch.int64)
    lam = _dev(lams, torch.float64)
    thr = _dev([pm1_np.lsbm_threshold(a) for a in pm1_np.ALPHAS], torch.int32)
    lib = ops._lib.load()
    for name, run, raw, want in (
            ("HILL", lambda s: ops.embed_ternary(cover[s], cost[s], lam[s], seeds[s]),
             lambda buf, ch: lib.wsu_embed_ternary(buf.data_ptr(), cost.data_ptr(), lam.data_ptr(), seeds.data_ptr(), buf.data_ptr(), ch.data_ptr(),
                                                   n, shape[0], shape[1], ops._stream()),
             [pm1_np.ternary_np(x, rho, v, pm1_np.SEED) for v in lams]),
            ("LSBM", lambda s: ops.embed_lsbm(cover[s], seeds[s], thr[s]),
             lambda buf, ch: lib.wsu_embed_lsbm(buf.data_ptr(), seeds.data_ptr(), thr.data_ptr(), buf.data_ptr(), ch.data_ptr(),
                                                n, shape[0], shape[1], ops._stream()),
             [pm1_np.lsbm_np(x, a, pm1_np.SEED) for a in pm1_np.ALPHAS])):
        stego, changes = run(slice(None))
        assert stego.dtype == torch.uint8 and changes.dtype == torch.int64 and torch.equal(cover, _dev(np.stack([x] * n))), name
        for i in range(n):
            np.testing.assert_array_equal(stego[i].cpu().numpy().astype(np.int64), want[i][0], err_msg=f"{name} alpha {pm1_np.ALPHAS[i]}")
        assert changes.tolist() == [w[1] for w in want], name
        assert changes.tolist() == (stego != cover).sum(dim=(1, 2)).tolist(), name
        alone = run(slice(1, 2))                                              # the second image starts off the 16-byte grid where H*W % 16 != 0
        assert torch.equal(alone[0][0], stego[1]) and alone[1].tolist() == changes[1:2].tolist(), name
        buf, ch = cover.clone(), torch.full((n,), 7, dtype=torch.int64, device=DEV)
        ops.check(raw(buf, ch), name)
        assert torch.equal(buf, stego) and torch.equal(ch, changes), name
    assert torch.equal(ops.embed_lsbm(cover, seeds, torch.zeros_like(thr))[0], cover)
    assert torch.equal(ops.embed_ternary(cover, cost, torch.full_like(lam, float("inf")), seeds)[0], cover)


def test_draws_where_the_plane_is_short_or_cover_and_stego_differ_in_alignment():
    """The shapes above reach the pixel loop's paths (a), (b) (70 x 90) and (c) (65 x 130); (d) and (e) need a plane placed by hand."""
    lib = ops._lib.load()
    seeds, lam = _dev([pm1_np.SEED], torch.int64), _dev([0.7], torch.float64)
    thr = _dev([pm1_np.lsbm_threshold(0.4)], torch.int32)

    def cost(h, w):                                                           # positive, finite, different from pixel to pixel
        return 0.25 + (np.arange(h * w, dtype=np.float64) % 5).reshape(h, w)

    costs = []                                                                # (alive until the test ends)

    def hill(ci, co, ch, h, w):
        costs.append(_dev(cost(h, w)[None]))
        return lib.wsu_embed_ternary(ci, costs[-1].data_ptr(), lam.data_ptr(), seeds.data_ptr(), co, ch, 1, h, w, ops._stream())

    def hill_np(p):
        assert pm1_np.min_gap(p, *pm1_np.ternary_thresholds(p, cost(*p.shape), 0.7), pm1_np.SEED) > 64      # no draw hangs on exp's last bits
        return pm1_np.ternary_np(p, cost(*p.shape), 0.7, pm1_np.SEED)[0]

    check_span_placements("de", hill, hill_np)
    check_span_placements("de", lambda ci, co, ch, h, w: lib.wsu_embed_lsbm(ci, seeds.data_ptr(), thr.data_ptr(), co, ch, 1, h, w, ops._stream()),
                          lambda p: pm1_np.lsbm_np(p, 0.4, pm1_np.SEED)[0])


def test_draws_depend_on_the_seed_alone():
    x, rho = pm1_np.case("photo", (70, 90))
    cover, cost = _dev(np.stack([x] * 2)), _dev(np.stack([rho] * 2))
    lam = _dev([6.0, 6.0], torch.float64)
    a, _ = ops.embed_ternary(cover, cost, lam, _dev([5, 5 | (1 << 32)], torch.int64))
    b, _ = ops.embed_ternary(cover, cost, lam, _dev([5 | (1 << 32), 5], torch.int64))
    assert torch.equal(a[0], b[1]) and torch.equal(a[1], b[0]) and not torch.equal(a[0], a[1])


# ---- the search ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("content,shape", INPUTS)
def test_lambda_search(content, shape):
    """H(lam_lo) >= m >= H(lam_hi) through the restatement's entropy, to the tolerance of K37; the bracket's width; `ok`"""
    x, rho = pm1_np.case(content, shape)
    n, tol = len(pm1_np.ALPHAS), _tol(shape)
    m = np.array([a * x.size for a in pm1_np.ALPHAS])
    lo, hi, ok = ops.ternary_lambda(_dev(np.stack([x] * n)), _dev(np.stack([rho] * n)), _dev(m))
    assert lo.shape == hi.shape == ok.shape == (n,) and lo.dtype == torch.float64 and ok.dtype == torch.bool
    lo, hi, ok = lo.cpu().numpy(), hi.cpu().numpy(), ok.cpu().numpy()
    for i, a in enumerate(pm1_np.ALPHAS):
        h_lo, h_hi = pm1_np.entropy(x, rho, lo[i]), pm1_np.entropy(x, rho, hi[i])
        print(f"alpha {a}: lam_lo {lo[i]:.17g} lam_hi / lam_lo - 1 {hi[i] / lo[i] - 1:.3e} H(lo) - m {h_lo - m[i]:.3e} H(hi) - m {h_hi - m[i]:.3e} ok {ok[i]}")
        assert bool(ok[i]) == ((content, shape, a) not in SHORT)
        assert 0 <= hi[i] / lo[i] - 1 <= 2.0 ** -29
        assert h_hi <= m[i] * (1 + tol)
        if ok[i]:
            assert h_lo >= m[i] * (1 - tol)
        else:
            assert lo[i] == hi[i] == ops.TERNARY_LADDER[0] == pm1_np.LADDER[0]
    assert tuple(ops.TERNARY_LADDER) == tuple(pm1_np.LADDER) and ops.TERNARY_REFINEMENTS == pm1_np.REFINEMENTS


# ---- simulate ---------------------------------------------------------------------------------------------------------------------------------

def test_simulate_hill_and_lsbm():
    shape = (64, 64)
    names, alphas = ("noise", "photo", "flat", "ends"), [0.01, 0.4, 1.0, 0.0]
    xs, rhos = zip(*(pm1_np.case(c, shape) for c in names))
    cover = _dev(np.stack(xs))
    seeds = [11, 12, 13, 14]
    stego, changes = embed_pm1.simulate(cover, "hill", alphas, seeds)
    again, _ = embed_pm1.simulate(cover, "HILL", alphas, torch.tensor(seeds), rho=ops.hill_cost_f64(cover))
    assert torch.equal(stego, again)
    assert torch.equal(stego[3], cover[3]) and changes[3].item() == 0          # no payload: the cover
    lam, _, ok = ops.ternary_lambda(cover, _dev(np.stack(rhos)), _dev(np.array(alphas) * 4096.0))
    assert ok.all()
    want = ops.embed_ternary(cover, _dev(np.stack(rhos)), torch.where(_dev(alphas, torch.float64) > 0, lam, torch.full_like(lam, float("inf"))),
                             _dev(seeds, torch.int64))
    assert torch.equal(stego, want[0]) and torch.equal(changes, want[1])      # simulate is the cost, the search and the draw
    d = stego.cpu().numpy().astype(np.int64) - np.stack(xs)
    assert np.abs(d).max() == 1 and changes.tolist() == np.count_nonzero(d, axis=(1, 2)).tolist()
    for i in range(3):
        q = sum(pm1_np.probabilities(xs[i], rhos[i], lam[i].item()))
        assert abs(changes[i].item() - q.sum()) <= 5 * np.sqrt((q * (1 - q)).sum()) + 1
    stego, changes = embed_pm1.simulate(cover, "LSBM", alphas, seeds)
    for i in range(4):
        want = pm1_np.lsbm_np(xs[i], alphas[i], seeds[i])
        np.testing.assert_array_equal(stego[i].cpu().numpy().astype(np.int64), want[0])
        assert changes[i].item() == want[1]
    # a payload beyond the capacity names its images
    x = _dev(np.stack([pm1_np.case("ends", (70, 90))[0]] * 3))
    with pytest.raises(ValueError, match=r"image\(s\) \[0, 2\]"):
        embed_pm1.simulate(x, "HILL", [1.0, 0.4, 1.2], [1, 2, 3])


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------

@fabrika.stego_spatial(iterator=None, convert_to=None, ignore_missing=False)
def _stego_rows(df, **kw):
    return df


ORDER = (10, 6, 7, 8, 9)                                                    # fabrika sorts names lexically


def test_write_dataset_cli_and_spam(tmp_path, capsys):
    data = tmp_path / "data"
    (data / "images").mkdir(parents=True)
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", data / "images" / f"{k}.png")
    (data / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    folders = embed_pm1.write_dataset(data, "LSBM", 0.4, stream=2)
    embed_pm1.main(["--data", str(data), "--stego-method", "hill", "--alphas", ".4", ".2", "--stream", "2"])
    assert capsys.readouterr().out.split() == [str(data / f"stego_HILL_alpha_{a}_independent_images") for a in (0.4, 0.2)]
    assert folders == [data / "stego_LSBM_alpha_0.4_independent_images"]
    covers = read_luma_batch([data / "images" / f"{k}.png" for k in ORDER])
    x = torch.from_numpy(covers).to(DEV)
    seeds = [embed.image_seed(f"{k}.png", 2) for k in ORDER]
    for m, a in (("LSBM", 0.4), ("HILL", 0.4), ("HILL", 0.2)):
        folder = embed_pm1.folder_name(m, a)
        assert (data / folder / "files.csv").read_text().splitlines()[:2] == ["name,height,width,stego_method,alpha", f"{folder}/10.png,512,512,{m},{a}"]
        rows = _stego_rows(data, stego_method=m, alpha=a)
        assert [str(n) for n in rows["name"]] == [str(data / folder / f"{k}.png") for k in ORDER]
        files = read_luma_batch([data / folder / f"{k}.png" for k in ORDER])
        twins, changes = embed_pm1.simulate(x, m, a, seeds)
        assert (files == twins.cpu().numpy()).all()
        d = files.astype(np.int64) - covers
        assert np.abs(d).max() == 1 and changes.tolist() == np.count_nonzero(d, axis=(1, 2)).tolist() and (changes > 1000).all()
        # the detector's features of the simulated twins are those of the files
        rows, F = spam.extract(data, m, a, simulate=True, stream=2, batch_size=3)
        assert rows["name"].tolist() == [f"{folder}/{k}.png" for k in ORDER] and (rows["stego_method"] == m).all() and (rows["alpha"] == a).all()
        np.testing.assert_array_equal(F, spam.extract(data, m, a)[1])
        if m == "LSBM":
            np.testing.assert_array_equal(F, spam_np.features(spam_np.counts(files)))
    # the LSB-replacement route is what it was
    rows, F = spam.extract(data, "LSBR", 0.4, simulate=True, stream=3, batch_size=3)
    twins = embed.simulate(x, "LSBR", 0.4, [embed.image_seed(f"{k}.png", 3) for k in ORDER])[0]
    assert rows["name"].tolist() == [f"{embed.folder_name('LSBR', 0.4)}/{k}.png" for k in ORDER]
    np.testing.assert_array_equal(F, spam.features(ops.spam_counts(twins)))
    with pytest.raises(ValueError, match="LSBR / HILLR / LSBM / HILL"):
        spam.extract(data, "LSBRS", 0.4, simulate=True)
