"""GPU: the sequential-payload WS changepoint (K27) and the sequential simulator LSBRS (K28) against numpy (sequential_np, embed_np), equal
as integers / bit for bit; K27's consistency with K11; both ends together on the golden covers; placement='sequential' through the
drivers of ws.estimate and ws.roc."""
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV, DEFAULT_MODE, check_span_placements, gpu_model
import embed_np
import sequential_np
from ws_unet_amd import embed, filters, ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.unet_run import unet_plane
from ws_unet_amd.ws import estimate, roc, sequential

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
ORDERS = ("rows", "rows_up")
KB = np.asarray(filters.NAMED_FILTERS_2D["KB"])[..., 0]
AVG = np.asarray(filters.NAMED_FILTERS_2D["AVG"])[..., 0]
ONE = 1 << 24
SHAPES = [(1, 3, 3), (1, 3, 4), (2, 4, 3), (1, 5, 258), (1, 5, 259), (1, 67, 259), (2, 131, 40), (3, 16, 300), (1, 300, 5)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _got(x, x_hat=None, **kw):
    """ops.ws_sequential with the curve, as numpy: (k (N,), t_max (N,), t_all (N,), curve (N,H-2))"""
    out = ops.ws_sequential(_dev(x), None if x_hat is None else _dev(x_hat), mean_filter=AVG, return_curve=True, **kw)
    assert all(t.dtype == torch.int64 and t.is_cuda for t in out)
    assert out[3].shape == (x.shape[0], x.shape[1] - 2) and all(t.shape == (x.shape[0],) for t in out[:3])
    return [t.cpu().numpy() for t in out]


def _want(x, order, weighted, x_hat=None, hat_scale=255., pixel_kernels=None):
    per = [sequential_np.ws_sequential_np(x[i], order, x_hat=None if x_hat is None else x_hat[i], hat_scale=hat_scale,
                                          pixel_kernel=None if pixel_kernels is None else pixel_kernels[i], mean_kernel=AVG, weighted=weighted)
           for i in range(x.shape[0])]
    return [np.array([p[j] for p in per]) for j in range(4)]


def _assert_equal(got, want, what):
    for name, g, w in zip(("k", "t_max", "t_all", "curve"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _hat_for_terms(x, t):
    """the interior-layout prediction (scale 1) under which the unweighted term of every interior pixel is exactly t (multiples of 1/4):
    s * (x - x_hat) - 1/4 = t"""
    xi = x[:, 1:-1, 1:-1]
    s = xi.astype(np.float32) - (xi ^ 1).astype(np.float32)
    return (xi.astype(np.float32) - s * (np.asarray(t, dtype=np.float32) + np.float32(0.25))).astype(np.float32)


# ---- K27 against the restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_changepoint_equals_numpy_as_integers(shape):
    """one interior pixel; two; two images of two rows; an interior row of exactly 256 and of 257 pixels; many rows of 257; more rows than a
    pass of the row kernel takes (4 x 64 = 256 > 129: one pass, 298: two) and than the finishing workgroup has threads"""
    n, h, w = shape
    rng = np.random.default_rng(sum(shape) * 7 + w)
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    x[0] = (x[0].astype(np.int32) // 8 + rng.integers(100, 110)).astype(np.uint8)      # a smooth image: positive and negative terms
    full = rng.random(shape, dtype=np.float32)
    inner = (rng.random((n, h - 2, w - 2), dtype=np.float32) * np.float32(255.0)).astype(np.float32)
    kernels = (rng.standard_normal((n, 3, 3)) * 0.3).astype(np.float32)
    for weighted in (0, 1):
        for order in ORDERS:
            kw = dict(weighted=weighted, order=order)
            _assert_equal(_got(x, pixel_filter=KB, **kw), _want(x, order, weighted, pixel_kernels=[KB] * n), f"KB {kw}")
            _assert_equal(_got(x, pixel_filter=kernels, **kw), _want(x, order, weighted, pixel_kernels=kernels), f"per-image filters {kw}")
            _assert_equal(_got(x, full, hat_scale=255., **kw), _want(x, order, weighted, x_hat=full, hat_scale=255.), f"full-frame x_hat {kw}")
            _assert_equal(_got(x, inner, hat_scale=1., **kw), _want(x, order, weighted, x_hat=inner, hat_scale=1.), f"interior x_hat {kw}")


@pytest.mark.parametrize("shape", [(1, 3, 3), (2, 4, 3), (1, 5, 259), (2, 131, 40), (1, 300, 5)])
def test_constant_plane_and_all_positive_terms(shape):
    n, h, w = shape
    m = (h - 2) * (w - 2)
    flat = np.full(shape, 77, dtype=np.uint8)
    for weighted in (0, 1):
        for order in ORDERS:
            # KB predicts a constant plane up to rounding: r ~ 0, every t ~ -wgt / 4 < 0 -> the empty prefix
            k, t_max, t_all, curve = _got(flat, pixel_filter=KB, weighted=weighted, order=order)
            _assert_equal((k, t_max, t_all, curve), _want(flat, order, weighted, pixel_kernels=[KB] * n), f"constant {weighted} {order}")
            assert (k == 0).all() and (t_max == 0).all() and (t_all < 0).all() and (np.diff(curve, axis=1) < 0).all()
    x = np.random.default_rng(11).integers(0, 256, shape, dtype=np.uint8)
    hat = _hat_for_terms(x, np.ones((n, h - 2, w - 2)))
    for order in ORDERS:
        k, t_max, t_all, curve = _got(x, hat, hat_scale=1., weighted=0, order=order)
        assert (k == m).all() and (t_max == m * ONE).all() and (t_all == m * ONE).all()
        np.testing.assert_array_equal(curve, np.broadcast_to(np.arange(1, h - 1) * (w - 2) * ONE, (n, h - 2)))


def _tie_case(shape, terms):
    """terms: {(interior row, interior column): t}, 0 elsewhere -> per order (got, want)"""
    x = np.random.default_rng(shape[2]).integers(0, 256, shape, dtype=np.uint8)
    t = np.zeros((1, shape[1] - 2, shape[2] - 2), dtype=np.float32)
    for (r, c), v in terms.items():
        t[0, r, c] = v
    hat = _hat_for_terms(x, t)
    out = {}
    for order in ORDERS:
        got, want = _got(x, hat, hat_scale=1., weighted=0, order=order), _want(x, order, 0, x_hat=hat, hat_scale=1.)
        _assert_equal(got, want, f"tie {shape} {terms} {order}")
        out[order] = [int(g[0]) for g in got[:3]]
    return out


def test_first_of_equal_maxima_wins():
    """t = +1, -1, +1 (T = 1, 0, .., 1): the maximum 1 is reached at k = 1 and again later -- in another 64-pixel step and another
    256-pixel chunk of the same row, or in another row"""
    for far in (70, 300, 597):
        out = _tie_case((1, 3, 600), {(0, 0): 1, (0, 1): -1, (0, far): 1})
        assert out["rows"] == [1, ONE, ONE] == out["rows_up"]                                  # one interior row: both orders are one path
    out = _tie_case((1, 5, 7), {(0, 0): 1, (0, 1): -1, (2, 0): 1})
    assert out["rows"] == [1, ONE, ONE]
    assert out["rows_up"] == [11, 2 * ONE, ONE]                                             # bottom-up: +1 at path position 1, then +1 -1 in the last row
    out = _tie_case((1, 300, 5), {(0, 0): 1, (0, 1): -1, (297, 2): 1})                      # the later maximum in the second pass of the row kernel
    assert out["rows"] == [1, ONE, ONE]
    # a whole plane of alternating +1 / -1: the maximum recurs at every odd position
    x = np.random.default_rng(2).integers(0, 256, (1, 6, 259), dtype=np.uint8)
    t = np.where(np.arange(4 * 257) % 2 == 0, 1.0, -1.0).reshape(1, 4, 257)
    hat = _hat_for_terms(x, t)
    for order in ORDERS:
        got = _got(x, hat, hat_scale=1., weighted=0, order=order)
        _assert_equal(got, _want(x, order, 0, x_hat=hat, hat_scale=1.), f"alternating {order}")
    assert [int(g[0]) for g in _got(x, hat, hat_scale=1., weighted=0, order="rows")[:3]] == [1, ONE, 0]


def test_sum_returning_to_zero_keeps_the_empty_prefix():
    """t = -1, .., +1 (T = -1, .., 0): the maximum 0 is T(0), met again at the end -- in another chunk of the row, or in another row"""
    for far in (70, 300, 597):
        out = _tie_case((1, 3, 600), {(0, 0): -1, (0, far): 1})
        assert out["rows"] == [0, 0, 0] == out["rows_up"]
    out = _tie_case((1, 5, 7), {(0, 0): -1, (2, 4): 1})
    assert out["rows"] == [0, 0, 0]
    assert out["rows_up"] == [5, ONE, 0]                                                    # bottom-up the +1 comes first, at path position 5
    out = _tie_case((1, 300, 5), {(0, 0): -1, (297, 2): 1})
    assert out["rows"] == [0, 0, 0] and out["rows_up"] == [3, ONE, 0]


def test_nan_inf_and_huge_predictions_follow_the_restatement():
    shape = (2, 9, 70)
    rng = np.random.default_rng(9)
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    full = rng.random(shape, dtype=np.float32)
    inner = (rng.random((2, 7, 68), dtype=np.float32) * np.float32(255.0)).astype(np.float32)
    for hat, (r0, c0) in ((full, (1, 1)), (inner, (0, 0))):
        for i, v in enumerate((np.nan, np.inf, -np.inf, 1e30, -1e30, np.nan)):
            hat[i % 2, r0 + i, c0 + 3 * i] = v
            hat[i % 2, r0 + 6 - i, c0 + 66 - i] = v
    for weighted in (0, 1):
        for order in ORDERS:
            for hat, scale in ((full, 255.), (inner, 1.)):
                got = _got(x, hat, hat_scale=scale, weighted=weighted, order=order)
                _assert_equal(got, _want(x, order, weighted, x_hat=hat, hat_scale=scale), f"special values {weighted} {order} {scale}")
    q = sequential_np.ws_terms(x[0], x_hat=inner[0], hat_scale=1., weighted=0)
    assert (q == 0).sum() >= 2 and (np.abs(q) == 4096 * ONE).sum() >= 3                    # the NaN rule and the clamp both took part


def test_an_image_alone_and_at_every_position_of_a_batch():
    rng = np.random.default_rng(21)
    x = rng.integers(0, 256, (3, 37, 300), dtype=np.uint8)
    y = rng.random((3, 37, 300), dtype=np.float32)
    for i in range(3):
        others = [j for j in range(3) if j != i]
        for source in ("filter", "x_hat"):
            def run(idx):
                kw = dict(pixel_filter=KB) if source == "filter" else dict(x_hat=y[idx], hat_scale=255.)
                return _got(x[idx], weighted=1, order="rows_up", **kw)
            alone = run([i])
            for pos in range(3):
                idx = others[:pos] + [i] + others[pos:]
                for a, b in zip(alone, run(idx)):
                    np.testing.assert_array_equal(a[0], b[pos], err_msg=f"image {i} at position {pos} ({source})")
    a, b = _got(x, pixel_filter=KB, weighted=1, order="rows"), _got(x, pixel_filter=KB, weighted=1, order="rows")
    _assert_equal(a, b, "two calls")


def test_without_the_curve_and_with_a_four_dimensional_prediction():
    x = np.random.default_rng(4).integers(0, 256, (2, 20, 33), dtype=np.uint8)
    y = np.random.default_rng(5).random((2, 1, 20, 33), dtype=np.float32)
    out = ops.ws_sequential(_dev(x), _dev(y), weighted=0)
    assert len(out) == 3
    want = _want(x, "rows", 0, x_hat=y[:, 0], hat_scale=255.)
    for g, w in zip(out, want[:3]):
        np.testing.assert_array_equal(g.cpu().numpy(), w)


# ---- consistency with K11 ----------------------------------------------------------------------------------------------------

def test_total_agrees_with_the_ws_statistic_of_k11():
    """t_all / 2^24 / M + 1/4 = mean(r) up to one float32 rounding of r - 1/4 at |r| < 256 (<= 2^-17) and the quantisation (<= 2^-25) per
    pixel: derived, not measured"""
    x = np.random.default_rng(17).integers(0, 256, (2, 67, 259), dtype=np.uint8)
    m = 65 * 257
    t_all = ops.ws_sequential(_dev(x), pixel_filter=KB, mean_filter=AVG, weighted=0)[2].cpu().numpy()
    _, sums = ops.ws_attack(_dev(x), None, pixel_filter=KB, mean_filter=AVG, weighted=0, return_sums=True)
    sums = sums.cpu().numpy()
    assert (sums[:, 0] == m).all()
    diff = np.abs(t_all / 2.0 ** 24 / m + 0.25 - sums[:, 1] / sums[:, 0])
    print("K27 total vs K11 mean:", diff)
    assert (diff <= 2.0 ** -16).all()


# ---- K28 against Philox of embed_np ------------------------------------------------------------------------------------------

SEEDS = [(5 << 32) | 77, 123456789]


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 5), (2, 3, 5), (1, 16, 300), (1, 67, 259)])
def test_sequential_simulator_equals_numpy_bit_for_bit(shape):
    n, h, w = shape
    cover = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    seeds = SEEDS[:n]
    xs, sd = _dev(cover), torch.tensor(np.array(seeds, dtype=np.uint64).view(np.int64)).to(DEV)
    thresholds = torch.from_numpy(np.array([ops.lsbr_threshold(1.0)] * n, dtype=np.uint32).view(np.int32)).to(DEV)
    full, full_changes = ops.embed_lsbr(xs, sd, thresholds)
    full = full.cpu().numpy()
    for order in ORDERS:
        pos = sequential_np.path_positions(h, w, order)
        twins = {}
        for alpha in (0.0, 1e-9, 0.3, 1.0):
            m = sequential_np.lsbrs_count(alpha, h, w)
            assert m == embed.lsbrs_count(alpha, h, w)
            stego, changes = ops.embed_lsbr_seq(xs, sd, torch.full((n,), m, dtype=torch.int64, device=DEV), order)
            assert stego.dtype == torch.uint8 and stego.shape == shape and changes.dtype == torch.int64
            stego, changes = stego.cpu().numpy(), changes.cpu().numpy()
            twins[alpha] = stego
            for i in range(n):
                np.testing.assert_array_equal(stego[i], sequential_np.lsbrs_np(cover[i], alpha, seeds[i], order), err_msg=f"{order} {alpha} image {i}")
            np.testing.assert_array_equal(changes, (stego != cover).sum(axis=(1, 2)))
            assert (stego[:, pos >= m] == cover[:, pos >= m]).all()                        # at and beyond position m: the cover
            via, via_changes = embed.simulate(xs, "lsbrs", alpha, seeds, order=order)
            assert (via.cpu().numpy() == stego).all() and (via_changes.cpu().numpy() == changes).all()
        np.testing.assert_array_equal(twins[1.0], full)                                    # alpha = 1 is LSBR at alpha = 1
        assert (twins[0.0] == cover).all() and (twins[1e-9] == cover).all()
        m = sequential_np.lsbrs_count(0.3, h, w)
        assert (twins[0.3][:, pos < m] == twins[1.0][:, pos < m]).all()                     # a prefix of the larger payload's twin
    assert (full_changes.cpu().numpy() == (full != cover).sum(axis=(1, 2))).all()


def test_sequential_simulator_takes_one_count_per_image_and_may_write_in_place():
    cover = np.random.default_rng(8).integers(0, 256, (3, 19, 23), dtype=np.uint8)
    seeds = [SEEDS[0], SEEDS[1], 3]
    counts = [0, 100, 19 * 23 + 5]                                                         # (a count past the last pixel is the last pixel)
    xs, sd = _dev(cover), torch.tensor(np.array(seeds, dtype=np.uint64).view(np.int64)).to(DEV)
    for order in ORDERS:
        stego, changes = ops.embed_lsbr_seq(xs, sd, torch.tensor(counts, dtype=torch.int64).to(DEV), order)
        for i, m in enumerate(counts):
            np.testing.assert_array_equal(stego[i].cpu().numpy(), sequential_np.lsbrs_np(cover[i], None, seeds[i], order, count=m))
        buf, ch = xs.clone(), torch.empty(3, dtype=torch.int64, device=DEV)
        lib = ops._lib.load()
        ops.check(lib.wsu_embed_lsbr_seq(buf.data_ptr(), sd.data_ptr(), torch.tensor(counts, dtype=torch.int64).to(DEV).data_ptr(),
                                         ops.order_id(order), buf.data_ptr(), ch.data_ptr(), 3, 19, 23, ops._stream()), "wsu_embed_lsbr_seq")
        assert torch.equal(buf, stego) and torch.equal(ch, changes)
    alphas = [0.0, 0.25, 1.0]
    stego = embed.simulate(xs, "LSBRS", alphas, seeds, order="rows_up")[0].cpu().numpy()
    for i, a in enumerate(alphas):
        np.testing.assert_array_equal(stego[i], sequential_np.lsbrs_np(cover[i], a, seeds[i], "rows_up"))
    # the shapes above reach the pixel loop's paths (a) and (c); (b), (d) and (e) need a plane placed by hand.  Two thirds of the pixels
    # are on the path: from the bottom that is whole rows and a part of one
    sd1, ms = sd[:1].contiguous(), {hw: torch.tensor([max(1, 2 * hw // 3)], dtype=torch.int64, device=DEV) for hw in (65, 15, 1)}
    for order in ORDERS:
        def run(ci, co, ch, h, w):
            return lib.wsu_embed_lsbr_seq(ci, sd1.data_ptr(), ms[h * w].data_ptr(), ops.order_id(order), co, ch, 1, h, w, ops._stream())
        check_span_placements("bde", run, lambda p: sequential_np.lsbrs_np(p, None, seeds[0], order, count=max(1, 2 * p.size // 3)))


# ---- both ends on the golden covers ------------------------------------------------------------------------------------------

ALPHAS = (0.05, 0.1, 0.2, 0.4)
CAP = 0.02


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


@pytest.fixture(scope="module")
def covers():
    return np.stack([_plane(f"cover_{k}.png") for k in COVERS])


@pytest.fixture(scope="module")
def kb_estimator():
    return filters.get_filter_estimator(filter_name="KB", flatten=False)


@pytest.fixture(scope="module")
def twins(covers):
    """{(order, alpha): (5,512,512) device LSBRS twins}, seeds = image_seed of the stems, stream 0"""
    x = _dev(covers)
    seeds = [embed.image_seed(f"{k}.png", 0) for k in COVERS]
    return {(order, a): embed.simulate(x, "LSBRS", a, seeds, order=order)[0] for order in ORDERS for a in ALPHAS}


def test_simulate_then_estimate_recovers_the_payload(covers, twins, kb_estimator):
    """|2 beta_hat - alpha| <= 0.02 for every image, stego and cover, on the device and in the restatement (whose own worst case on these
    inputs is 0.0062: cover 8, bottom-up, alpha 0.2; all others <= 0.0022); over the top-down stegos the sequential estimator's mean error
    is below the uniform-placement statistic's with the same predictor and weights"""
    avg = estimate.NAMED_FILTERS["AVG"]
    err_seq, err_rand = [], []
    for order in ORDERS:
        cases = [(0.0, _dev(covers))] + [(a, twins[(order, a)]) for a in ALPHAS]
        for alpha, x in cases:
            k = estimate._changepoint(x, kb_estimator, avg, 1, order)[0].cpu().numpy()
            beta = estimate._stat(x, kb_estimator, avg, 1, False, placement="sequential", order=order)
            assert beta.is_cuda and beta.dtype == torch.float32 and beta.shape == (5,)
            beta = beta.cpu().numpy().astype(np.float64)
            planes = x.cpu().numpy()
            k_np = np.array([sequential_np.ws_sequential_np(p, order, pixel_kernel=KB, mean_kernel=AVG, weighted=1)[0] for p in planes])
            p_np = np.array([sequential_np.payload(int(v), 512, 512, order) for v in k_np])
            print(f"{order} alpha={alpha}: device 2 beta_hat {2 * beta}, restated {p_np}")
            np.testing.assert_array_equal(k, k_np)
            assert np.abs(2 * beta - p_np).max() <= 2.0 ** -24                               # float32 rows of a value below 1
            assert (np.abs(p_np - alpha) <= CAP).all(), (order, alpha, p_np)
            assert (np.abs(2 * beta - alpha) <= CAP).all(), (order, alpha, 2 * beta)
            if order == "rows" and alpha > 0:
                err_seq += list(np.abs(2 * beta - alpha))
                rand = estimate._stat(x, kb_estimator, avg, 1, False, placement="random").cpu().numpy().astype(np.float64)
                assert np.array_equal(rand, estimate._stat(x, kb_estimator, avg, 1, False).cpu().numpy().astype(np.float64))
                err_rand += list(np.abs(2 * rand - alpha))
    print(f"mean |2 beta_hat - alpha| over the top-down stegos: sequential {np.mean(err_seq):.5f}, uniform-placement WS {np.mean(err_rand):.5f}")
    assert len(err_seq) == 20 and np.mean(err_seq) < np.mean(err_rand)


# ---- the drivers -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the five golden covers and their LSBRS alpha 0.2 twins (top-down), written by embed.write_dataset; a second root holds the bottom-up twins"""
    roots = {}
    for order in ORDERS:
        root = tmp_path_factory.mktemp(f"sequential_{order}")
        (root / "images").mkdir()
        for k in COVERS:
            shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
        (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
        folders = embed.write_dataset(root, "LSBRS", 0.2, order=order)
        assert [f.name for f in folders] == [embed.folder_name("LSBRS", 0.2, order)]
        roots[order] = root
    return roots


def test_written_twins_are_the_simulated_ones(dataset, twins):
    for order in ORDERS:
        folder = dataset[order] / embed.folder_name("LSBRS", 0.2, order)
        head = (folder / "files.csv").read_text().splitlines()[:2]
        assert head == ["name,height,width,stego_method,alpha", f"{folder.name}/10.png,512,512,LSBRS,0.2"]
        files = np.stack([_plane(folder / f"{k}.png") for k in COVERS])
        assert (files == twins[(order, 0.2)].cpu().numpy()).all()


@pytest.mark.parametrize("order", ORDERS)
def test_sequential_rows_of_ws_estimate(dataset, twins, order):
    root = dataset[order]
    kw = dict(correct_bias=False, weighted=1, placement="sequential", order=order)
    resb = estimate.run(root, "LSBRS", 0.2, "KB", None, (3,), batched=True, batch_size=2, **kw)
    res = estimate.run(root, "LSBRS", 0.2, "KB", None, (3,), progress_on=False, **kw)
    folder = embed.folder_name("LSBRS", 0.2, order)
    assert resb["name"].tolist() == [f"{folder}/{k}.png" for k in (10, 6, 7, 8, 9)] == res["name"].tolist()
    np.testing.assert_array_equal(resb["beta_hat"].to_numpy(np.float32), res["beta_hat"].to_numpy(np.float32))
    for r in (resb, res):
        assert (r["placement"] == "sequential").all() and (r["order"] == order).all() and (r["weighted"] == 1).all()
    planes = twins[(order, 0.2)].cpu().numpy()
    want = {k: sequential_np.payload(sequential_np.ws_sequential_np(planes[i], order, pixel_kernel=KB, mean_kernel=AVG, weighted=1)[0], 512, 512, order) / 2
            for i, k in enumerate(COVERS)}
    np.testing.assert_array_equal(resb["beta_hat"].to_numpy(np.float32), np.array([want[k] for k in (10, 6, 7, 8, 9)], dtype=np.float32))
    # the default placement: exactly the columns of a call that does not name it
    plain = estimate.run(root, "LSBRS", 0.2, "KB", None, (3,), correct_bias=False, weighted=1, batched=True, batch_size=2)
    rand = estimate.run(root, "LSBRS", 0.2, "KB", None, (3,), correct_bias=False, weighted=1, batched=True, batch_size=2, placement="random",
                        order=order)
    rand1 = estimate.run(root, "LSBRS", 0.2, "KB", None, (3,), correct_bias=False, weighted=1, placement="random", progress_on=False)
    assert list(rand.columns) == list(plain.columns) and "placement" not in plain.columns and "order" not in plain.columns
    plain1 = estimate.run(root, "LSBRS", 0.2, "KB", None, (3,), correct_bias=False, weighted=1, progress_on=False)
    assert list(rand1.columns) == list(plain1.columns) and rand1.equals(plain1)
    assert set(resb.columns) == set(plain.columns) | {"placement", "order"}
    assert rand.equals(plain)
    cov = estimate.run(root, None, None, "KB", None, (3,), batched=True, **kw)
    assert len(cov) == 5 and (2 * cov["beta_hat"].to_numpy(np.float64) <= CAP).all()


def test_sequential_scores_of_the_roc_tables(dataset):
    root = dataset["rows"]
    res = roc.collect_ws_scores(root, ["LSBRS"], [0.2], ("KB", "OLSa"), placement="sequential")
    assert res["model_name"].unique().tolist() == ["KB", "OLSa"] and len(res) == 2 * 10
    assert (res["placement"] == "sequential").all() and (res["order"] == "rows").all()
    assert sorted(res["stego_method"].unique()) == ["Cover", "LSBRS"]
    for name in ("KB", "OLSa"):
        run = estimate.run(root, "LSBRS", 0.2, name, None, (3,), correct_bias=False, weighted=0, batched=True, placement="sequential")
        got = res[(res.model_name == name) & (res.stego_method == "LSBRS")]
        assert got["name"].tolist() == run["name"].tolist() and len(got) == 5
        np.testing.assert_array_equal(got["beta_hat"].to_numpy(np.float32), run["beta_hat"].to_numpy(np.float32))
    plain = roc.collect_ws_scores(root, ["LSBRS"], [0.2], ("KB",))
    assert "placement" not in plain.columns and "order" not in plain.columns
    assert plain.equals(roc.collect_ws_scores(root, ["LSBRS"], [0.2], ("KB",), placement="random"))
    df = roc.produce_roc(res)
    assert sorted(roc.auc_table(df)["model_name"]) == ["KB", "OLSa"]


def test_unet_prediction_stays_on_the_device(covers):
    """an untrained unet_1 in the default mode: the changepoint of its own full-frame output, read back, in the restatement"""
    model = gpu_model(1, "he", mode=DEFAULT_MODE)
    x = _dev(covers[:2])
    est = estimate.UNetEstimator(model)
    avg = estimate.NAMED_FILTERS["AVG"]
    y = unet_plane(model, x).cpu().numpy()
    assert y.shape == (2, 512, 512) and y.dtype == np.float32
    for order, weighted in (("rows", 1), ("rows_up", 0)):
        got = [t.cpu().numpy() for t in estimate._changepoint(x, est, avg, weighted, order, return_curve=True)]
        _assert_equal(got, _want(covers[:2], order, weighted, x_hat=y, hat_scale=255.), f"unet {order} {weighted}")
        beta = estimate._stat(x, est, avg, weighted, False, placement="sequential", order=order).cpu().numpy()
        np.testing.assert_array_equal(beta, (sequential.payload(got[0], 512, 512, order) / 2).astype(np.float32))
    with pytest.raises(ValueError, match="512x512"):
        estimate._stat(x[:, :100, :100].contiguous(), est, avg, 1, False, placement="sequential")
