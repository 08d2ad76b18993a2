"""GPU: the WS changepoint along a cost order (K33: ops.ws_ordered, ops.interior_order, ws/adaptive.py) and the HILLRM simulator (K34)
against numpy (adaptive_np), equal as integers / bit for bit; K33's consistency with K27; accuracy on the golden HILLR files;
placement='adaptive' through the drivers of ws.estimate and ws.roc."""
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_util import DEV
import adaptive_np
import hill_np
from ws_unet_amd import embed, filters, ops
from ws_unet_amd.imread import imread4_u8
from ws_unet_amd.ws import adaptive, estimate, roc

pytestmark = pytest.mark.gpu

COVERS = (6, 7, 8, 9, 10)
KB = np.asarray(filters.NAMED_FILTERS_2D["KB"])[..., 0]
AVG = np.asarray(filters.NAMED_FILTERS_2D["AVG"])[..., 0]
ONE = 1 << 24
FLIP_RATES = (1.0, 0.5)
# M = 1; a few pixels; more rows than one wave step has columns (298 > 64) and no multiple of the 512-position step or the 2048-position
# chunk (M = 20264: ten chunks, the last one short, in three workgroups of four waves)
SHAPES = [(2, 3, 3), (2, 5, 7), (3, 70, 300)]
# more interior rows than one pass of the term kernel takes (298 > 4 x 64); more chunks than the finishing workgroup has threads
# (M = 725^2 = 525625: 257 chunks, two per thread)
LONG_SHAPES = [(1, 300, 5), (1, 727, 727)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _got(x, path, x_hat=None, **kw):
    """ops.ws_ordered as numpy: (k (N,), t_max (N,), t_all (N,))"""
    out = ops.ws_ordered(_dev(x), _dev(path), None if x_hat is None else _dev(x_hat), mean_filter=AVG, **kw)
    assert len(out) == 3 and all(t.dtype == torch.int64 and t.is_cuda and t.shape == (x.shape[0],) for t in out)
    return [t.cpu().numpy() for t in out]


def _want(x, path, flip_rate, weighted, x_hat=None, hat_scale=255., pixel_kernels=None):
    per = [adaptive_np.ws_ordered_np(x[i], path[i], flip_rate, x_hat=None if x_hat is None else x_hat[i], hat_scale=hat_scale,
                                     pixel_kernel=None if pixel_kernels is None else pixel_kernels[i], mean_kernel=AVG, weighted=weighted)
           for i in range(x.shape[0])]
    return [np.array([p[j] for p in per]) for j in range(3)]


def _assert_equal(got, want, what):
    for name, g, w in zip(("k", "t_max", "t_all"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def _paths(rng, n, m):
    return np.stack([rng.permutation(m) for _ in range(n)]).astype(np.int32)


def _planes(rng, shape):
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    x[0] = (x[0].astype(np.int32) // 8 + rng.integers(100, 110)).astype(np.uint8)          # a smooth image: positive and negative terms
    return x


def _hat_for_terms(x, t, flip_rate):
    """the interior-layout prediction (scale 1) under which the unweighted term of every interior pixel is exactly t (multiples of 1/4):
    s * (x - x_hat) - flip_rate / 2 = t"""
    xi = x[:, 1:-1, 1:-1]
    s = xi.astype(np.float32) - (xi ^ 1).astype(np.float32)
    return (xi.astype(np.float32) - s * (np.asarray(t, dtype=np.float32) + np.float32(flip_rate / 2))).astype(np.float32)


# ---- K33 against the restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_changepoint_along_a_path_equals_numpy_as_integers(shape):
    n, h, w = shape
    m = (h - 2) * (w - 2)
    rng = np.random.default_rng(sum(shape) * 7 + w)
    x = _planes(rng, shape)
    path = _paths(rng, n, m)
    full = rng.random(shape, dtype=np.float32)
    inner = (rng.random((n, h - 2, w - 2), dtype=np.float32) * np.float32(255.0)).astype(np.float32)
    kernels = (rng.standard_normal((n, 3, 3)) * 0.3).astype(np.float32)
    for weighted in (0, 1):
        for flip_rate in FLIP_RATES:
            kw = dict(weighted=weighted, flip_rate=flip_rate)
            _assert_equal(_got(x, path, pixel_filter=KB, **kw), _want(x, path, flip_rate, weighted, pixel_kernels=[KB] * n), f"KB {kw}")
            _assert_equal(_got(x, path, pixel_filter=kernels, **kw), _want(x, path, flip_rate, weighted, pixel_kernels=kernels),
                          f"per-image filters {kw}")
            _assert_equal(_got(x, path, full, hat_scale=255., **kw), _want(x, path, flip_rate, weighted, x_hat=full, hat_scale=255.),
                          f"full-frame x_hat {kw}")
            _assert_equal(_got(x, path, inner, hat_scale=1., **kw), _want(x, path, flip_rate, weighted, x_hat=inner, hat_scale=1.),
                          f"interior x_hat {kw}")


@pytest.mark.parametrize("shape", LONG_SHAPES)
def test_changepoint_where_the_row_stride_and_the_finishing_runs_wrap(shape):
    n, h, w = shape
    m = (h - 2) * (w - 2)
    rng = np.random.default_rng(sum(shape))
    x = _planes(rng, shape)
    path = _paths(rng, n, m)
    full = rng.random(shape, dtype=np.float32)
    for flip_rate in FLIP_RATES:
        _assert_equal(_got(x, path, pixel_filter=KB, weighted=1, flip_rate=flip_rate), _want(x, path, flip_rate, 1, pixel_kernels=[KB] * n),
                      f"KB {flip_rate}")
        _assert_equal(_got(x, path, full, weighted=0, flip_rate=flip_rate), _want(x, path, flip_rate, 0, x_hat=full), f"x_hat {flip_rate}")


def test_term_plane_and_fold_on_their_own_and_entries_off_the_plane():
    """kernel A's plane is the restatement's; the fold of that plane is the one-call result; a path entry outside 0..M-1 (here -1, M, -M
    and M + 5, in the first step, in a later chunk and at the very end) adds nothing"""
    shape = (3, 70, 300)
    n, h, w = shape
    m = (h - 2) * (w - 2)
    rng = np.random.default_rng(33)
    x = _planes(rng, shape)
    path = _paths(rng, n, m)
    for weighted, flip_rate in ((1, 1.0), (0, 0.5)):
        terms = ops.ws_ordered_terms(_dev(x), pixel_filter=KB, mean_filter=AVG, weighted=weighted, flip_rate=flip_rate)
        assert terms.dtype == torch.int64 and terms.shape == (n, m)
        want = np.stack([adaptive_np.ordered_terms(x[i], pixel_kernel=KB, mean_kernel=AVG, weighted=weighted, tau=adaptive_np.tau_of(flip_rate))
                         for i in range(n)]).reshape(n, m)
        np.testing.assert_array_equal(terms.cpu().numpy(), want)
        whole = _got(x, path, pixel_filter=KB, weighted=weighted, flip_rate=flip_rate)
        _assert_equal([t.cpu().numpy() for t in ops.ws_ordered_fold(terms, _dev(path), h, w)], whole, "terms then fold")
        holes = path.copy()
        for i, (at, bad) in enumerate(((3, -1), (5000, m), (m - 1, -m))):
            holes[i, at] = bad
            holes[i, at // 2] = m + 5
        got = _got(x, holes, pixel_filter=KB, weighted=weighted, flip_rate=flip_rate)
        _assert_equal(got, [np.array([adaptive_np.changepoint_along(want[i], holes[i])[j] for i in range(n)]) for j in range(3)], "holes")
    with pytest.raises(ValueError, match="uint8"):
        ops.ws_ordered(_dev(x).to(torch.int16), _dev(path), pixel_filter=KB, weighted=0)
    with pytest.raises(ValueError, match="path must be"):
        ops.ws_ordered(_dev(x), _dev(path.astype(np.int64)), pixel_filter=KB, weighted=0)
    with pytest.raises(ValueError, match="path must be"):
        ops.ws_ordered(_dev(x), _dev(path[:, :-1]), pixel_filter=KB, weighted=0)


# ---- the identity path and degenerate terms ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_identity_path_at_half_is_the_sequential_statistic_and_the_batch_does_not_matter(shape):
    n, h, w = shape
    m = (h - 2) * (w - 2)
    rng = np.random.default_rng(h * w)
    x = _planes(rng, shape)
    y = rng.random(shape, dtype=np.float32)
    ident = np.broadcast_to(np.arange(m, dtype=np.int32), (n, m)).copy()
    path = _paths(rng, n, m)
    for weighted in (0, 1):
        for pred in (dict(pixel_filter=KB), dict(x_hat=_dev(y))):
            seq = [t.cpu().numpy() for t in ops.ws_sequential(_dev(x), mean_filter=AVG, weighted=weighted, order="rows", **pred)]
            got = [t.cpu().numpy() for t in ops.ws_ordered(_dev(x), _dev(ident), mean_filter=AVG, weighted=weighted, flip_rate=0.5, **pred)]
            _assert_equal(got, seq, f"identity {weighted} {list(pred)}")
    base = _got(x, path, y, weighted=1, flip_rate=1.0)
    for perm in ([*range(1, n), 0], list(reversed(range(n)))):
        again = _got(x[perm], path[perm], y[perm], weighted=1, flip_rate=1.0)
        _assert_equal(again, [b[perm] for b in base], f"images permuted {perm}")
    alone = _got(x[n - 1:], path[n - 1:], y[n - 1:], weighted=1, flip_rate=1.0)
    _assert_equal(alone, [b[n - 1:] for b in base], "the last image alone")


@pytest.mark.parametrize("flip_rate", FLIP_RATES)
def test_all_negative_all_positive_and_a_repeated_maximum(flip_rate):
    shape = (2, 70, 300)
    n, h, w = shape
    m = (h - 2) * (w - 2)
    rng = np.random.default_rng(12)
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    path = _paths(rng, n, m)
    kw = dict(hat_scale=1., weighted=0, flip_rate=flip_rate)
    k, t_max, t_all = _got(x, path, _hat_for_terms(x, -np.ones((n, h - 2, w - 2)), flip_rate), **kw)
    assert (k == 0).all() and (t_max == 0).all() and (t_all == -m * ONE).all()
    k, t_max, t_all = _got(x, path, _hat_for_terms(x, np.ones((n, h - 2, w - 2)), flip_rate), **kw)
    assert (k == m).all() and (t_max == m * ONE).all() and (t_all == m * ONE).all()
    # t = +1, -1, 0 .., +1 along the path (T = 1, 0, .., 1): the maximum 1 is reached at k = 1 and again later -- in the same lane's run,
    # another lane, another step of the chunk, another chunk, the last position
    for far in (5, 70, 600, 3000, m - 1):
        t = np.zeros((n, m), dtype=np.float32)
        for i in range(n):
            t[i, path[i, 0]], t[i, path[i, 1]], t[i, path[i, far]] = 1, -1, 1
        hat = _hat_for_terms(x, t.reshape(n, h - 2, w - 2), flip_rate)
        got = _got(x, path, hat, **kw)
        _assert_equal(got, _want(x, path, flip_rate, 0, x_hat=hat, hat_scale=1.), f"repeated maximum {far}")
        assert (got[0] == 1).all() and (got[1] == ONE).all() and (got[2] == ONE).all()
        # and T = -1, .., 0: the empty prefix keeps the maximum 0
        got = _got(x, path, _hat_for_terms(x, -t.reshape(n, h - 2, w - 2), flip_rate), **kw)
        assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2] == -ONE).all()


# ---- ops.interior_order --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 3, 3), (2, 5, 7), (3, 70, 300)])
def test_interior_order_is_the_stable_argsort(shape):
    rng = np.random.default_rng(shape[2])
    keys = rng.integers(0, 8, shape).astype(np.float32)                                     # eight values: ties everywhere
    keys[-1] = 1.0                                                                          # all equal: the raster order
    got = ops.interior_order(_dev(keys))
    n, m = shape[0], (shape[1] - 2) * (shape[2] - 2)
    assert got.dtype == torch.int32 and got.shape == (n, m) and got.is_cuda and got.is_contiguous()
    for i in range(n):
        np.testing.assert_array_equal(got[i].cpu().numpy(), adaptive_np.interior_order_np(keys[i]))
    np.testing.assert_array_equal(got[-1].cpu().numpy(), np.arange(m))
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    path = adaptive.path_for(_dev(x), "hill")
    cost = ops.hill_cost(_dev(x)).cpu().numpy()
    for i in range(n):
        np.testing.assert_array_equal(path[i].cpu().numpy(), adaptive_np.interior_order_np(cost[i]))


# ---- HILLRM (K34) --------------------------------------------------------------------------------------------------------------

SEEDS = [(5 << 32) | 77, 123456789]


def _plane(name):
    return np.ascontiguousarray(imread4_u8(GOLDEN / name)[..., 3])


@pytest.fixture(scope="module")
def covers():
    return np.stack([_plane(f"cover_{k}.png") for k in COVERS])


def test_hillrm_equals_numpy_bit_for_bit_on_a_golden_cover(covers):
    cover = covers[:1]
    seed = embed.image_seed("6.png", 0)
    stego, changes = embed.simulate(_dev(cover), "HILLRM", 0.1, [seed])
    assert stego.dtype == torch.uint8 and stego.shape == cover.shape and changes.dtype == torch.int64 and changes.shape == (1,)
    stego = stego.cpu().numpy()
    want = adaptive_np.hillrm_np(cover[0], 0.1, seed)
    np.testing.assert_array_equal(stego[0], want)
    assert ((stego ^ cover) <= 1).all() and int(changes[0]) == (stego != cover).sum()
    used = embed.hillrm_rank(0.1, 512, 512) + 1
    print(f"HILLRM alpha 0.1: {int(changes[0])} changes among {used} used pixels")
    assert 0.45 * used < int(changes[0]) < 0.55 * used                                      # a fair coin on 26215 pixels: 6 sigma = 0.019
    zero, none = embed.simulate(_dev(cover), "hillrm", 0.0, [seed])
    assert (zero.cpu().numpy() == cover).all() and int(none[0]) == 0
    key = ops.hill_cost_f64(_dev(cover))
    again = embed.simulate(_dev(cover), "HILLRM", 0.1, [seed], key=key)[0].cpu().numpy()
    assert (again == stego).all()
    hillr = embed.simulate(_dev(cover), "HILLR", 0.2)[0].cpu().numpy()                      # HILLR at twice the change rate flips every used pixel
    assert ((stego != cover) <= (hillr != cover)).all()


@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 9, 7), (1, 16, 300), (2, 67, 259)])
def test_hillrm_on_small_and_odd_planes(shape):
    """a plane narrower than the cost's padding; planes of 63 and 17353 pixels: the last quad is short and the second image starts at an
    address that is no multiple of four"""
    n, h, w = shape
    cover = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    seeds = SEEDS[:n]
    for alpha in (0.0, 0.3, 1.0):
        stego, changes = embed.simulate(_dev(cover), "HILLRM", alpha, seeds)
        stego = stego.cpu().numpy()
        for i in range(n):
            np.testing.assert_array_equal(stego[i], adaptive_np.hillrm_np(cover[i], alpha, seeds[i]), err_msg=f"alpha {alpha} image {i}")
        np.testing.assert_array_equal(changes.cpu().numpy(), (stego != cover).sum(axis=(1, 2)))
    thr = torch.from_numpy(np.array([ops.lsbr_threshold(1.0)] * n, dtype=np.uint32).view(np.int32)).to(DEV)
    sd = torch.tensor(np.array(seeds, dtype=np.uint64).view(np.int64)).to(DEV)
    full = ops.embed_lsbr(_dev(cover), sd, thr)[0]
    assert torch.equal(embed.simulate(_dev(cover), "HILLRM", 1.0, seeds)[0], full)          # alpha = 1 is LSBR at alpha = 1
    alphas = [0.0, 0.6][:n]
    per = embed.simulate(_dev(cover), "HILLRM", alphas, seeds)[0].cpu().numpy()
    for i, a in enumerate(alphas):
        np.testing.assert_array_equal(per[i], adaptive_np.hillrm_np(cover[i], a, seeds[i]))


# ---- accuracy on the golden files ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kb_estimator():
    return filters.get_filter_estimator(filter_name="KB", flatten=False)


def _batched(names, kb_estimator, **kw):
    rows = estimate.attack_batch([str(GOLDEN / f) for f in names], [{} for _ in names], channels=(3,), pixel_estimator=kb_estimator,
                                 weighted=1, **kw)
    return np.array([r["beta_hat"] for r in rows], dtype=np.float64)


def _restated(names, device_keys):
    """beta_hat of the restatement, with its own float64 cost or with the device's float32 keys"""
    out = []
    for f in names:
        x = _plane(f)
        keys = ops.hill_cost(_dev(x[None]))[0].cpu().numpy() if device_keys else hill_np.hill_cost(x)
        k = adaptive_np.ws_ordered_np(x, adaptive_np.interior_order_np(keys), 1.0, pixel_kernel=KB, mean_kernel=AVG, weighted=1)[0]
        out.append(adaptive_np.beta_np(k, 512, 512, 1.0))
    return np.array(out)


def test_accuracy_on_the_golden_hillr_files(kb_estimator):
    """KB, weighted, flip_rate 1, through ws.estimate's batched path.  HILLR at alpha 0.4 changes 0.2 of the pixels: every estimate is
    within 0.01 of that (the restatement with numpy's float64 cost: at most 0.0039) and closer than the plain weighted WS estimate; at
    alpha 0.01 (0.005 of the pixels) every stego estimate exceeds every cover estimate (restated: at least 0.0023 against at most 0.0012)"""
    adaptive_kw = dict(placement="adaptive", criterion="hill", flip_rate=1.0)
    sets = {a: [f"stego_HILLR_{a}_{k}.png" for k in COVERS] for a in ("0.4", "0.01")} | {"cover": [f"cover_{k}.png" for k in COVERS]}
    got = {a: _batched(names, kb_estimator, **adaptive_kw) for a, names in sets.items()}
    for a, names in sets.items():
        own = _restated(names, device_keys=True)
        print(f"{a}: device {got[a]}, restated on the device's keys {own}, restated on numpy's float64 cost {_restated(names, False)}")
        assert np.abs(got[a] - own).max() <= 2.0 ** -24                                        # the same k; float32 rows of a value below 1
    plain = _batched(sets["0.4"], kb_estimator)
    print(f"0.4: plain weighted WS {plain}")
    assert (np.abs(got["0.4"] - 0.2) < np.abs(plain - 0.2)).all()
    assert (np.abs(got["0.4"] - 0.2) < 0.01).all()
    assert got["0.01"].min() > got["cover"].max()


# ---- the drivers -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the five golden covers and their HILLR alpha 0.4 twins, written by embed.write_dataset (the golden stego files bit for bit)"""
    root = tmp_path_factory.mktemp("adaptive")
    (root / "images").mkdir()
    for k in COVERS:
        shutil.copy(GOLDEN / f"cover_{k}.png", root / "images" / f"{k}.png")
    (root / "images" / "files.csv").write_text("name,height,width\n" + "".join(f"images/{k}.png,512,512\n" for k in COVERS))
    folder, = embed.write_dataset(root, "HILLR", 0.4)
    for k in COVERS:
        assert (_plane(folder / f"{k}.png") == _plane(f"stego_HILLR_0.4_{k}.png")).all()
    return root


def test_adaptive_rows_of_ws_estimate(dataset, kb_estimator):
    kw = dict(correct_bias=False, weighted=1, placement="adaptive")
    resb = estimate.run(dataset, "HILLR", 0.4, "KB", None, (3,), batched=True, batch_size=2, **kw)
    res = estimate.run(dataset, "HILLR", 0.4, "KB", None, (3,), progress_on=False, **kw)
    folder = embed.folder_name("HILLR", 0.4)
    assert resb["name"].tolist() == [f"{folder}/{k}.png" for k in (10, 6, 7, 8, 9)] == res["name"].tolist()
    np.testing.assert_array_equal(resb["beta_hat"].to_numpy(np.float32), res["beta_hat"].to_numpy(np.float32))
    for r in (resb, res):
        assert (r["placement"] == "adaptive").all() and (r["criterion"] == "hill").all() and (r["flip_rate"] == 1.0).all()
    for i, k in enumerate((10, 6, 7, 8, 9)):                                                # the rows of `attack`, image by image
        row = estimate.attack(str(dataset / folder / f"{k}.png"), (3,), kb_estimator, weighted=1, imread=imread4_u8,
                              process_image=filters.get_processor_2d((3,)), placement="adaptive", tag=k)
        assert row["beta_hat"] == np.float32(resb["beta_hat"].iloc[i]) and row["tag"] == k
        assert list(row)[-3:] == ["placement", "criterion", "flip_rate"] and "order" not in row
    half = estimate.run(dataset, "HILLR", 0.4, "KB", None, (3,), batched=True, flip_rate=0.5, criterion="hill", **kw)
    assert (half["flip_rate"] == 0.5).all() and not np.array_equal(half["beta_hat"].to_numpy(), resb["beta_hat"].to_numpy())
    # the default placement: exactly the table of a call that does not name it, byte for byte the one that the commit before
    # placement='adaptive' existed wrote with this very call on an MI355X (tests/golden/ws_estimate_KB_HILLR_0.4_weighted.csv)
    plain = estimate.run(dataset, "HILLR", 0.4, "KB", None, (3,), correct_bias=False, weighted=1, batched=True, batch_size=2)
    rand = estimate.run(dataset, "HILLR", 0.4, "KB", None, (3,), correct_bias=False, weighted=1, batched=True, batch_size=2, placement="random",
                        criterion="hill", flip_rate=0.5)
    assert set(resb.columns) == set(plain.columns) | {"placement", "criterion", "flip_rate"} and "order" not in resb.columns
    assert not {"placement", "criterion", "flip_rate", "order"} & set(plain.columns)
    assert rand.to_csv(index=False) == plain.to_csv(index=False)
    assert plain.to_csv(index=False).encode() == (GOLDEN / "ws_estimate_KB_HILLR_0.4_weighted.csv").read_bytes()
    cov = estimate.run(dataset, None, None, "KB", None, (3,), batched=True, **kw)
    assert len(cov) == 5 and (cov["placement"] == "adaptive").all()


def test_adaptive_scores_of_the_roc_tables(dataset):
    res = roc.collect_ws_scores(dataset, ["HILLR"], [0.4], ("KB", "OLSa"), placement="adaptive")
    assert res["model_name"].unique().tolist() == ["KB", "OLSa"] and len(res) == 2 * 10
    assert (res["placement"] == "adaptive").all() and (res["criterion"] == "hill").all() and (res["flip_rate"] == 1.0).all()
    assert "order" not in res.columns and sorted(res["stego_method"].unique()) == ["Cover", "HILLR"]
    for name in ("KB", "OLSa"):
        run = estimate.run(dataset, "HILLR", 0.4, name, None, (3,), correct_bias=False, weighted=0, batched=True, placement="adaptive")
        got = res[(res.model_name == name) & (res.stego_method == "HILLR")]
        assert got["name"].tolist() == run["name"].tolist() and len(got) == 5
        np.testing.assert_array_equal(got["beta_hat"].to_numpy(np.float32), run["beta_hat"].to_numpy(np.float32))
    plain = roc.collect_ws_scores(dataset, ["HILLR"], [0.4], ("KB",))
    assert not {"placement", "criterion", "flip_rate", "order"} & set(plain.columns)
    assert plain.equals(roc.collect_ws_scores(dataset, ["HILLR"], [0.4], ("KB",), placement="random"))
    df = roc.produce_roc(res)
    assert sorted(roc.auc_table(df)["model_name"]) == ["KB", "OLSa"]


def test_hillrm_twins_through_the_embed_cli_and_the_matching_estimator(dataset, covers):
    embed.main(["--data", str(dataset), "--stego-method", "hillrm", "--alphas", "0.4"])
    folder = dataset / embed.folder_name("HILLRM", 0.4)
    head = (folder / "files.csv").read_text().splitlines()[:2]
    assert head == ["name,height,width,stego_method,alpha", f"{folder.name}/10.png,512,512,HILLRM,0.4"]
    seeds = [embed.image_seed(f"{k}.png", 0) for k in COVERS]
    twins = embed.simulate(_dev(covers), "HILLRM", 0.4, seeds)[0].cpu().numpy()
    files = np.stack([_plane(folder / f"{k}.png") for k in COVERS])
    assert (files == twins).all()
    res = estimate.run(dataset, "HILLRM", 0.4, "KB", None, (3,), correct_bias=False, weighted=1, batched=True, placement="adaptive", flip_rate=0.5)
    print("HILLRM alpha 0.4, flip_rate 0.5: beta_hat", res["beta_hat"].to_numpy(), "true", (twins != covers).mean(axis=(1, 2)))
    assert len(res) == 5 and (res["stego_method"] == "HILLRM").all() and (res["flip_rate"] == 0.5).all()
