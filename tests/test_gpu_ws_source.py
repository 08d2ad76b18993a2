"""GPU: what the WS statistic entries share (csrc/wsu_metric.h: WsSource and its maker, ws_fold_step, mp_block_finish; ops._ws_source):
every entry refuses the same bad prediction sources, one predictor gives the same bits by each of its three routes, the ordered fold is
exact where a row or a path ends one position before, on and behind a wave step or a chunk, and K33 on the raster path is K27."""
import numpy as np
import pytest
import torch

from gpu_util import DEV
import adaptive_np
import sequential_np
from ws_unet_amd import filters, ops

pytestmark = pytest.mark.gpu

KB = np.asarray(filters.NAMED_FILTERS_2D["KB"])[..., 0]
AVG = np.asarray(filters.NAMED_FILTERS_2D["AVG"])[..., 0]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _raster(x):
    n, h, w = x.shape
    return torch.arange((h - 2) * (w - 2), dtype=torch.int32, device=x.device).repeat(n, 1)


def _accumulate(x, x_hat=None, **kw):
    num, den = (torch.zeros((x.shape[1] - 2, x.shape[2] - 2), dtype=torch.int64, device=x.device) for _ in range(2))
    ops.ws_residual_accumulate(x, num, den, x_hat, **kw)
    return num, den


# every statistic entry as f(x_u8 on the device, x_hat=None, **source and weights) -> a tuple of device tensors
ENTRIES = {
    "ws_attack": lambda x, x_hat=None, **kw: ops.ws_attack(x, x_hat, return_sums=True, **kw),
    "ws_sequential": lambda x, x_hat=None, **kw: ops.ws_sequential(x, x_hat, return_curve=True, **kw),
    "ws_ordered_terms": lambda x, x_hat=None, **kw: (ops.ws_ordered_terms(x, x_hat, **kw),),
    "ws_ordered": lambda x, x_hat=None, **kw: ops.ws_ordered(x, _raster(x), x_hat, **kw),
    "ws_residual_accumulate": _accumulate,
}


def _plane(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_entry_refuses_the_same_bad_sources(entry):
    f = ENTRIES[entry]
    x = _dev(_plane((2, 5, 7), 35))
    hat = torch.zeros((2, 5, 7), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="exactly one"):
        f(x, hat, pixel_filter=KB, mean_filter=AVG)
    with pytest.raises(ValueError, match="exactly one"):
        f(x, mean_filter=AVG)
    with pytest.raises(ValueError, match="3 filters for 2 images"):
        f(x, pixel_filter=np.stack([KB] * 3), mean_filter=AVG)
    with pytest.raises(ValueError, match="does not match"):
        f(x, torch.zeros(2 * 5 * 7 + 1, dtype=torch.float32, device=DEV), mean_filter=AVG)
    with pytest.raises(ValueError, match="uint8"):
        f(x.to(torch.int16), pixel_filter=KB, mean_filter=AVG)
    if entry == "ws_attack":
        beta, sums = f(x, pixel_filter=KB, mean_filter=AVG, weighted=-1)
        assert beta.shape == (2,) and bool(torch.isfinite(sums).all())
    else:
        with pytest.raises(ValueError, match="weighted=-1 is not defined"):
            f(x, pixel_filter=KB, mean_filter=AVG, weighted=-1)


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 3, 3)])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_one_predictor_by_its_three_routes_has_the_same_bits(entry, shape):
    """KB in the kernel; KB once per image; KB's prediction (ops.filter3x3_valid, pixel units: hat_scale = 1) as interiors and as full
    frames, whose border is never read"""
    f = ENTRIES[entry]
    x = _dev(_plane(shape, sum(shape)))
    inner = ops.filter3x3_valid(x.to(torch.float32), KB)
    full = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    full[:, 1:-1, 1:-1] = inner
    for weighted in (0, 1):
        want = f(x, pixel_filter=KB, mean_filter=AVG, weighted=weighted)
        routes = {"per image": f(x, pixel_filter=np.stack([KB] * shape[0]), mean_filter=AVG, weighted=weighted),
                  "interiors": f(x, inner, mean_filter=AVG, hat_scale=1.0, weighted=weighted),
                  "full frames": f(x, full, mean_filter=AVG, hat_scale=1.0, weighted=weighted)}
        for name, got in routes.items():
            assert len(got) == len(want)
            for g, t in zip(got, want):
                assert g.dtype == t.dtype and torch.equal(g, t), (name, weighted)


@pytest.mark.parametrize("order", ["rows", "rows_up"])
@pytest.mark.parametrize("w", [513, 514, 515])
def test_rows_that_end_around_a_wave_step(w, order):
    """K27, interior rows of 511, 512 and 513 pixels: one position short of a step of 512, exactly one, and one into the second"""
    shape = (2, 4, w)
    rng = np.random.default_rng(w)
    x = _plane(shape, w)
    x[0] = (x[0].astype(np.int32) // 8 + 100).astype(np.uint8)                         # a smooth image: positive and negative terms
    y = rng.random(shape, dtype=np.float32)
    for weighted, kw, ref in ((1, dict(pixel_filter=KB), dict(pixel_kernel=KB)), (0, dict(x_hat=_dev(y)), None)):
        got = ops.ws_sequential(_dev(x), mean_filter=AVG, weighted=weighted, order=order, return_curve=True, **kw)
        for i in range(shape[0]):
            want = sequential_np.ws_sequential_np(x[i], order, mean_kernel=AVG, weighted=weighted, **(ref or dict(x_hat=y[i])))
            for name, g, t in zip(("k", "t_max", "t_all", "curve"), got, want):
                np.testing.assert_array_equal(g[i].cpu().numpy(), t, err_msg=f"{name} image {i} weighted {weighted}")


@pytest.mark.parametrize("shape", [(1, 25, 91), (1, 34, 66), (1, 5, 685)])
def test_paths_that_end_around_a_chunk(shape):
    """K33, shuffled paths of 2047 = 23 x 89, 2048 = 32 x 64 and 2049 = 3 x 683 positions: one short of a chunk of 4 x 512, one chunk, and a
    second chunk of one position"""
    n, h, w = shape
    m = (h - 2) * (w - 2)
    assert m in (2047, 2048, 2049)
    rng = np.random.default_rng(m)
    x = (_plane(shape, m).astype(np.int32) // 8 + 100).astype(np.uint8)
    path = np.stack([rng.permutation(m) for _ in range(n)]).astype(np.int32)
    for weighted, flip_rate in ((1, 1.0), (0, 0.5)):
        got = ops.ws_ordered(_dev(x), _dev(path), pixel_filter=KB, mean_filter=AVG, weighted=weighted, flip_rate=flip_rate)
        want = adaptive_np.ws_ordered_np(x[0], path[0], flip_rate, pixel_kernel=KB, mean_kernel=AVG, weighted=weighted)
        assert [int(t[0]) for t in got] == [int(v) for v in want], (weighted, flip_rate)


def test_the_raster_path_at_half_is_the_sequential_statistic():
    """K33 with the raster path and flip_rate = 0.5 against K27 from the top on rows of 513 pixels: the two kernels carry the same step"""
    shape = (2, 6, 515)
    x = _plane(shape, 515)
    x[1] = (x[1].astype(np.int32) // 8 + 100).astype(np.uint8)
    xd = _dev(x)
    for weighted in (0, 1):
        seq = ops.ws_sequential(xd, pixel_filter=KB, mean_filter=AVG, weighted=weighted, order="rows")
        got = ops.ws_ordered(xd, _raster(xd), pixel_filter=KB, mean_filter=AVG, weighted=weighted, flip_rate=0.5)
        for name, g, t in zip(("k", "t_max", "t_all"), got, seq):
            assert torch.equal(g, t), (name, weighted)
