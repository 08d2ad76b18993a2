"""GPU: wsu_pair_batch_planes_f32 (ops.pair_batch_planes / ops.side_planes) -- the batch assembly with the parity and demosaic side planes
behind the image -- against numpy, exactly.  Expected values: the host transform's data.parity_oracle / data.demosaic_oracle on u8 / 255
(which run BEFORE the flips and the rotation in the reference's pipeline), then the D4 element."""
import numpy as np
import pytest
import torch

from gpu_util import DEV
from ws_unet_amd import _lib, data, ops
from ws_unet_amd.data.pairs import apply_op

pytestmark = pytest.mark.gpu

SIDES = (0, 1, 2, 3)


def _planes(files, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (files, h, w), dtype=np.uint8)


def _expect_inputs(planes, idx, op, side):
    """(n,P,H,W): oracle planes appended to u8 / 255 by the host transform, then D(op) on the last two axes"""
    out = []
    for i, o in zip(idx, op):
        t = torch.from_numpy(planes[i].astype(np.float32) / np.float32(255))[None]
        if side & 1:
            t = data.parity_oracle(t)
        if side & 2:
            t = data.demosaic_oracle(t)
        out.append(np.ascontiguousarray(apply_op(t.numpy(), o)))
    return np.stack(out)


def _check(planes, idx_in, idx_cov, op, sides=SIDES):
    d = torch.from_numpy(planes).to(DEV)
    n, (h, w) = len(op), planes.shape[1:]
    x0, c0 = ops.pair_batch(d, idx_in, idx_cov, op)
    for side in sides:
        x, c = ops.pair_batch_planes(d, idx_in, idx_cov, op, parity=bool(side & 1), demosaic=bool(side & 2))
        xi, none = ops.pair_batch_planes(d, idx_in, None, op, parity=bool(side & 1), demosaic=bool(side & 2))
        torch.cuda.synchronize()
        p = 1 + (side & 1) + 3 * (side >> 1)
        assert x.shape == (n, p, h, w) and c.shape == (n, 1, h, w) and x.dtype == c.dtype == torch.float32 and none is None
        assert torch.equal(x[:, :1], x0) and torch.equal(c, c0), f"side {side}: plane 0 / covers differ from ops.pair_batch at {h}x{w}"
        assert torch.equal(xi, x), f"side {side}: covers=None changes the inputs at {h}x{w}"
        want = _expect_inputs(planes, idx_in, op, side)
        got = x.cpu().numpy()
        for s in range(n):
            for k in range(p):
                assert np.array_equal(got[s, k], want[s, k]), f"inputs[{s}] plane {k}: source {idx_in[s]} op {op[s]} side {side} at {h}x{w}"


@pytest.mark.parametrize("size", [1, 2, 5, 66, 68])
def test_square_planes_all_ops(size):
    """1, 2: less than a word; 5: odd side, the mirrors keep the Bayer phase; 66: the byte-wise kernel, partial tiles; 68: the word kernel,
    partial tiles.  Repeated and crossed indices: every op with idx_in == idx_cov and with idx_in != idx_cov."""
    planes = _planes(3, size, size, size)
    op = list(range(8)) * 2
    idx_in = [0, 1, 2, 0, 1, 2, 0, 1, 2, 2, 1, 0, 2, 1, 0, 1]
    idx_cov = [0, 0, 2, 1, 1, 0, 0, 2, 1, 2, 0, 0, 1, 1, 2, 1]
    assert {(o, a == b) for o, a, b in zip(op, idx_in, idx_cov)} == {(o, e) for o in range(8) for e in (True, False)}
    _check(planes, idx_in, idx_cov, op)


@pytest.mark.parametrize("h,w", [(2, 3), (5, 7), (6, 72)])
def test_non_square_planes_take_the_mirrors(h, w):
    planes = _planes(2, h, w, h * w)
    _check(planes, [0, 1, 1, 0, 1, 0, 0, 1], [0, 0, 1, 1, 1, 1, 0, 0], [0, 1, 2, 3, 0, 1, 2, 3])


def test_workload_plane_size_once():
    planes = _planes(2, 512, 512, 512)
    _check(planes, [0, 1, 0, 1, 1, 0, 1, 0], [0, 0, 0, 0, 1, 1, 1, 1], list(range(8)), sides=(3,))


def test_side_planes_is_the_identity_assembly():
    planes = _planes(3, 6, 10, 9)
    d = torch.from_numpy(planes).to(DEV)
    for parity in (False, True):
        for demosaic in (False, True):
            y = ops.side_planes(d, parity, demosaic)
            side = int(parity) + 2 * int(demosaic)
            assert np.array_equal(y.cpu().numpy(), _expect_inputs(planes, [0, 1, 2], [0, 0, 0], side))
            assert torch.equal(y[:, 0], ops.u8_to_unit(d))
            assert y.shape[1] == ops.side_plane_count(parity, demosaic)


def test_empty_batch_and_argument_errors():
    d = torch.from_numpy(_planes(3, 5, 7, 0)).to(DEV)
    x, c = ops.pair_batch_planes(d, [], [], [], parity=True, demosaic=True)
    assert x.shape == (0, 5, 5, 7) and c.shape == (0, 1, 5, 7) and x.dtype == torch.float32 and x.is_cuda
    for bad in (([3], [0], [0]), ([0], [-1], [0]), ([0], [0], [8]), ([0], [0], [4])):       # index `files`, index -1, op 8, op 4 on 5x7
        with pytest.raises(ValueError):
            ops.pair_batch_planes(d, *bad, parity=True)
    with pytest.raises(ValueError, match="side"):
        ops._pair_batch_planes(d, [0], [0], [0], 4, True)
    lib = _lib.load()
    assert lib.wsu_pair_batch_planes_f32(None, 1, 4, 4, None, None, None, 1, 1, 3, None, None, None) == -1 and b"null" in lib.wsu_last_error()
    p = d.data_ptr()
    for side in (4, -1):
        assert lib.wsu_pair_batch_planes_f32(p, 3, 5, 7, p, p, p, 1, 0, side, p, p, None) == -1 and b"side" in lib.wsu_last_error()
    assert lib.wsu_pair_batch_planes_f32(p, 3, 5, 7, p, None, p, 1, 0, 3, p, p, None) == -1 and b"together" in lib.wsu_last_error()
    assert lib.wsu_pair_batch_planes_f32(p, 3, 5, 7, p, p, p, 1, 1, 3, p, p, None) == -1 and b"square" in lib.wsu_last_error()
    assert lib.wsu_pair_batch_planes_f32(p, 3, 5, 7, p, p, p, 0, 0, 3, p, p, None) == 0      # n == 0: nothing to do


def test_out_of_range_samples_write_nothing():
    """The raw entry point with what the wrapper refuses: such a sample's planes keep their bytes, its neighbours are assembled."""
    planes = _planes(2, 8, 8, 3)
    d = torch.from_numpy(planes).to(DEV)
    n = 4
    idx_in = torch.tensor([0, 2, 1, 1], dtype=torch.int32, device=DEV)                      # sample 1: index `files`
    idx_cov = torch.tensor([0, 0, -1, 0], dtype=torch.int32, device=DEV)                    # sample 2: cover index -1
    op = torch.tensor([1, 0, 0, 6], dtype=torch.uint8, device=DEV)
    x = torch.full((n, 5, 8, 8), -1.0, device=DEV)
    c = torch.full((n, 1, 8, 8), -1.0, device=DEV)
    rc = _lib.load().wsu_pair_batch_planes_f32(d.data_ptr(), 2, 8, 8, idx_in.data_ptr(), idx_cov.data_ptr(), op.data_ptr(), n, 1, 3,
                                              x.data_ptr(), c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for s in (1, 2):
        assert (x[s] == -1).all() and (c[s] == -1).all()
    assert np.array_equal(x[0].cpu().numpy(), _expect_inputs(planes, [0], [1], 3)[0])
    assert np.array_equal(x[3].cpu().numpy(), _expect_inputs(planes, [1], [6], 3)[0])
