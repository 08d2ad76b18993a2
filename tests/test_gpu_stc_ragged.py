"""GPU: the syndrome-trellis kernels with a message length per image (K43 / K44, ops.stc_embed_ragged / stc_extract_ragged) against the
numpy restatement (stc_np) image by image, bit for bit: lengths 0, 1, n, on both sides of the block-width boundaries, and an image whose
wet pixels leave no solution, in one batch and alone; equal lengths against ops.stc_embed / stc_extract; the receiver on bit 1; lengths
out of range, which the kernels report without touching memory on their account; argument errors."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import DEV
import stc_np
from ws_unet_amd import ops

pytestmark = pytest.mark.gpu

SEED = stc_np.SEED
GRID = [(6, (24, 40)), (7, (24, 40)), (7, (33, 31)), (10, (24, 40))]
PAD = 11                                                                        # message rows are longer than any k: first[i] > 0 fits


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _seeds(n):
    return _dev(np.full(n, SEED, dtype=np.uint64).view(np.int64))


def _cols(h, wmax):
    return _dev(stc_np.columns(h, wmax).view(np.int32))


def plan(shape, h):
    """(image, k, first) per image of the batch: no block; one block of n columns; n blocks of one; n / k not an integer; k divides n
    (every block equally wide); k = n - 1 (one block of two); every block cropped (k < h); widths 2 and 3 around n / k = 2.5; all wet"""
    n = shape[0] * shape[1]
    div = next(k for k in range(n // 10, 1, -1) if n % k == 0)
    return [("a", 0, 0), ("b", 1, 3), ("a", n, 0), ("b", 2 * n // 5 + 1, 5), ("a", div, PAD), ("b", n - 1, 1), ("a", h - 1, 0),
            ("b", 2 * n // 5, 7), ("wet", n, 2), ("allwet", n // 3, 0)]


@functools.lru_cache(maxsize=None)
def batch_np(shape, h):
    n = shape[0] * shape[1]
    rows = plan(shape, h)
    rng = np.random.default_rng([shape[0], shape[1], h, 43])
    msg = rng.integers(0, 2, (len(rows), n + PAD)).astype(np.uint8)
    covers, rhos = zip(*(stc_np.image_case(shape, w) for w, _, _ in rows))
    return np.stack(covers), np.stack(rhos), msg


@functools.lru_cache(maxsize=None)
def want(shape, h, i, change, keyed):
    """stc_np.stego of image i of the plan, computed once"""
    n = shape[0] * shape[1]
    _, k, f = plan(shape, h)[i]
    cover, rho, msg = batch_np(shape, h)
    if k == 0:
        return cover[i], 0.0, 0, True
    return stc_np.stego(cover[i], rho[i], msg[i, f:f + k], stc_np.columns(h, -(-n // k)), h, path=stc_np.key_path(SEED, n) if keyed else None,
                        change=change, seed=SEED)


def _same(got, i, ref, what):
    stego, cost, changes, ok = (t[i] for t in got)
    np.testing.assert_array_equal(stego.cpu().numpy(), ref[0], err_msg=what)
    assert cost.cpu().numpy().view(np.uint64) == np.float64(ref[1]).view(np.uint64), (what, cost.item(), ref[1])
    assert changes.item() == ref[2] and bool(ok.item()) == ref[3], what


@pytest.mark.parametrize("h,shape", GRID)
def test_a_ragged_batch_equals_the_restatement_image_by_image(h, shape):
    n = shape[0] * shape[1]
    rows = plan(shape, h)
    cover, rho, msg = (_dev(a) for a in batch_np(shape, h))
    ks, first = _i32(k for _, k, _ in rows), _i32(f for _, _, f in rows)
    cols, seeds = _cols(h, n), _seeds(len(rows))
    keyed = h != 6
    path = _dev(np.tile(stc_np.key_path(SEED, n), (len(rows), 1))) if keyed else None
    change = "pm1" if h == 7 else "flip"
    got = ops.stc_embed_ragged(cover, rho, msg, cols, seeds, ks=ks, first=first, h=h, path=path, change=change)
    assert got[0].dtype == torch.uint8 and got[1].dtype == torch.float64 and got[2].dtype == torch.int64 and got[3].dtype == torch.uint8
    refs = [want(shape, h, i, change, keyed) for i in range(len(rows))]
    for i, (w, k, f) in enumerate(rows):
        _same(got, i, refs[i], f"h {h} image {i} ({w}, k {k}, first {f})")
    assert [r[3] for r in refs][:8] == [True] * 8 and not refs[8][3] and not refs[9][3]          # the plan's last two have no solution
    assert got[1][0].item() == 0.0 and torch.equal(got[0][0], cover[0])
    # the receiver: every row holds its image's bits where the plan put them and nothing else
    read = ops.stc_extract_ragged(got[0], cols, ks=ks, first=first, bits=n + PAD, h=h, path=path)
    assert read.shape == (len(rows), n + PAD) and read.dtype == torch.uint8
    read_np, msg_np = read.cpu().numpy(), batch_np(shape, h)[2]
    for i, (w, k, f) in enumerate(rows):
        assert not read_np[i, :f].any() and not read_np[i, f + k:].any(), i
        if refs[i][3]:
            np.testing.assert_array_equal(read_np[i, f:f + k], msg_np[i, f:f + k], err_msg=f"image {i}")
        elif k:
            flat = batch_np(shape, h)[0][i].reshape(-1) & 1
            flat = flat[stc_np.key_path(SEED, n)] if keyed else flat
            np.testing.assert_array_equal(read_np[i, f:f + k], stc_np.syndrome(flat, k, stc_np.columns(h, -(-n // k)), h), err_msg=f"image {i}")
    # each image alone, and the batch again in slices of three
    for i in range(len(rows)):
        one = ops.stc_embed_ragged(cover[i:i + 1], rho[i:i + 1], msg[i:i + 1], cols, seeds[i:i + 1], ks=ks[i:i + 1], first=first[i:i + 1], h=h,
                                   path=None if path is None else path[i:i + 1], change=change)
        assert all(torch.equal(a[0], b[i]) for a, b in zip(one, got)), i
    cut = ops.stc_embed_ragged(cover, rho, msg, cols, seeds, ks=ks, first=first, h=h, path=path, change=change,
                               workspace_cap=3 * ops.stc_workspace_bytes(n, h))
    assert all(torch.equal(a, b) for a, b in zip(cut, got))


@pytest.mark.parametrize("h,shape", GRID)
def test_equal_lengths_are_the_uniform_entry_points(h, shape):
    n = shape[0] * shape[1]
    names = ("b", "a", "wet")
    for k in stc_np.ks_of(shape, h):
        cover, rho = (_dev(np.stack(v)) for v in zip(*(stc_np.image_case(shape, w) for w in names)))
        msg = _dev(np.stack([stc_np.message_case(shape, k, w) for w in names]))
        cols, seeds = _cols(h, -(-n // k)), _seeds(3)
        for change in ("flip", "pm1"):
            uniform = ops.stc_embed(cover, rho, msg, cols, seeds, h=h, change=change)
            ragged = ops.stc_embed_ragged(cover, rho, msg, cols, seeds, ks=_i32([k] * 3), h=h, change=change)
            assert all(torch.equal(a, b) for a, b in zip(uniform, ragged)), (h, k, change)
        assert torch.equal(ops.stc_extract_ragged(uniform[0], cols, ks=_i32([k] * 3), bits=k, h=h), ops.stc_extract(uniform[0], cols, k, h=h))


def test_the_receiver_reads_the_bit_it_is_told():
    shape, h = (33, 31), 7
    n = 1023
    planes = np.stack([stc_np.image_case(shape, w)[0] for w in ("a", "b")])
    ks = [2 * n // 5 + 1, 77]
    cols = _cols(h, -(-n // 77))
    for bit in (0, 1, 7):
        got = ops.stc_extract_ragged(_dev(planes), cols, ks=_i32(ks), bits=max(ks), bit=bit, h=h).cpu().numpy()
        for i, k in enumerate(ks):
            np.testing.assert_array_equal(got[i, :k], stc_np.syndrome((planes[i].reshape(-1) >> bit) & 1, k, stc_np.columns(h, -(-n // k)), h))
            assert not got[i, k:].any()
    # two calls fill one row: bit 1 first, then bit 0 behind it
    out = torch.zeros((2, ks[0] + 77), dtype=torch.uint8, device=DEV)
    ops.stc_extract_ragged(_dev(planes), cols, ks=_i32(ks), bit=1, h=h, out=out)
    ops.stc_extract_ragged(_dev(planes), cols, ks=_i32([77, 77]), first=_i32(ks), bit=0, h=h, out=out)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[1, 77:154], stc_np.syndrome(planes[1].reshape(-1) & 1, 77, stc_np.columns(h, -(-n // 77)), h))
    np.testing.assert_array_equal(got[1, :77], stc_np.syndrome((planes[1].reshape(-1) >> 1) & 1, 77, stc_np.columns(h, -(-n // 77)), h))


@pytest.mark.parametrize("h", [6, 7])
def test_lengths_out_of_range_are_reported_not_followed(h):
    """k < 0, k > n, first < 0, first + k past the row, and a k whose blocks are wider than the column table: each is copied with cost
    +inf and ok 0 and reads nothing; the good image between them is embedded as if alone"""
    shape, n, k = (8, 16), 128, 52
    cover, rho = (_dev(np.stack([v] * 6)) for v in stc_np.image_case(shape, "a"))
    msg = _dev(np.stack([stc_np.message_case(shape, k, "a")] * 6))
    cols = _cols(h, -(-n // k))                                              # 3 entries: k = 30 would need 5
    ks, first = _i32([-1, n + 1, k, k, 1, 30]), _i32([0, 0, 0, -1, k, 0])
    stego, cost, changes, ok = ops.stc_embed_ragged(cover, rho, msg, cols, _seeds(6), ks=ks, first=first, h=h)
    assert ok.tolist() == [0, 0, 1, 0, 0, 0] and changes.tolist()[:2] == [0, 0] and changes.tolist()[3:] == [0, 0, 0]
    assert all(cost[i].item() == float("inf") and torch.equal(stego[i], cover[i]) for i in (0, 1, 3, 4, 5))
    _ref = stc_np.reference(shape, "a", h, k)
    np.testing.assert_array_equal(stego[2].cpu().numpy(), _ref[0])
    assert cost[2].item() == _ref[1] and changes[2].item() == _ref[2]
    out = torch.full((6, k), 9, dtype=torch.uint8, device=DEV)
    ops.stc_extract_ragged(stego, cols, ks=ks, first=first, h=h, out=out)
    assert (out[[0, 1, 3, 4, 5]] == 9).all() and torch.equal(out[2], msg[2])


def test_argument_errors():
    cover = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    rho = torch.ones((2, 8, 8), dtype=torch.float64, device=DEV)
    msg = torch.zeros((2, 20), dtype=torch.uint8, device=DEV)
    cols, seeds, ks = _cols(7, 4), _seeds(2), _i32([20, 7])
    with pytest.raises(ValueError, match="outside 1..10"):
        ops.stc_embed_ragged(cover, rho, msg, cols, seeds, ks=ks, h=11)
    with pytest.raises(ValueError, match="rho must be"):
        ops.stc_embed_ragged(cover, rho.float(), msg, cols, seeds, ks=ks, h=7)
    with pytest.raises(ValueError, match="message must be"):
        ops.stc_embed_ragged(cover, rho, msg[:1], cols, seeds, ks=ks, h=7)
    with pytest.raises(ValueError, match="ks must be"):
        ops.stc_embed_ragged(cover, rho, msg, cols, seeds, ks=ks.to(torch.int64), h=7)
    with pytest.raises(ValueError, match="ks must be"):
        ops.stc_embed_ragged(cover, rho, msg, cols, seeds, ks=ks[:1], h=7)
    with pytest.raises(ValueError, match="first must be"):
        ops.stc_embed_ragged(cover, rho, msg, cols, seeds, ks=ks, first=ks.to(torch.int64), h=7)
    with pytest.raises(ValueError, match="cols must be"):
        ops.stc_embed_ragged(cover, rho, msg, cols.to(torch.int64), seeds, ks=ks, h=7)
    with pytest.raises(ValueError, match="path must be"):
        ops.stc_embed_ragged(cover, rho, msg, cols, seeds, ks=ks, h=7, path=torch.zeros((2, 63), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="seeds must be"):
        ops.stc_embed_ragged(cover, rho, msg, cols, seeds[:1], ks=ks, h=7)
    with pytest.raises(ValueError, match="change"):
        ops.stc_embed_ragged(cover, rho, msg, cols, seeds, ks=ks, h=7, change="both")
    with pytest.raises(ValueError, match="workspace_cap"):
        ops.stc_embed_ragged(cover, rho, msg, cols, seeds, ks=ks, h=7, workspace_cap=0)
    with pytest.raises(ValueError, match="bit=8"):
        ops.stc_extract_ragged(cover, cols, ks=ks, bits=20, bit=8, h=7)
    with pytest.raises(ValueError, match="`out`, or `bits`"):
        ops.stc_extract_ragged(cover, cols, ks=ks, h=7)
    with pytest.raises(ValueError, match="message must be"):
        ops.stc_extract_ragged(cover, cols, ks=ks, h=7, out=torch.zeros((2, 20), dtype=torch.int32, device=DEV))
