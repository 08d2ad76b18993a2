"""GPU: what the count kernels share (csrc/wsu_count.h: the strip tile and its loaders, the flush, the launch set-up) on inputs that the
per-kernel files do not reach: planes whose base is off the 16-byte grid, pairs / groups / runs across the column-tile boundary, a batch
against its images one by one, and a dirty table handed to every raw entry point twice.  K24 ols_moments, K25 spa_tables, K26 rs_counts,
K36 spam_counts, K31 jpeg_energies, each bit for bit against its numpy restatement (ols_np, structural_np, spam_np, jpeg_np)."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import DEV
import jpeg_np
import ols_np
import spam_np
import structural_np
from ws_unet_amd import _lib, ops

pytestmark = pytest.mark.gpu

SPAM_CONFIGS = ((2, 3), (1, 4))                                             # (order, T)
JPEG_TABLES = jpeg_np.tables((50, 90))
# name -> (the op on a device tensor, the restatement on the host planes)
STRIP = {"K24": (ops.ols_moments, ols_np.moments), "K25": (ops.spa_tables, structural_np.spa_table), "K26": (ops.rs_counts, structural_np.rs_counts)}
STRIP.update({f"K36 {o},{t}": (functools.partial(ops.spam_counts, order=o, T=t), functools.partial(spam_np.counts, order=o, T=t)) for o, t in SPAM_CONFIGS})
K31 = (lambda x: ops.jpeg_energies(x, JPEG_TABLES), lambda x: jpeg_np.energies(x, JPEG_TABLES))
ALL = dict(STRIP, K31=K31)


@functools.lru_cache(maxsize=None)
def _planes(shape, constant=None):
    """random pixels with a smooth corner (small differences: the hot bins among the others); image `constant` of the batch all 77"""
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    x[:, : (shape[1] + 1) // 2, : shape[2] // 3] //= 64
    if constant is not None:
        x[constant] = 77
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(name, shape, constant=None):
    return ALL[name][1](_planes(shape, constant))


def _at_offset(xn, offset):
    """xn as a contiguous device view that starts `offset` bytes into a flat buffer (whose own base is on the 16-byte grid)"""
    buf = torch.zeros(offset + xn.size + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + xn.size].view(xn.shape)
    v.copy_(torch.from_numpy(xn.copy()))
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + offset
    return v


# ---- the image base off the 16-byte grid -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 1, 4, 12])
@pytest.mark.parametrize("shape", [(2, 9, 48), (1, 5, 52)])
def test_strip_kernels_with_the_base_off_the_16_byte_grid(shape, offset):
    """w = 48: every row has the base's alignment (offset 0: the 16-byte load; 4 and 12: K36's word path with a strip off the 16-byte
    grid, the byte path for K25 / K26; 1: bytes everywhere).  w = 52, w % 16 == 4: the rows cycle through the four 4-byte classes."""
    x = _at_offset(_planes(shape), offset)
    for name, (op, _) in STRIP.items():
        np.testing.assert_array_equal(op(x).cpu().numpy(), _want(name, shape), err_msg=name)


@pytest.mark.parametrize("offset", [0, 1, 4, 8, 12])
def test_jpeg_energies_with_the_base_off_the_16_byte_grid(offset):
    """K31 reads a block's rows as 8-byte words and its entry point refuses a plane that is not 8-byte aligned (include/wsu.h;
    tests/test_jpeg_host.py holds it to that), so of the offsets 0, 1, 4 and 12 only 0 can be computed: there and at 8 (off the 16-byte
    grid, on the 8-byte one) the energies are numpy's, at 1, 4 and 12 the call must fail with that message and launch nothing."""
    shape = (1, 8, 48)
    x = _at_offset(_planes(shape), offset)
    if offset % 8:
        with pytest.raises(_lib.WsuError, match="8-byte aligned"):
            K31[0](x)
    else:
        np.testing.assert_array_equal(K31[0](x).cpu().numpy(), _want("K31", shape))


# ---- across the column-tile boundary (512 columns) --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", [("K25", (1, 2, 513)), ("K25", (1, 33, 513)), ("K26", (1, 3, 516)), ("K36 2,3", (1, 33, 516)), ("K36 1,4", (1, 33, 516))])
def test_pairs_groups_and_runs_across_the_column_tile_boundary(name, shape):
    """K25: the horizontal pair of columns 511 and 512 is read through the `right` byte, the vertical pairs of column 512 sit in a second
    tile one pixel wide (33 rows: in two row tiles).  K26: group 128 is the only group of the second tile.  K36: down-left runs start in
    the second tile and end in the first."""
    got = ALL[name][0](torch.from_numpy(_planes(shape).copy()).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(got, _want(name, shape), err_msg=name)


# ---- a batch is its images one by one ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ALL))
def test_a_batch_equals_its_images_one_by_one(name):
    """n = 3, two row tiles, the middle image constant: the hot fields carry all of it and nothing of its neighbours, and every sum lands
    in its own image's row of the table"""
    shape = (3, 40, 48)
    x = torch.from_numpy(_planes(shape, 1).copy()).to(DEV)
    op = ALL[name][0]
    got = op(x)
    np.testing.assert_array_equal(got.cpu().numpy(), _want(name, shape, 1), err_msg=name)
    for i in range(3):
        assert torch.equal(op(x[i:i + 1])[0], got[i]), (name, i)


# ---- the shared memset ------------------------------------------------------------------------------------------------------------------

def test_every_raw_entry_point_zeroes_a_dirty_table_twice():
    shape = (3, 40, 48)
    n, h, w = shape
    x = torch.from_numpy(_planes(shape, 1).copy()).to(DEV)
    lib = ops._lib.load()
    t32 = np.ascontiguousarray(JPEG_TABLES, dtype=np.int32)
    tail = lambda out: (out.data_ptr(), n, h, w)
    calls = {"K24": ("wsu_ols_moments", lambda out: lib.wsu_ols_moments(x.data_ptr(), *tail(out), ops._stream())),
             "K25": ("wsu_spa_tables", lambda out: lib.wsu_spa_tables(x.data_ptr(), *tail(out), ops._stream())),
             "K26": ("wsu_rs_counts", lambda out: lib.wsu_rs_counts(x.data_ptr(), *tail(out), ops._stream())),
             "K36 2,3": ("wsu_spam_counts", lambda out: lib.wsu_spam_counts(x.data_ptr(), *tail(out), 2, 3, ops._stream())),
             "K31": ("wsu_jpeg_energies", lambda out: lib.wsu_jpeg_energies(x.data_ptr(), t32.ctypes.data, len(t32), *tail(out), ops._stream()))}
    for name, (symbol, call) in calls.items():
        want = _want(name, shape, 1)
        out = torch.full(want.shape, 12345, dtype=torch.int64, device=DEV)
        for _ in range(2):
            ops.check(call(out), symbol)
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=name)
