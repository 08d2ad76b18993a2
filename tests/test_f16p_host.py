"""CPU: the host side of mode 'f16p' (planar H storage, one f16 product per tap; include/wsu.h K1h) -- sizes of the format and of the packed
weights, argument validation of the new entry points before any HIP call, the mode's name, and model construction."""
import pytest

from ws_unet_amd import _lib, ops

PLANAR_H = 2


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_format_and_packed_sizes(lib):
    assert ops.PLANAR_H == PLANAR_H
    # a chunk = two f16 planes of [H][W][16 B] = 32 H W bytes
    assert lib.wsu_planar_h_bytes(1, 16, 1, 1) == 32
    assert lib.wsu_planar_h_bytes(2, 64, 5, 7) == 2 * 4 * 32 * 5 * 7
    assert lib.wsu_planar_h_bytes(3, 48, 512, 512) == 3 * 3 * 32 * 512 * 512
    assert lib.wsu_planar_h_bytes(1, 24, 4, 4) == 0 and lib.wsu_planar_h_bytes(0, 16, 4, 4) == 0
    assert ops.PlanarH.chunk_bytes(6, 10) == 32 * 60
    # weights: per (64-co block, 16-channel chunk) [tap 9][plane 2][64 co][16 B] = 18 KB
    assert lib.wsu_conv3x3_packed_h_bytes(16, 64) == 18432
    assert lib.wsu_conv3x3_packed_h_bytes(128, 256) == 4 * 8 * 18432
    assert lib.wsu_conv3x3_packed_h_bytes(128, 256) == 2 * 9 * 128 * 256       # 2 bytes per weight, nothing else
    assert lib.wsu_conv3x3_packed_h_bytes(24, 64) == 0 and lib.wsu_conv3x3_packed_h_bytes(16, 32) == 0
    # fused decoder entry, low half: per (block, chunk of x_low, dy) [class 4][dx 2][plane 2][64 co][16 B] = 16 KB
    assert lib.wsu_conv3x3_up_packed_h_bytes(16, 64) == 2 * 16384
    assert lib.wsu_conv3x3_up_packed_h_bytes(128, 64) == 8 * 2 * 16384
    assert lib.wsu_conv3x3_up_packed_h_bytes(128, 64) == 2 * 16 * 128 * 64     # 16 combined 2-byte weights per (co, c)
    assert lib.wsu_conv3x3_up_packed_h_bytes(20, 64) == 0 and lib.wsu_conv3x3_up_packed_h_bytes(16, 100) == 0
    t = ops.PlanarH.empty(2, 32, 6, 10, "cpu")
    assert tuple(t.data.shape) == (2, 2, 32 * 60) and not isinstance(t, ops.PlanarQ)


def _rejects(rc, lib, *words):
    assert rc == -1, rc
    msg = lib.wsu_last_error()
    for w in words:
        assert w in msg, (w, msg)


PLANAR_Q = 1
BOTH = pytest.mark.parametrize("fmt", ["q", "h"])


@BOTH
def test_conv3x3_h_fwd_rejects_bad_arguments(lib, fmt):
    f, own = (lib.wsu_conv3x3_h_fwd, PLANAR_H) if fmt == "h" else (lib.wsu_conv3x3_q_fwd, PLANAR_Q)
    # (x1, x2, w, bias, y, y_pool, head_w, head_b, head_out, head_logit, head_cout, n, h, w, c1, c2, cout, relu, y_format, range_flag, stream)
    _rejects(f(None, None, None, None, None, None, None, None, None, None, 0, 1, 8, 8, 64, 0, 64, 1, own, None, None), lib, b"null")
    if fmt == "h":
        _rejects(f(1, None, 1, None, 1, None, None, None, None, None, 0, 1, 8, 8, 64, 0, 64, 1, 1, None, None), lib, b"y_format", b"WSU_PLANAR_H")
    else:
        _rejects(f(1, None, 1, None, 1, None, None, None, None, None, 0, 1, 8, 8, 64, 0, 64, 1, PLANAR_H, None, None), lib, b"y_format")
    _rejects(f(1, None, 1, None, 1, None, None, None, None, None, 0, 1, 8, 8, 64, 0, 96, 1, own, None, None), lib, b"cout=96")
    _rejects(f(1, None, 1, None, None, 1, None, None, None, None, 0, 1, 7, 8, 64, 0, 64, 1, own, None, None), lib, b"even h, w", b"h=7")
    _rejects(f(1, None, 1, None, 1, None, None, None, None, None, 0, 1, 8, 8, 40, 0, 64, 1, own, None, None), lib, b"c1=40")
    _rejects(f(1, None, 1, None, 1, None, None, None, None, None, 0, 1, 1, 8, 64, 0, 64, 1, own, None, None), lib, b"reflect")


@BOTH
def test_conv3x3_up_h_fwd_rejects_bad_arguments(lib, fmt):
    f = lib.wsu_conv3x3_up_h_fwd if fmt == "h" else lib.wsu_conv3x3_up_q_fwd
    # (x_low, x_skip, w_skip, w_low, bias, y, n, h, w, cl, c2, cout, relu, range_flag, stream)
    _rejects(f(1, None, 1, 1, 1, 1, 1, 16, 16, 128, 64, 64, 1, None, None), lib, b"null")
    _rejects(f(1, 1, 1, 1, 1, 1, 1, 16, 16, 128, 64, 80, 1, None, None), lib, b"cout=80")
    _rejects(f(1, 1, 1, 1, 1, 1, 1, 15, 16, 128, 64, 64, 1, None, None), lib, b"h=15")
    _rejects(f(1, 1, 1, 1, 1, 1, 1, 16, 17, 128, 64, 64, 1, None, None), lib, b"w=17")
    _rejects(f(1, 1, 1, 1, 1, 1, 1, 16, 16, 120, 64, 64, 1, None, None), lib, b"cl=120")


@BOTH
def test_packers_reject_bad_arguments(lib, fmt):
    pack, up_pack = (lib.wsu_conv3x3_pack_h, lib.wsu_conv3x3_up_pack_h) if fmt == "h" else (lib.wsu_conv3x3_pack_f4, lib.wsu_conv3x3_up_pack)
    _rejects(pack(None, 1, 64, 64, None), lib, b"null")
    _rejects(pack(1, 1, 64, 48, None), lib, b"cout=48")
    _rejects(up_pack(1, 1, None, None, None, 1, None, 128, 64, 64, 64, None), lib, b"null")
    _rejects(up_pack(1, 1, None, None, 1, 1, None, 128, 64, 64, 72, None), lib, b"cout=72")


def test_packers_and_first_layer_reject_bad_arguments(lib):
    # (x, w, bias, y, n, h, w, cin, cout, relu, y_format, range_flag, relu_mask_out, stream): format H accepted, other values still rejected,
    # and the training forward's ReLU mask still belongs to format A only
    _rejects(lib.wsu_conv3x3_first_pl_fwd(1, 1, None, 1, 1, 8, 8, 1, 64, 1, 3, None, None, None), lib, b"WSU_PLANAR_H")
    _rejects(lib.wsu_conv3x3_first_pl_fwd(1, 1, None, 1, 1, 8, 8, 1, 64, 1, PLANAR_H, None, 1, None), lib, b"relu_mask_out")
    _rejects(lib.wsu_conv3x3_first_pl_fwd(None, 1, None, 1, 1, 8, 8, 1, 64, 1, PLANAR_H, None, None, None), lib, b"null")


def test_wrong_format_tensors_are_refused_before_any_launch():
    with pytest.raises(AssertionError, match="planar Q tensors"):
        ops.conv3x3_q(ops.PlanarH.empty(1, 16, 4, 4, "cpu"), None, None, None, 64)
    q = ops.PlanarQ.empty(1, 16, 4, 4, "cpu")
    with pytest.raises(AssertionError, match="planar H tensors"):
        ops.conv3x3_up_h(q, q, None, None, None, 64)


def test_mode_name_resolves():
    assert ops.mode_id("f16p") == _lib.MODE_F16P == 9
    assert _lib.MODES["f16p"] == 9
    assert ops.mode_id("f16f4p") == 8                    # the default keeps its id


def test_model_constructs_on_cpu():
    from ws_unet_amd.model import get_model
    m = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None, mode="f16p")
    assert m.mode == "f16p" and m.train_mode == "f16f8p"
    assert m._planar_ok()
    m0 = get_model("unet_2", in_channels=1, out_channels=1, channel=[0], drop_rate=None)
    assert m0.mode == "f16f4p"                           # the library default is unchanged
