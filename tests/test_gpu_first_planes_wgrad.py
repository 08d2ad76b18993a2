"""GPU: wsu_conv3x3_first_pl_bwd_weight_planes -- the first layer's weight / bias gradient of the planar training path for 1..8 input planes.

Reference: fp64 autograd of the reflect-padded conv on the values the planar gradient holds, as
test_gpu_train_pl_edges.py::test_conv3x3_first_pl_bwd_weight_channel_counts does for the single-plane kernel; the bands are that test's
(same arithmetic: fp32 fused multiply-adds per thread, block partials summed in a fixed order): relative L2 dw < 1e-5, db < 2e-6.
Measured on an MI355X (`pytest -s` prints every case): dw 1.4e-7, db 8.4e-8 at most."""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, GRAD_LO, planar_decode, planar_encode
from ws_unet_amd import _lib, ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 2), (2, 3, 5), (1, 4, 2), (2, 24, 40)]       # the smallest reflect every tap; the last has several blocks (48 rows)


def rel_l2(got, ref) -> float:
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def _case(n, h, w, cin, c, f16):
    g = planar_encode(torch.randn((n, c, h, w), generator=torch.Generator().manual_seed(52)), GRAD_LO)
    gq = planar_decode(g, GRAD_LO, f16_only=f16)
    x = torch.rand((n, cin, h, w), generator=torch.Generator().manual_seed(18 + cin))
    w1 = torch.zeros((c, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    b1 = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    F.conv2d(F.pad(x.double(), (1, 1, 1, 1), mode="reflect"), w1, b1).backward(gq.double())
    return g, x.to(DEV), w1.grad, b1.grad


@pytest.mark.parametrize("products", ["f16f8", "f16"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", [16, 64, 256])
@pytest.mark.parametrize("cin", [1, 2, 4, 5, 8])
def test_weight_gradient_for_every_plane_count(cin, c, shape, products):
    n, h, w = shape
    g, x, rw, rb = _case(n, h, w, cin, c, products == "f16")
    dw, db = ops.conv3x3_first_pl_bwd_weight_planes(g, x, products=products)
    torch.cuda.synchronize()
    ew, eb = rel_l2(dw.cpu(), rw), rel_l2(db.cpu(), rb)
    print(f"first_pl_bwd_weight_planes cin={cin} c={c} {shape} {products}: dw {ew:.2e} db {eb:.2e}")
    assert tuple(dw.shape) == (c, cin, 3, 3) and tuple(db.shape) == (c,)
    assert ew < 1e-5 and eb < 2e-6, (ew, eb)
    dw2, db2 = ops.conv3x3_first_pl_bwd_weight_planes(g, x, products=products)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)                            # deterministic
    dw3, none = ops.conv3x3_first_pl_bwd_weight_planes(g, x, want_bias=False, products=products)
    assert none is None and torch.equal(dw, dw3)


def test_refused_arguments():
    lib = _lib.load()
    g, x, _, _ = _case(1, 4, 4, 8, 16, False)
    big = torch.empty(lib.wsu_conv3x3_first_pl_bwd_weight_planes_workspace_bytes(8, 256) // 4, dtype=torch.float32, device=DEV)
    out = torch.empty(512 * 9 * 9, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(cin, c, ws_bytes):
        return lib.wsu_conv3x3_first_pl_bwd_weight_planes(g.data_ptr(), x.data_ptr(), out.data_ptr(), None, big.data_ptr(), ws_bytes, 1, 4, 4,
                                                          cin, c, 1, st)
    for cin, c in ((0, 16), (9, 16), (1, 512)):
        assert call(cin, c, big.numel() * 4) == -1 and b"bad shape" in lib.wsu_last_error(), (cin, c)
    need = lib.wsu_conv3x3_first_pl_bwd_weight_planes_workspace_bytes(8, 16)
    assert need == (2048 + 1) * 16 * 73 * 4
    assert call(8, 16, need - 4) == -1 and b"workspace" in lib.wsu_last_error()
    assert lib.wsu_conv3x3_first_pl_bwd_weight_planes(None, None, None, None, None, 0, 1, 4, 4, 1, 16, 1, None) == -1
    with pytest.raises(_lib.WsuError):                                             # the wrapper raises the library's error
        ops.conv3x3_first_pl_bwd_weight_planes(g, torch.rand((1, 9, 4, 4), device=DEV))
    assert call(8, 16, need) == 0
    torch.cuda.synchronize()
