"""The fused decoder entry (csrc/conv3x3_qu.hip) with one step per low-resolution chunk (both dy slices behind one barrier, the steps in two LDS
regions by parity): against the two-kernel path convt2x2_pl -> conv3x3_q and against itself across launches, at unet_2's two decoder shapes, a
unet_4 entry (many low chunks), odd image sizes, batch 1, and chunk counts that make a tile's step count odd (the region parity flips from tile
to tile).  Every call goes through the C ABI.  The two-kernel path takes multiples of 32 input and 64 output channels for its transposed conv:
low-channel counts of an odd number of chunks are checked against the CPU restatement of the kernel's arithmetic instead."""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, planar_encode, planar_h_decode, planar_h_encode, planar_q_decode, planar_q_encode
from test_gpu_qu import _case, _q_roundtrip, _up_q_ref

pytestmark = pytest.mark.gpu


def _exact(xl, xs, wt, bt, w3, b3):
    xu = F.conv_transpose2d(xl.double(), wt.double(), bt.double(), stride=2)
    return torch.relu(F.conv2d(F.pad(torch.cat([xu, xs.double()], 1), (1, 1, 1, 1), mode="reflect"), w3.double(), b3.double())).float()


@pytest.mark.parametrize("n,hl,wl,cl,cup,c2,cout", [
    (2, 32, 32, 256, 128, 128, 128),          # unet_2 upconv3 + d31: 8 skip steps + 16 low steps per tile
    (2, 64, 64, 128, 64, 64, 64),             # unet_2 upconv4 + d41: 4 skip steps + 8 low steps
    (1, 8, 8, 1024, 512, 512, 512),           # a unet_4 entry: 32 skip steps + 64 low steps, eight output blocks
    (1, 32, 48, 48, 64, 32, 64),              # 64 x 96, three low chunks (not a multiple of two), five steps per tile
    (1, 1024, 768, 32, 64, 16, 64),           # 2048 x 1536, batch 1: three steps per tile, 6144 tiles
    (3, 12, 20, 80, 64, 48, 128),             # 24 x 40: ragged tiles, five low chunks and three skip chunks, two output blocks
])
def test_fused_entry_against_the_two_kernel_path_and_itself(n, hl, wl, cl, cup, c2, cout):
    from ws_unet_amd import ops
    xl, xs, wt, bt, w3, b3 = _case(n, hl, wl, cl, cup, c2, cout, seed=7)
    w_skip, w_low, bias, dense = ops.pack_conv3x3_up(w3.to(DEV), wt.to(DEV), bt.to(DEV), b3.to(DEV), want_dense=True)
    ql, qs = planar_q_encode(xl), planar_q_encode(xs)
    fused = planar_q_decode(ops.conv3x3_up_q(ql, qs, w_skip, w_low, bias, cout))
    for _ in range(3):                                           # (decoded: the scale-byte area has slots past the image that nothing writes)
        assert torch.equal(planar_q_decode(ops.conv3x3_up_q(ql, qs, w_skip, w_low, bias, cout)), fused)
    if cl % 32:                                                  # the kernel's arithmetic restated, through the output encoding (as test_gpu_qu)
        ref = torch.relu(_up_q_ref(xl, xs, w3, dense.cpu(), bias.cpu(), cup))
        scale = float(ref.abs().max())
        d = (fused - _q_roundtrip(ref)).abs()
        assert float((d > 3e-5 * scale).float().mean()) < 0.02 and float(d.max()) < 2.5e-4 * scale, float(d.max()) / scale
        return
    xuq = ops.convt2x2_pl(planar_encode(xl), ops.pack_convt2x2(wt.to(DEV), ops.mode_id("f16f8")), bt.to(DEV), cup, y_format=ops.PLANAR_Q)
    two = planar_q_decode(ops.conv3x3_q(xuq, qs, ops.pack_conv3x3_f4(w3.to(DEV)), b3.to(DEV), cout))
    scale = float(two.abs().max())
    assert float((fused - two).abs().max()) < 6e-4 * scale, float((fused - two).abs().max()) / scale
    if 4 * hl * wl <= 1 << 16:                                   # (the fp64 composition on the CPU only where it is cheap)
        exact = _exact(xl, xs, wt, bt, w3, b3)
        e_f, e_t = float((fused - exact).abs().mean()), float((two - exact).abs().mean())
        assert e_f <= 1.1 * e_t, (e_f, e_t)


@pytest.mark.parametrize("n,hl,wl,cl,cup,c2,cout", [
    (1, 32, 48, 48, 16, 32, 64),
    (2, 16, 16, 128, 64, 64, 64),
])
def test_fused_entry_format_h_repeatable(n, hl, wl, cl, cup, c2, cout):
    """format H (mode 'f16p') shares the step plan: the same result on every launch, and as close to the exact composition as test_gpu_f16p asks"""
    from ws_unet_amd import ops
    from test_gpu_f16p import r16
    xl, xs, wt, bt, w3, b3 = _case(n, hl, wl, cl, cup, c2, cout, seed=9)
    xl, xs = r16(xl), r16(xs)
    wsk, wlo, bias = ops.pack_conv3x3_up_h(w3.to(DEV), wt.to(DEV), bt.to(DEV), b3.to(DEV))
    hl_, hs_ = planar_h_encode(xl), planar_h_encode(xs)
    got = planar_h_decode(ops.conv3x3_up_h(hl_, hs_, wsk, wlo, bias, cout))
    for _ in range(3):
        assert torch.equal(planar_h_decode(ops.conv3x3_up_h(hl_, hs_, wsk, wlo, bias, cout)), got)
    exact = _exact(xl, xs, wt, bt, w3, b3).double()
    rel = float((got.double() - exact).norm() / exact.norm())
    assert rel <= 6e-4, rel


@pytest.mark.parametrize("nsteps,n,h,w", [(2, 1, 64, 96), (4, 1, 64, 96), (2, 2, 128, 128)])
def test_whole_net_fused_entries_against_the_two_kernel_path(nsteps, n, h, w):
    from gpu_util import gpu_model, images01
    _, x = images01(n, h, w, seed=31)
    m = gpu_model(nsteps, "he", "f16f4p")
    assert m.fuse_up_planar
    with torch.no_grad():
        y_f = m(x.to(DEV)).cpu()
        m.fuse_up_planar = False
        y_t = m(x.to(DEV)).cpu()
        m.fuse_up_planar = True
        y_f2 = m(x.to(DEV)).cpu()
    assert torch.equal(y_f, y_f2)
    assert float((y_f - y_t).abs().max()) < 6e-4
