"""Phase stamps of the fused decoder entry conv3x3_qu (the -DWSU_QU_STAMPS build: `make -C ws_unet_amd/csrc qustamp`) at unet_2's two decoder
shapes, batch 32 @ 512x512: per step kind (S = a skip chunk, L = a low chunk) the shader cycles of matrix wave 0 from barrier exit to the end of
its matrix section and in the barrier that opens the step, and of loader wave 0 in its vmcnt wait before (and in) that barrier; the tile
epilogue of matrix wave 0; in-kernel clock = s_memtime / s_memrealtime x 100 MHz.
    python tools/stamp_qu.py"""
import ctypes, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent)); sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import numpy as np, torch
from ws_unet_amd import _lib
_lib.LIB_PATH = Path(_lib.LIB_PATH).parent / "libwsu_qustamp.so"
from ws_unet_amd import ops
from gpu_util import planar_q_encode

g = torch.Generator(device="cuda").manual_seed(1)
lib = _lib.load()
lib.wsu_debug_read_qu_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
for (name, n, sl, cl, c2, cout) in [("upconv3+d31", 32, 128, 256, 128, 128), ("upconv4+d41", 32, 256, 128, 64, 64)]:
    cup = cl // 2
    xl = torch.randn((n, cl, sl, sl), device="cuda", generator=g).clamp_min(0)
    xs = torch.randn((n, c2, 2 * sl, 2 * sl), device="cuda", generator=g).clamp_min(0)
    w3 = torch.randn((cout, cup + c2, 3, 3), device="cuda", generator=g) * (2.0 / (9 * (cup + c2))) ** 0.5
    wt = torch.randn((cl, cup, 2, 2), device="cuda", generator=g) * (1.0 / cl) ** 0.5
    w_skip, w_low, bias = ops.pack_conv3x3_up(w3, wt, None, None)
    ql, qs = planar_q_encode(xl), planar_q_encode(xs)
    for _ in range(10):
        ops.conv3x3_up_q(ql, qs, w_skip, w_low, bias, cout)
    torch.cuda.synchronize()
    buf = (ctypes.c_ulonglong * (256 * 16))()
    assert lib.wsu_debug_read_qu_stamps(buf, 256) == 0
    st = np.array(buf[:], dtype=np.float64).reshape(256, 16)
    st = st[st[:, 15] > 0]
    nS, nL = st[:, 5], st[:, 6]
    med = lambda v: float(np.median(v))
    print(f"{name}: workgroups {len(st)}, steps/WG S {med(nS):.0f} L {med(nL):.0f}, kernel {med(st[:, 13]) / 100:.0f} us, "
          f"clock {med(st[:, 14] / st[:, 13]) * 0.1:.3f} GHz")
    for k, nm, cnt in ((0, "S", nS), (1, "L", nL)):
        print(f"  {nm} step (cycles/step): matrix section {med(st[:, k] / cnt):6.0f}  barrier (matrix wave 0) {med(st[:, 2 + k] / cnt):6.0f}  "
              f"loader vmcnt wait {med(st[:, 8 + k] / cnt):6.0f}  barrier (loader 0) {med(st[:, 10 + k] / cnt):6.0f}")
    ntile = nS / (c2 // 16)
    print(f"  epilogue {med(st[:, 4] / ntile):.0f} cycles/tile; loader DMA issue {med(st[:, 12] / (nS + nL)):.0f} cycles/step; "
          f"matrix wave 0 total {med(st[:, 7]):.0f} cycles")
