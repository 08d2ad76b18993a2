"""Thin torch-tensor wrappers over the C ABI (include/wsu.h).

PyTorch is plumbing here: it owns device memory (caching allocator) and the HIP
stream; every computation is a libwsu kernel.  Activations are NHWC tensors of
shape (N, H, W, C), fp32 for modes 'f32' / 'bf16x3', bf16 for mode 'bf16'.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import MODES, MODE_BF16, MODE_BF16X3, MODE_BF16X3S, MODE_F16F8, MODE_F16F8X, MODE_F16F8P, MODE_F16F8Q, MODE_F16F4P, MODE_F16P, check


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """HIP-event timer around libwsu launches on the stream they are launched on (torch's current stream).
    bench.py enables it for the timed region to get the dominant kernel's average launch duration."""

    def __init__(self):
        self.records = []          # (kernel, meta, start_event, end_event)

    def launch(self, kernel: str, meta: dict, fn):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        rc = fn()
        e.record()
        if _layer is not None:
            meta = dict(meta, layer=_layer)
        self.records.append((kernel, meta, s, e))
        return rc

    def per_layer(self):
        """layer tag (set_layer) -> {'kernel', 'launches', 'total_ms', 'avg_ms', 'flops', 'bytes'} with flops / bytes PER LAUNCH;
        launches without a tag are skipped (call after a device sync)."""
        out = {}
        for k, meta, s, e in self.records:
            name = meta.get("layer")
            if name is None:
                continue
            d = out.setdefault(name, {"kernel": k, "launches": 0, "total_ms": 0.0, "flops": meta.get("flops", 0.0), "bytes": meta.get("bytes", 0.0),
                                      **{key: meta[key] for key in ("bytes_2B", "tiles", "steps_per_tile") if key in meta}})
            d["launches"] += 1
            d["total_ms"] += s.elapsed_time(e)
        for d in out.values():
            d["avg_ms"] = d["total_ms"] / max(1, d["launches"])
        return out

    def summary(self):
        """kernel -> {'launches', 'total_ms', 'avg_ms', 'flops', 'bytes'} (call after a device sync)."""
        out = {}
        for k, meta, s, e in self.records:
            d = out.setdefault(k, {"launches": 0, "total_ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["total_ms"] += s.elapsed_time(e)
            d["flops"] += meta.get("flops", 0.0)
            d["bytes"] += meta.get("bytes", 0.0)
        for d in out.values():
            d["avg_ms"] = d["total_ms"] / max(1, d["launches"])
        return out


_timer: Optional[KernelTimer] = None
_layer: Optional[str] = None


def set_layer(name: Optional[str]) -> None:
    """Label the launches that follow (UNet.forward_features names its layers); only read while a KernelTimer is installed."""
    global _layer
    _layer = name


def set_timer(t: Optional[KernelTimer]) -> None:
    global _timer
    _timer = t


def _launch(kernel: str, meta: dict, fn) -> int:
    return fn() if _timer is None else _timer.launch(kernel, meta, fn)


def _ptr(t) -> Optional[int]:
    return None if t is None else t.data_ptr()


def act_dtype(mode: int) -> torch.dtype:
    """dtype of an activation tensor's allocation.  'bf16x3s' / 'f16f8' tensors are float32-typed buffers holding the split encodings of
    include/wsu.h (bf16 hi / lo halves, 4 bytes per element; f16 + one e4m3 residual, 3 bytes per element -> ``store_channels``):
    only libwsu kernels read them."""
    return torch.bfloat16 if mode == MODE_BF16 else torch.float32


def store_channels(c: int, mode: int) -> int:
    """Last dimension of the float32-shaped allocation holding ``c`` channels: 'f16f8' keeps 3 bytes per element."""
    return c * 3 // 4 if mode == MODE_F16F8 else c


def logical_channels(t: torch.Tensor, mode: int) -> int:
    return t.shape[3] * 4 // 3 if mode == MODE_F16F8 else t.shape[3]


def _esz(mode: int) -> int:
    return 2 if mode == MODE_BF16 else (3 if mode == MODE_F16F8 else 4)


def weight_mode(mode: int) -> int:
    """The packed weights of 'bf16x3s' are the 'bf16x3' ones; 'f16f8' has its own packing, shared by 'f16f8x' (the same arithmetic on
    fp32 tensors: the training forward)."""
    return MODE_BF16X3 if mode == MODE_BF16X3S else (MODE_F16F8 if mode in (MODE_F16F8X, MODE_F16F8P, MODE_F16F8Q, MODE_F16F4P, MODE_F16P) else mode)


def first_layer_weight_mode(mode: int) -> int:
    """Packing of the 3x3 weights handed to conv3x3_fused_first (the layer's own mode; kept as the one place that decides it)."""
    return weight_mode(mode)


def _dev_check(*ts: Optional[torch.Tensor]) -> None:
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.WsuError("libwsu kernels run on the GPU only: got a CPU tensor (no CPU fallback exists)")
        if not t.is_contiguous():
            raise _lib.WsuError("libwsu kernels need contiguous tensors")


def mode_id(mode) -> int:
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"unknown precision mode {mode!r}; choose from {sorted(MODES)}")
        return MODES[mode]
    return int(mode)


# ---- weight packing ---------------------------------------------------------------------------------

def pack_conv3x3(w: torch.Tensor, mode: int, dgrad: bool = False) -> torch.Tensor:
    """w: (Cout, Cin, 3, 3) fp32 OIHW on the device -> packed byte buffer."""
    lib = _lib.load()
    w = w.detach()
    _dev_check(w)
    assert w.dtype == torch.float32 and w.dim() == 4 and w.shape[2:] == (3, 3)
    cout, cin = w.shape[:2]
    mode = weight_mode(mode)
    out = torch.empty(lib.wsu_conv3x3_packed_bytes(cin, cout, mode), dtype=torch.uint8, device=w.device)
    fn = lib.wsu_conv3x3_pack_dgrad if dgrad else lib.wsu_conv3x3_pack
    check(fn(w.data_ptr(), out.data_ptr(), cin, cout, mode, _stream()), "wsu_conv3x3_pack")
    return out


def pack_conv3x3_f4(w: torch.Tensor) -> torch.Tensor:
    """w: (Cout, Cin, 3, 3) fp32 OIHW on the device -> the packed weights of conv3x3_q: f16 planes + block-scaled fp4 cross-term
    granules + scale bytes (wsu_conv3x3_pack_f4)."""
    return _pack_conv3x3_planar(PLANAR_Q, w)


def pack_convt2x2(w: torch.Tensor, mode: int) -> torch.Tensor:
    """w: (Cin, Cout, 2, 2) fp32 on the device -> packed byte buffer."""
    lib = _lib.load()
    w = w.detach()
    _dev_check(w)
    assert w.dtype == torch.float32 and w.dim() == 4 and w.shape[2:] == (2, 2)
    cin, cout = w.shape[:2]
    mode = weight_mode(mode)
    out = torch.empty(lib.wsu_convt2x2_packed_bytes(cin, cout, mode), dtype=torch.uint8, device=w.device)
    check(lib.wsu_convt2x2_pack(w.data_ptr(), out.data_ptr(), cin, cout, mode, _stream()), "wsu_convt2x2_pack")
    return out


# ---- forward ops --------------------------------------------------------------------------------------

def conv3x3(x1: torch.Tensor, x2: Optional[torch.Tensor], w_packed: torch.Tensor, bias: Optional[torch.Tensor],
            cout: int, mode: int, relu: bool = True, pool: bool = False, pool_idx: bool = False,
            pad_zero: bool = False):
    """Returns y, or (y, y_pool[, idx]) when ``pool``."""
    lib = _lib.load()
    _dev_check(x1, x2, w_packed, bias)
    n, h, w = x1.shape[:3]
    c1 = logical_channels(x1, mode)
    c2 = 0 if x2 is None else logical_channels(x2, mode)
    dt = act_dtype(mode)
    assert x1.dtype == dt and (x2 is None or (x2.dtype == dt and x2.shape[:3] == x1.shape[:3]))
    y = torch.empty((n, h, w, store_channels(cout, mode)), dtype=dt, device=x1.device)
    yp = idx = None
    if pool:
        yp = torch.empty((n, h // 2, w // 2, store_channels(cout, mode)), dtype=dt, device=x1.device)
        if pool_idx:
            idx = torch.empty((n, h // 2, w // 2, cout), dtype=torch.uint8, device=x1.device)
    esz = _esz(mode)
    meta = {"flops": 2.0 * 9 * (c1 + c2) * cout * n * h * w,
            "bytes": float(n * h * w * (c1 + c2 + cout) * esz + (n * h * w // 4 * cout * esz if pool else 0) + 9 * (c1 + c2) * cout * max(esz, 4 if mode == MODE_F16F8 else 0))}
    check(_launch("conv3x3", meta, lambda: lib.wsu_conv3x3_fwd(
        x1.data_ptr(), _ptr(x2), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), _ptr(yp), _ptr(idx),
        n, h, w, c1, c2, cout, mode, int(relu), int(pad_zero), _stream())), "wsu_conv3x3_fwd")
    if not pool:
        return y
    return (y, yp, idx) if pool_idx else (y, yp)


def conv3x3_head(x1: torch.Tensor, x2: Optional[torch.Tensor], w_packed: torch.Tensor, bias: Optional[torch.Tensor],
                 head_w: torch.Tensor, head_b: Optional[torch.Tensor], mode: int, want_logit: bool = False, want_y: bool = False):
    """Last 3x3 conv (64 output channels) + ReLU fused with the 1x1 head + sigmoid.  Returns out (N,co,H,W) fp32
    [, logit][, y NHWC]."""
    lib = _lib.load()
    hw2 = head_w.detach().reshape(head_w.shape[0], -1)
    _dev_check(x1, x2, w_packed, bias, hw2, head_b)
    n, h, w = x1.shape[:3]
    c1 = logical_channels(x1, mode)
    c2 = 0 if x2 is None else logical_channels(x2, mode)
    cout, hc = hw2.shape[1], hw2.shape[0]
    out = torch.empty((n, hc, h, w), dtype=torch.float32, device=x1.device)
    logit = torch.empty_like(out) if want_logit else None
    y = torch.empty((n, h, w, store_channels(cout, mode)), dtype=act_dtype(mode), device=x1.device) if want_y else None
    esz = _esz(mode)
    meta = {"flops": 2.0 * 9 * (c1 + c2) * cout * n * h * w,
            "bytes": float(n * h * w * ((c1 + c2) * esz + hc * 4) + 9 * (c1 + c2) * cout * max(esz, 4 if mode == MODE_F16F8 else 0))}
    check(_launch("conv3x3", meta, lambda: lib.wsu_conv3x3_head_fwd(
        x1.data_ptr(), _ptr(x2), w_packed.data_ptr(), _ptr(bias), _ptr(y), hw2.data_ptr(), _ptr(head_b), out.data_ptr(), _ptr(logit),
        n, h, w, c1, c2, cout, hc, mode, _stream())), "wsu_conv3x3_head_fwd")
    res = [out]
    if want_logit:
        res.append(logit)
    if want_y:
        res.append(y)
    return res[0] if len(res) == 1 else tuple(res)


def conv3x3_fused_first(x_nchw: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w_packed: torch.Tensor,
                        bias: Optional[torch.Tensor], cout: int, mode: int, relu: bool = True, pool: bool = False, pool_idx: bool = False):
    """e11 + e12 (+pool) in one launch (wsu_conv3x3_fused_first_fwd): x_nchw (N,1,H,W) fp32 -> y NHWC [, y_pool [, idx]]."""
    lib = _lib.load()
    w1 = w1.detach().contiguous()
    _dev_check(x_nchw, w1, b1, w_packed, bias)
    n, cin, h, w = x_nchw.shape
    assert cin == 1 and tuple(w1.shape) == (64, 1, 3, 3) and x_nchw.dtype == torch.float32
    y = torch.empty((n, h, w, store_channels(cout, mode)), dtype=act_dtype(mode), device=x_nchw.device)
    yp = torch.empty((n, h // 2, w // 2, store_channels(cout, mode)), dtype=act_dtype(mode), device=x_nchw.device) if pool else None
    idx = torch.empty((n, h // 2, w // 2, cout), dtype=torch.uint8, device=x_nchw.device) if (pool and pool_idx) else None
    esz = _esz(mode)
    meta = {"flops": 2.0 * 9 * 64 * cout * n * h * w,
            "bytes": float(n * h * w * (4 + cout * esz) + 9 * 64 * cout * max(esz, 4 if mode == MODE_F16F8 else 0) + (n * (h // 2) * (w // 2) * cout * esz if pool else 0))}
    check(_launch("conv3x3", meta, lambda: lib.wsu_conv3x3_fused_first_fwd(
        x_nchw.data_ptr(), w1.data_ptr(), _ptr(b1), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), _ptr(yp), _ptr(idx),
        n, h, w, cout, mode, int(relu), _stream())), "wsu_conv3x3_fused_first_fwd")
    if pool:
        return (y, yp, idx) if pool_idx else (y, yp)
    return y


PLANAR_PLANES = 3            # stored planes per 16-channel chunk: f16 ch 0-7 | f16 ch 8-15 | e4m3 residuals ch 0-15


def planar_shape(n: int, c: int, h: int, w: int):
    """Allocation shape (float32-typed) of a planar 'F16F8P' activation tensor: [n][C/16][3 planes][H][W][16 B] (include/wsu.h)."""
    return (n, c // 16, PLANAR_PLANES, h, w, 4)


PLANAR_A, PLANAR_Q, PLANAR_H = 0, 1, 2     # include/wsu.h WSU_PLANAR_*: the e4m3-residual planar format / the planar Q format of mode 'f16f4p' /
                                           # the planar H format of mode 'f16p'


class _Planar:
    """A planar activation tensor of the Q / H inference paths: `data` uint8 (N, C/16, chunk_bytes(h, w)), opaque to everything but the kernels
    of its format `fmt` (PLANAR_Q / PLANAR_H)."""
    __slots__ = ("data", "n", "c", "h", "w")

    def __init__(self, data: torch.Tensor, n: int, c: int, h: int, w: int):
        self.data, self.n, self.c, self.h, self.w = data, n, c, h, w

    @classmethod
    def empty(cls, n: int, c: int, h: int, w: int, device):
        assert c % 16 == 0
        return cls(torch.empty((n, c // 16, cls.chunk_bytes(h, w)), dtype=torch.uint8, device=device), n, c, h, w)

    @property
    def device(self):
        return self.data.device

    def data_ptr(self) -> int:
        return self.data.data_ptr()


class PlanarQ(_Planar):
    """A planar Q activation tensor ('F16F4P' storage, include/wsu.h, round 4): per image and 16-channel chunk the planes f16 ch 0-7 | f16 ch
    8-15 | Q (32 fp4 nibbles per pixel: the f16 parts and the residuals * 2^11, both over the block's power-of-two scale) as [H][W][16 B], then
    one E8M0 scale byte per pixel in 16 x 32-pixel tile blocks.  `data`: uint8 (N, C/16, chunk_bytes).  Written by the producing kernel's
    epilogue (conv3x3_q / convt2x2_pl / conv3x3_first_pl with y_format=PLANAR_Q), read by conv3x3_q; opaque to everything else."""
    __slots__ = ()
    fmt = PLANAR_Q

    @staticmethod
    def chunk_bytes(h: int, w: int) -> int:
        return 48 * h * w + 512 * ((h + 15) // 16) * ((w + 31) // 32)


class PlanarH(_Planar):
    """A planar H activation tensor ('F16P' storage of mode 'f16p', include/wsu.h K1h): per image and 16-channel chunk the planes f16 ch 0-7 |
    f16 ch 8-15 as [H][W][16 B] -- the first two planes of a PlanarQ chunk, no Q plane and no scale bytes (2 bytes per element).  `data`: uint8
    (N, C/16, 32 H W).  Written by conv3x3_h / conv3x3_up_h / conv3x3_first_pl(y_format=PLANAR_H), read by conv3x3_h and conv3x3_up_h."""
    __slots__ = ()
    fmt = PLANAR_H

    @staticmethod
    def chunk_bytes(h: int, w: int) -> int:
        return 32 * h * w


# What the Q path (mode 'f16f4p') and the H path (mode 'f16p': one product per tap, f16(w) * f16(x), include/wsu.h K1h) differ in on the host: the
# tensor class, the names (a public function = its KernelTimer key, then its lib functions) and the stored bytes per activation element and per
# weight, each as (numerator, denominator).
_PlanarFormat = namedtuple("_PlanarFormat", "cls letter conv conv_fwd packer pack packed_bytes up up_fwd up_packer up_pack up_packed_bytes "
                                            "act_bytes weight_bytes")
_PLANAR = {
    PLANAR_Q: _PlanarFormat(PlanarQ, "Q", "conv3x3_q", "wsu_conv3x3_q_fwd", "pack_conv3x3_f4", "wsu_conv3x3_pack_f4", "wsu_conv3x3_packed_f4_bytes",
                            "conv3x3_up_q", "wsu_conv3x3_up_q_fwd", "pack_conv3x3_up", "wsu_conv3x3_up_pack", "wsu_conv3x3_up_packed_bytes",
                            (49, 16), (28, 9)),
    PLANAR_H: _PlanarFormat(PlanarH, "H", "conv3x3_h", "wsu_conv3x3_h_fwd", "pack_conv3x3_h", "wsu_conv3x3_pack_h", "wsu_conv3x3_packed_h_bytes",
                            "conv3x3_up_h", "wsu_conv3x3_up_h_fwd", "pack_conv3x3_up_h", "wsu_conv3x3_up_pack_h", "wsu_conv3x3_up_packed_h_bytes",
                            (2, 1), (2, 1)),
}


def _planar_out(fmt: int, n: int, c: int, h: int, w: int, device):
    if fmt in _PLANAR:
        return _PLANAR[fmt].cls.empty(n, c, h, w, device)
    return torch.empty(planar_shape(n, c, h, w), dtype=torch.float32, device=device)


def _pack_conv3x3_planar(fmt: int, w: torch.Tensor) -> torch.Tensor:
    f = _PLANAR[fmt]
    lib = _lib.load()
    w = w.detach().contiguous()
    _dev_check(w)
    assert w.dtype == torch.float32 and w.dim() == 4 and w.shape[2:] == (3, 3)
    cout, cin = w.shape[:2]
    nbytes = getattr(lib, f.packed_bytes)(cin, cout)
    if nbytes == 0:
        raise _lib.WsuError(f"{'fp4' if fmt == PLANAR_Q else 'f16'} packing needs cin % 16 == 0 and cout % 64 == 0 (got {cin}, {cout})")
    out = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    check(getattr(lib, f.pack)(w.data_ptr(), out.data_ptr(), cin, cout, _stream()), f.pack)
    return out


def _conv3x3_planar(fmt: int, x1, x2, w_packed, bias, cout, relu, pool, want_y, head_w, head_b, want_logit, range_flag, y_format):
    f = _PLANAR[fmt]
    lib = _lib.load()
    hw2 = None if head_w is None else head_w.detach().reshape(head_w.shape[0], -1).contiguous()
    assert isinstance(x1, f.cls) and (x2 is None or isinstance(x2, f.cls)), f"{f.conv} reads planar {f.letter} tensors (ops.Planar{f.letter})"
    _dev_check(x1.data, None if x2 is None else x2.data, w_packed, bias, hw2, head_b)
    n, h, w, c1 = x1.n, x1.h, x1.w, x1.c
    c2 = 0
    if x2 is not None:
        assert (x2.n, x2.h, x2.w) == (n, h, w)
        c2 = x2.c
    assert w_packed.numel() * w_packed.element_size() == int(getattr(lib, f.packed_bytes)(c1 + c2, cout)), \
        f"w_packed_{f.packer.rsplit('_', 1)[1]} is not {f.packer} of (cin, cout)"
    hc = 0 if hw2 is None else hw2.shape[0]
    yf = PLANAR_A if (hc and fmt == PLANAR_Q) else y_format           # format Q: a y beside the head is written for convt2x2_pl
    y = _planar_out(yf, n, cout, h, w, x1.device) if want_y else None
    yp = _planar_out(yf, n, cout, h // 2, w // 2, x1.device) if pool else None
    out = torch.empty((n, hc, h, w), dtype=torch.float32, device=x1.device) if hc else None
    logit = torch.empty_like(out) if (hc and want_logit) else None
    act = n * h * w * ((c1 + c2) + (cout if want_y else 0)) + (n * (h // 2) * (w // 2) * cout if pool else 0)     # planar elements read + written
    (an, ad), (wn, wd) = f.act_bytes, f.weight_bytes
    meta = {"flops": 2.0 * 9 * (c1 + c2) * cout * n * h * w,
            "bytes": float(act * an / ad + n * h * w * hc * 4 + 9 * (c1 + c2) * cout * wn / wd),
            "bytes_2B": float(act * 2 + n * h * w * hc * 4 + 9 * (c1 + c2) * cout * 2),
            "tiles": n * ((h + 15) // 16) * ((w + 31) // 32) * (cout // 64), "steps_per_tile": (c1 + c2) // 16}
    check(_launch(f.conv, meta, lambda: getattr(lib, f.conv_fwd)(
        x1.data_ptr(), _ptr(x2), w_packed.data_ptr(), _ptr(bias), _ptr(y), _ptr(yp), _ptr(hw2), _ptr(head_b), _ptr(out), _ptr(logit), hc,
        n, h, w, c1, c2, cout, int(relu), yf, _ptr(range_flag), _stream())), f.conv_fwd)
    if hc:
        res = [out] + ([logit] if want_logit else []) + ([y] if want_y else [])
        return res[0] if len(res) == 1 else tuple(res)
    return (y, yp) if pool else y


def _pack_conv3x3_up_planar(fmt: int, w3, wt, bt, b3, want_dense):
    f = _PLANAR[fmt]
    lib = _lib.load()
    w3, wt = w3.detach().contiguous(), wt.detach().contiguous()
    bt = None if bt is None else bt.detach().contiguous()
    b3 = None if b3 is None else b3.detach().contiguous()
    _dev_check(w3, wt, bt, b3)
    assert w3.dtype == torch.float32 and w3.dim() == 4 and w3.shape[2:] == (3, 3) and wt.dtype == torch.float32 and wt.dim() == 4 and wt.shape[2:] == (2, 2)
    cout, ctot = w3.shape[:2]
    cl, cup = wt.shape[:2]
    c2 = ctot - cup
    nbytes = getattr(lib, f.up_packed_bytes)(cl, cout)
    if nbytes == 0 or c2 <= 0 or c2 % 16:
        raise _lib.WsuError(f"fused upsample packing needs cl % 16 == 0, c2 % 16 == 0 (> 0) and cout % 64 == 0 (got cl={cl}, cup={cup}, c2={c2}, cout={cout})")
    w_skip = _pack_conv3x3_planar(fmt, w3[:, cup:])
    w_low = torch.empty(nbytes, dtype=torch.uint8, device=w3.device)
    bias = torch.empty(cout, dtype=torch.float32, device=w3.device)
    dense = torch.empty((cout, cl, 2, 2, 2, 2), dtype=torch.float32, device=w3.device) if want_dense else None
    check(getattr(lib, f.up_pack)(w3.data_ptr(), wt.data_ptr(), _ptr(bt), _ptr(b3), w_low.data_ptr(), bias.data_ptr(), _ptr(dense),
                                  cl, cup, c2, cout, _stream()), f.up_pack)
    return (w_skip, w_low, bias, dense) if want_dense else (w_skip, w_low, bias)


def _conv3x3_up_planar(fmt: int, x_low, x_skip, w_skip_packed, w_low_packed, bias, cout, relu, range_flag):
    f = _PLANAR[fmt]
    lib = _lib.load()
    assert isinstance(x_low, f.cls) and isinstance(x_skip, f.cls), f"{f.up} reads planar {f.letter} tensors (ops.Planar{f.letter})"
    _dev_check(x_low.data, x_skip.data, w_skip_packed, w_low_packed, bias)
    n, h, w, c2, cl = x_skip.n, x_skip.h, x_skip.w, x_skip.c, x_low.c
    assert (x_low.n, 2 * x_low.h, 2 * x_low.w) == (n, h, w), "x_low must have half the skip tensor's height and width"
    assert w_skip_packed.numel() == int(getattr(lib, f.packed_bytes)(c2, cout)), f"w_skip_packed is not {f.packer} of (c2, cout)"
    assert w_low_packed.numel() == int(getattr(lib, f.up_packed_bytes)(cl, cout)), f"w_low_packed is not {f.up_packer} of (cl, cout)"
    assert bias is not None and bias.numel() == cout
    y = f.cls.empty(n, cout, h, w, x_skip.device)
    cup = cl // 2
    act = n * h * w * (c2 + cout) + n * (h // 2) * (w // 2) * cl
    (an, ad), (wn, wd) = f.act_bytes, f.weight_bytes
    # algorithmic work = the two reference ops it replaces: ConvTranspose2d (2 * 4 * cl * cup MACs per low pixel) + the 3x3 conv over cup + c2 channels
    meta = {"flops": 2.0 * 9 * (cup + c2) * cout * n * h * w + 2.0 * 4 * cl * cup * n * (h // 2) * (w // 2),
            "flops_executed": 2.0 * (9 * c2 + 4 * cl) * cout * n * h * w,
            "bytes": float(act * an / ad + (9 * c2 + 16 * cl) * cout * wn / wd), "bytes_2B": float(act * 2 + (9 * (cup + c2) * cout + 4 * cl * cup) * 2),
            "tiles": n * ((h + 15) // 16) * ((w + 31) // 32) * (cout // 64), "steps_per_tile": c2 // 16 + 2 * (cl // 16)}
    check(_launch(f.up, meta, lambda: getattr(lib, f.up_fwd)(
        x_low.data_ptr(), x_skip.data_ptr(), w_skip_packed.data_ptr(), w_low_packed.data_ptr(), bias.data_ptr(), y.data_ptr(),
        n, h, w, cl, c2, cout, int(relu), _ptr(range_flag), _stream())), f.up_fwd)
    return y


def conv3x3_q(x1: PlanarQ, x2: Optional[PlanarQ], w_packed_f4: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
              relu: bool = True, pool: bool = False, want_y: bool = True,
              head_w: Optional[torch.Tensor] = None, head_b: Optional[torch.Tensor] = None, want_logit: bool = False,
              range_flag: Optional[torch.Tensor] = None, y_format: int = PLANAR_Q):
    """3x3 reflect conv (+ReLU, +2x2 max-pool, +1x1 head and sigmoid) in the fp4-cross-term arithmetic on planar Q activations
    (wsu_conv3x3_q_fwd, csrc/conv3x3_q.hip; the default inference mode 'f16f4p').  x1 / x2: PlanarQ; w_packed_f4 from pack_conv3x3_f4;
    y / y_pool: PlanarQ (y_format=PLANAR_Q) or e4m3-residual planar tensors (PLANAR_A: what convt2x2_pl reads; always for a y beside the head).
    Returns y [, y_pool] or, with head_w, out [, logit][, y]."""
    return _conv3x3_planar(PLANAR_Q, x1, x2, w_packed_f4, bias, cout, relu, pool, want_y, head_w, head_b, want_logit, range_flag, y_format)


def conv3x3_q_fused_first(x_nchw: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w_packed_f4: torch.Tensor,
                          bias: Optional[torch.Tensor], cout: int, relu: bool = True, range_flag: Optional[torch.Tensor] = None):
    """e11 + e12 + pool of the default mode in one launch (wsu_conv3x3_q_fused_first_fwd): x_nchw (N,1,H,W) fp32 -> (y, y_pool) PlanarQ.  Bitwise
    conv3x3_first_pl(y_format=PLANAR_Q) followed by conv3x3_q(pool=True); xe11 never reaches HBM."""
    lib = _lib.load()
    w1 = w1.detach()
    _dev_check(x_nchw, w1, b1, w_packed_f4, bias)
    n, cin, h, w = x_nchw.shape
    assert cin == 1 and x_nchw.dtype == torch.float32 and x_nchw.is_contiguous()
    # w1: (64,1,3,3) OIHW, or already the tap-major table (9, 64) the kernel's scalar loads read (UNet caches it per weight version)
    assert tuple(w1.shape) in ((64, 1, 3, 3), (9, 64)) and w1.dtype == torch.float32
    w1t = w1.contiguous() if tuple(w1.shape) == (9, 64) else w1.reshape(64, 9).t().contiguous()
    b1 = torch.zeros(64, dtype=torch.float32, device=x_nchw.device) if b1 is None else b1.detach().contiguous()
    assert w_packed_f4.numel() == int(lib.wsu_conv3x3_packed_f4_bytes(64, cout)), "conv3x3_q_fused_first needs weights from pack_conv3x3_f4 of (64, cout)"
    y = PlanarQ.empty(n, cout, h, w, x_nchw.device)
    yp = PlanarQ.empty(n, cout, h // 2, w // 2, x_nchw.device)
    act = n * h * w * cout + n * (h // 2) * (w // 2) * cout
    meta = {"flops": 2.0 * 9 * 64 * cout * n * h * w + 2.0 * 9 * 64 * n * h * w,
            "bytes": float(n * h * w * 4 + act * 49 / 16 + 9 * 64 * cout * 28 / 9), "bytes_2B": float(n * h * w * 4 + act * 2 + 9 * 64 * cout * 2),
            "tiles": n * ((h + 15) // 16) * ((w + 31) // 32) * (cout // 64), "steps_per_tile": 4}
    check(_launch("conv3x3_q", meta, lambda: lib.wsu_conv3x3_q_fused_first_fwd(
        x_nchw.data_ptr(), w1t.data_ptr(), b1.data_ptr(), w_packed_f4.data_ptr(), _ptr(bias), y.data_ptr(), yp.data_ptr(),
        n, h, w, cout, int(relu), _ptr(range_flag), _stream())), "wsu_conv3x3_q_fused_first_fwd")
    return y, yp


def pack_conv3x3_up(w3: torch.Tensor, wt: torch.Tensor, bt: Optional[torch.Tensor], b3: Optional[torch.Tensor], want_dense: bool = False):
    """Weights of the fused decoder-block entry conv3x3_up_q (wsu_conv3x3_up_pack, csrc/conv3x3_qu.hip).  w3: (Cout, Cup + C2, 3, 3) fp32, the
    block's first conv (input channels [0, Cup) = the transposed conv's output, torch.cat([xu, skip]) order, unet.py:172,178,184); wt: (Cl, Cup, 2, 2)
    fp32, the nn.ConvTranspose2d weights; bt / b3: their biases.  Returns (w_skip_packed, w_low_packed, bias[, wc_dense]): the skip half packed
    like any conv3x3_q weight, the upsampled half as parity-class 2x2-tap weights combined in fp32 on the device, the combined bias, and on
    request the combined weights (Cout, Cl, 2, 2, 2, 2) [py][px][dy][dx]."""
    return _pack_conv3x3_up_planar(PLANAR_Q, w3, wt, bt, b3, want_dense)


def conv3x3_up_q(x_low: PlanarQ, x_skip: PlanarQ, w_skip_packed: torch.Tensor, w_low_packed: torch.Tensor, bias: torch.Tensor, cout: int,
                 relu: bool = True, range_flag: Optional[torch.Tensor] = None) -> PlanarQ:
    """relu(conv3x3_reflect(cat[conv_transpose2x2_s2(x_low), x_skip])) of a decoder block (unet.py:171-173, 177-179, 183-185) in one launch, in the
    arithmetic of the default inference mode (wsu_conv3x3_up_q_fwd, csrc/conv3x3_qu.hip): the upsampled half runs as a 2x2-tap conv on x_low with
    weights combined per output-pixel parity class -- the upsampled tensor never exists.  x_low: PlanarQ at (h/2, w/2); x_skip: PlanarQ at (h, w);
    weights from pack_conv3x3_up.  Returns y: PlanarQ."""
    return _conv3x3_up_planar(PLANAR_Q, x_low, x_skip, w_skip_packed, w_low_packed, bias, cout, relu, range_flag)


# ---- mode 'f16p': one product per tap, f16(w) * f16(x), on planar H tensors (include/wsu.h K1h) -------------------------------------------

def pack_conv3x3_h(w: torch.Tensor) -> torch.Tensor:
    """w: (Cout, Cin, 3, 3) fp32 OIHW on the device -> the packed weights of conv3x3_h: two f16 planes per tap, round to nearest even
    (wsu_conv3x3_pack_h)."""
    return _pack_conv3x3_planar(PLANAR_H, w)


def conv3x3_h(x1: PlanarH, x2: Optional[PlanarH], w_packed_h: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
              relu: bool = True, pool: bool = False, want_y: bool = True,
              head_w: Optional[torch.Tensor] = None, head_b: Optional[torch.Tensor] = None, want_logit: bool = False,
              range_flag: Optional[torch.Tensor] = None):
    """3x3 reflect conv (+ReLU, +2x2 max-pool, +1x1 head and sigmoid) in the one-product arithmetic of mode 'f16p' on planar H activations
    (wsu_conv3x3_h_fwd: the conv3x3_q kernel instantiated for format H).  x1 / x2: PlanarH; w_packed_h from pack_conv3x3_h; y / y_pool (and a y
    beside the head): PlanarH.  Returns y [, y_pool] or, with head_w, out [, logit][, y]."""
    return _conv3x3_planar(PLANAR_H, x1, x2, w_packed_h, bias, cout, relu, pool, want_y, head_w, head_b, want_logit, range_flag, PLANAR_H)


def pack_conv3x3_up_h(w3: torch.Tensor, wt: torch.Tensor, bt: Optional[torch.Tensor], b3: Optional[torch.Tensor], want_dense: bool = False):
    """Weights of conv3x3_up_h (wsu_conv3x3_up_pack_h): as pack_conv3x3_up, the skip half packed by pack_conv3x3_h and the parity-class weights
    combined in fp32 on the device and rounded to f16 once.  Returns (w_skip_packed, w_low_packed, bias[, wc_dense])."""
    return _pack_conv3x3_up_planar(PLANAR_H, w3, wt, bt, b3, want_dense)


def conv3x3_up_h(x_low: PlanarH, x_skip: PlanarH, w_skip_packed: torch.Tensor, w_low_packed: torch.Tensor, bias: torch.Tensor, cout: int,
                 relu: bool = True, range_flag: Optional[torch.Tensor] = None) -> PlanarH:
    """conv3x3_up_q in the one-product arithmetic of mode 'f16p' on planar H tensors (wsu_conv3x3_up_h_fwd): relu(conv3x3_reflect(cat[
    conv_transpose2x2_s2(x_low), x_skip])) in one launch.  x_low: PlanarH at (h/2, w/2); x_skip: PlanarH at (h, w); weights from
    pack_conv3x3_up_h.  Returns y: PlanarH."""
    return _conv3x3_up_planar(PLANAR_H, x_low, x_skip, w_skip_packed, w_low_packed, bias, cout, relu, range_flag)


def conv3x3_pl(x1: torch.Tensor, x2: Optional[torch.Tensor], w_packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
               relu: bool = True, pool: bool = False, want_y: bool = True,
               head_w: Optional[torch.Tensor] = None, head_b: Optional[torch.Tensor] = None, want_logit: bool = False,
               range_flag: Optional[torch.Tensor] = None, x_residual=True, want_mask: bool = False):
    """3x3 reflect conv (+ReLU, +2x2 max-pool, +1x1 head and sigmoid) on planar F16F8P activations (wsu_conv3x3_pl_fwd).
    x1 / x2: planar tensors (N, C/16, 4, H, W, 4); w_packed from pack_conv3x3(mode f16f8) (the block-scaled fp4 cross terms of the default
    inference mode: conv3x3_q on PlanarQ tensors).  Returns y [, y_pool] or, with head_w, out [, logit][, y]."""
    lib = _lib.load()
    hw2 = None if head_w is None else head_w.detach().reshape(head_w.shape[0], -1).contiguous()
    _dev_check(x1, x2, w_packed, bias, hw2, head_b)
    assert x1.dtype == torch.float32 and x1.dim() == 6 and x1.shape[2] == PLANAR_PLANES and x1.shape[5] == 4 and x1.is_contiguous()
    n, nch1, _, h, w, _ = x1.shape
    c1 = nch1 * 16
    c2 = 0
    if x2 is not None:
        assert x2.dtype == torch.float32 and x2.dim() == 6 and x2.shape[0] == n and x2.shape[3:5] == x1.shape[3:5] and x2.is_contiguous()
        c2 = x2.shape[1] * 16
    y = torch.empty(planar_shape(n, cout, h, w), dtype=torch.float32, device=x1.device) if want_y else None
    yp = torch.empty(planar_shape(n, cout, h // 2, w // 2), dtype=torch.float32, device=x1.device) if pool else None
    hc = 0 if hw2 is None else hw2.shape[0]
    out = torch.empty((n, hc, h, w), dtype=torch.float32, device=x1.device) if hc else None
    logit = torch.empty_like(out) if (hc and want_logit) else None
    mask = relu_mask_alloc(n, cout, h, w, x1.device) if want_mask else None      # 1-bit ReLU mask of y for the next conv's data gradient (training)
    act = n * h * w * ((c1 + c2) + (cout if want_y else 0)) + (n * (h // 2) * (w // 2) * cout if pool else 0)     # planar elements read + written
    meta = {"flops": 2.0 * 9 * (c1 + c2) * cout * n * h * w,
            "bytes": float(act * 3 + n * h * w * hc * 4 + 9 * (c1 + c2) * cout * 4),
            # SURVEY 8d counts 2 bytes per activation element (bf16) and per weight: reported beside the format's own 3 B (bench.py per_layer)
            "bytes_2B": float(act * 2 + n * h * w * hc * 4 + 9 * (c1 + c2) * cout * 2),
            "tiles": n * ((h + 15) // 16) * ((w + 31) // 32) * (cout // 64), "steps_per_tile": (c1 + c2) // 16}
    check(_launch("conv3x3_pl", meta, lambda: lib.wsu_conv3x3_pl_fwd(
        x1.data_ptr(), _ptr(x2), w_packed.data_ptr(), _ptr(bias), _ptr(y), _ptr(yp), _ptr(hw2), _ptr(head_b), _ptr(out), _ptr(logit), hc,
        n, h, w, c1, c2, cout, int(relu), int(x_residual), _ptr(range_flag), _ptr(mask), _stream())), "wsu_conv3x3_pl_fwd")
    if hc:
        res = [out] + ([logit] if want_logit else []) + ([y] if want_y else [])
        return res[0] if len(res) == 1 else tuple(res)
    if want_mask:
        return y, mask
    return (y, yp) if pool else y


def conv3x3_pl_fused_first(x_nchw: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w_packed: torch.Tensor,
                           bias: Optional[torch.Tensor], cout: int, relu: bool = True, pool: bool = False,
                           range_flag: Optional[torch.Tensor] = None):
    """e11 + e12 (+pool) of the planar path in one launch (wsu_conv3x3_pl_fused_first_fwd): x_nchw (N,1,H,W) fp32 -> y planar [, y_pool]."""
    lib = _lib.load()
    w1 = w1.detach().contiguous()
    _dev_check(x_nchw, w1, b1, w_packed, bias)
    n, cin, h, w = x_nchw.shape
    assert cin == 1 and tuple(w1.shape) == (64, 1, 3, 3) and x_nchw.dtype == torch.float32 and x_nchw.is_contiguous()
    # the fused kernel multiplies e4m3 cross terms: it reads the 36 KB (block, chunk) slices of pack_conv3x3(mode f16f8), not the fp4 packing
    assert w_packed.numel() * w_packed.element_size() == int(lib.wsu_conv3x3_packed_bytes(64, cout, _lib.MODE_F16F8)), \
        "conv3x3_pl_fused_first needs weights from pack_conv3x3(w, mode_id('f16f8'))"
    y = torch.empty(planar_shape(n, cout, h, w), dtype=torch.float32, device=x_nchw.device)
    yp = torch.empty(planar_shape(n, cout, h // 2, w // 2), dtype=torch.float32, device=x_nchw.device) if pool else None
    act = n * h * w * cout + (n * (h // 2) * (w // 2) * cout if pool else 0)
    meta = {"flops": 2.0 * 9 * 64 * cout * n * h * w,
            "bytes": float(n * h * w * 4 + act * 3 + 9 * 64 * cout * 4), "bytes_2B": float(n * h * w * 4 + act * 2 + 9 * 64 * cout * 2),
            "tiles": n * ((h + 15) // 16) * ((w + 31) // 32) * (cout // 64), "steps_per_tile": 4}
    check(_launch("conv3x3_pl", meta, lambda: lib.wsu_conv3x3_pl_fused_first_fwd(
        x_nchw.data_ptr(), w1.data_ptr(), _ptr(b1), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), _ptr(yp),
        n, h, w, cout, int(relu), _ptr(range_flag), _stream())), "wsu_conv3x3_pl_fused_first_fwd")
    return (y, yp) if pool else y


def convt2x2_pl(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
                range_flag: Optional[torch.Tensor] = None, y_format: int = PLANAR_A):
    """nn.ConvTranspose2d(k=2, s=2) + bias on planar F16F8P activations (wsu_convt2x2_pl_fwd); w_packed from pack_convt2x2(mode f16f8).
    y_format=PLANAR_Q: the result is a PlanarQ (the input of conv3x3_q)."""
    lib = _lib.load()
    _dev_check(x, w_packed, bias)
    assert x.dtype == torch.float32 and x.dim() == 6 and x.shape[2] == PLANAR_PLANES and x.shape[5] == 4 and x.is_contiguous()
    n, nch, _, h, w, _ = x.shape
    cin = nch * 16
    y = _planar_out(y_format, n, cout, 2 * h, 2 * w, x.device)
    meta = {"flops": 2.0 * 4 * cin * cout * n * h * w, "bytes": float(n * h * w * (cin + 4 * cout) * 3 + 4 * cin * cout * 4),
            "bytes_2B": float(n * h * w * (cin + 4 * cout) * 2 + 4 * cin * cout * 2),
            "tiles": n * ((h + 3) // 4) * ((w + 31) // 32) * (cout // 64), "steps_per_tile": cin // 32}
    check(_launch("convt2x2_pl", meta, lambda: lib.wsu_convt2x2_pl_fwd(
        x.data_ptr(), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), n, h, w, cin, cout, y_format, _ptr(range_flag), _stream())), "wsu_convt2x2_pl_fwd")
    return y


def relu_mask_alloc(n: int, c: int, h: int, w: int, device) -> torch.Tensor:
    """A relu_mask plane (include/wsu.h): uint8 (N, C/8, 16 * ceil(h / 16), 32 * ceil(w / 32)); rows / columns beyond the image are padding
    that nothing reads as a mask of a stored pixel -- zeroed so that the allocation is deterministic."""
    return torch.zeros((n, c // 8, (h + 15) // 16 * 16, (w + 31) // 32 * 32), dtype=torch.uint8, device=device)


def conv3x3_first_pl(x_nchw: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = True,
                     range_flag: Optional[torch.Tensor] = None, want_mask: bool = False, y_format: int = PLANAR_A):
    """First layer (N, cin <= 8, H, W) fp32 -> planar F16F8P tensor with w.shape[0] channels (wsu_conv3x3_first_pl_fwd) [, its relu_mask plane];
    y_format=PLANAR_Q: a PlanarQ; y_format=PLANAR_H: a PlanarH."""
    lib = _lib.load()
    w = w.detach().contiguous()
    _dev_check(x_nchw, w, bias)
    n, cin, h, wd = x_nchw.shape
    cout = w.shape[0]
    assert x_nchw.dtype == torch.float32 and x_nchw.is_contiguous() and w.shape[1] == cin
    y = _planar_out(y_format, n, cout, h, wd, x_nchw.device)
    mask = relu_mask_alloc(n, cout, h, wd, x_nchw.device) if want_mask else None
    meta = {"flops": 2.0 * 9 * cin * cout * n * h * wd, "bytes": float(n * h * wd * (cin * 4 + cout * (2 if y_format == PLANAR_H else 3))),
            "bytes_2B": float(n * h * wd * (cin * 4 + cout * 2))}
    check(_launch("conv3x3_first_pl", meta, lambda: lib.wsu_conv3x3_first_pl_fwd(
        x_nchw.data_ptr(), w.data_ptr(), _ptr(bias), y.data_ptr(), n, h, wd, cin, cout, int(relu), y_format, _ptr(range_flag), _ptr(mask), _stream())), "wsu_conv3x3_first_pl_fwd")
    return (y, mask) if want_mask else y


def pack_conv3x3_ring(w: torch.Tensor) -> torch.Tensor:
    """The four border-ring weight sets of the planar data gradient (wsu_conv3x3_pack_ring)."""
    lib = _lib.load()
    w = w.detach()
    _dev_check(w)
    cout, cin = w.shape[:2]
    out = torch.empty(4 * lib.wsu_conv3x3_packed_bytes(cin, cout, MODE_F16F8), dtype=torch.uint8, device=w.device)
    check(lib.wsu_conv3x3_pack_ring(w.data_ptr(), out.data_ptr(), cin, cout, _stream()), "wsu_conv3x3_pack_ring")
    return out


PRODUCTS = {"f16f8": 0, "f16": 1}                     # wsu.h WSU_PRODUCTS_F16F8 / WSU_PRODUCTS_F16


def products_id(name: str) -> int:
    if name not in PRODUCTS:
        raise ValueError(f"products must be one of {sorted(PRODUCTS)} (got {name!r})")
    return PRODUCTS[name]


def conv3x3_pl_bwd_data(g: torch.Tensor, w_packed_dgrad: torch.Tensor, w_packed_ring: Optional[torch.Tensor], cin: int, csplit: int,
                        mask1: Optional[torch.Tensor] = None, mask2: Optional[torch.Tensor] = None, pad_zero: bool = False,
                        mask1_bits: Optional[torch.Tensor] = None, mask2_bits: Optional[torch.Tensor] = None, products: str = "f16f8"):
    """Data gradient of the 3x3 conv on planar tensors (wsu_conv3x3_pl_bwd_data).  g: planar gradient (N, Cout/16, 3, H, W, 4); returns
    dx1 (csplit channels) and dx2 (cin - csplit channels, or None), planar gradients.  products: 'f16f8' | 'f16' (wsu.h WSU_PRODUCTS_*)."""
    lib = _lib.load()
    _dev_check(g, w_packed_dgrad, w_packed_ring, mask1, mask2, mask1_bits, mask2_bits)
    assert g.dtype == torch.float32 and g.dim() == 6 and g.shape[2] == PLANAR_PLANES and g.is_contiguous()
    n, nch, _, h, w, _ = g.shape
    for mb, cm in ((mask1_bits, csplit), (mask2_bits, cin - csplit)):
        assert mb is None or (mb.dtype == torch.uint8 and mb.is_contiguous() and tuple(mb.shape) == (n, cm // 8, (h + 15) // 16 * 16, (w + 31) // 32 * 32)), "relu_mask plane shape"
    cout = nch * 16
    dx1 = torch.empty(planar_shape(n, csplit, h, w), dtype=torch.float32, device=g.device)
    dx2 = torch.empty(planar_shape(n, cin - csplit, h, w), dtype=torch.float32, device=g.device) if csplit < cin else None
    nbytes = 0 if pad_zero else lib.wsu_conv3x3_pl_bwd_data_workspace_bytes(n, h, w, cin, cout)
    ws = workspace(nbytes, g.device) if nbytes else None
    meta = {"flops": 2.0 * 9 * cin * cout * n * h * w, "bytes": float(n * h * w * (cin * 5 + cout * (2 if products == "f16" else 3)))}
    check(_launch("conv3x3_pl_bwd_data", meta, lambda: lib.wsu_conv3x3_pl_bwd_data(
        g.data_ptr(), w_packed_dgrad.data_ptr(), _ptr(w_packed_ring), _ptr(ws), 0 if ws is None else ws.numel() * 4,
        dx1.data_ptr(), _ptr(dx2), csplit, _ptr(mask1), _ptr(mask2), _ptr(mask1_bits), _ptr(mask2_bits), n, h, w, cin, cout, int(pad_zero),
        products_id(products), _stream())), "wsu_conv3x3_pl_bwd_data")
    return dx1, dx2


def conv3x3_pl_bwd_weight(g: torch.Tensor, x1: torch.Tensor, x2: Optional[torch.Tensor], want_bias: bool = True, products: str = "f16f8"):
    """Weight / bias gradient of the 3x3 conv on planar operands (wsu_conv3x3_pl_bwd_weight): g planar gradient, x1 / x2 planar inputs.
    products: 'f16f8' | 'f16' (wsu.h WSU_PRODUCTS_*)."""
    lib = _lib.load()
    _dev_check(g, x1, x2)
    n, nco, _, h, w, _ = g.shape
    cout, c1 = nco * 16, x1.shape[1] * 16
    c2 = 0 if x2 is None else x2.shape[1] * 16
    dw = torch.empty((cout, c1 + c2, 3, 3), dtype=torch.float32, device=g.device)
    db = torch.empty(cout, dtype=torch.float32, device=g.device) if want_bias else None
    ws = workspace(lib.wsu_wgrad_workspace_bytes(cout, c1 + c2, 9), g.device)
    meta = {"flops": 2.0 * 9 * (c1 + c2) * cout * n * h * w,
            "bytes": float(n * h * w * (2 if products == "f16" else 3) * (cout * ((c1 + c2) // 64) + (c1 + c2) * (cout // 64)))}
    check(_launch("conv3x3_pl_bwd_weight", meta, lambda: lib.wsu_conv3x3_pl_bwd_weight(
        g.data_ptr(), x1.data_ptr(), _ptr(x2), dw.data_ptr(), _ptr(db), ws.data_ptr(), ws.numel() * 4,
        n, h, w, c1, c2, cout, products_id(products), _stream())), "wsu_conv3x3_pl_bwd_weight")
    return dw, db


def convt2x2_pl_bwd_weight(x: torch.Tensor, dy: torch.Tensor, want_bias: bool = True, products: str = "f16f8"):
    """Weight / bias gradient of the transposed conv on planar operands: x planar input (N, Cin/16, 3, h, w, 4), dy planar gradient at (2h, 2w)."""
    lib = _lib.load()
    _dev_check(x, dy)
    n, nci, _, h, w, _ = x.shape
    cin, cout = nci * 16, dy.shape[1] * 16
    assert dy.shape[3] == 2 * h and dy.shape[4] == 2 * w
    dw = torch.empty((cin, cout, 2, 2), dtype=torch.float32, device=x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if want_bias else None
    ws = workspace(lib.wsu_wgrad_workspace_bytes(cin, cout, 4), x.device)
    meta = {"flops": 2.0 * 4 * cin * cout * n * h * w, "bytes": float(n * h * w * 3 * (cin * (cout // 64) + 4 * cout * (cin // 64)))}
    check(_launch("convt2x2_pl_bwd_weight", meta, lambda: lib.wsu_convt2x2_pl_bwd_weight(
        x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _ptr(db), ws.data_ptr(), ws.numel() * 4, n, h, w, cin, cout, products_id(products), _stream())), "wsu_convt2x2_pl_bwd_weight")
    return dw, db


def pack_convt2x2_pl_dgrad(w: torch.Tensor) -> torch.Tensor:
    """w: (Cin, Cout, 2, 2) -> data-gradient weights of the planar transposed conv (wsu_convt2x2_pl_pack_dgrad)."""
    lib = _lib.load()
    w = w.detach()
    _dev_check(w)
    cin, cout = w.shape[:2]
    out = torch.empty(cin * cout * 16, dtype=torch.uint8, device=w.device)
    check(lib.wsu_convt2x2_pl_pack_dgrad(w.data_ptr(), out.data_ptr(), cin, cout, _stream()), "wsu_convt2x2_pl_pack_dgrad")
    return out


def convt2x2_pl_bwd_data(dy: torch.Tensor, w_packed_dgrad: torch.Tensor, cin: int, mask: Optional[torch.Tensor], products: str = "f16f8") -> torch.Tensor:
    """dy: planar gradient (N, Cout/16, 3, 2h, 2w, 4) -> dx planar gradient with cin channels at (h, w), masked by (mask > 0)."""
    lib = _lib.load()
    _dev_check(dy, w_packed_dgrad, mask)
    n, nco, _, oh, ow, _ = dy.shape
    h, w, cout = oh // 2, ow // 2, nco * 16
    dx = torch.empty(planar_shape(n, cin, h, w), dtype=torch.float32, device=dy.device)
    meta = {"flops": 2.0 * 4 * cin * cout * n * h * w, "bytes": float(n * h * w * (cout * 12 + cin * 5))}
    check(_launch("convt2x2_pl_bwd_data", meta, lambda: lib.wsu_convt2x2_pl_bwd_data(
        dy.data_ptr(), w_packed_dgrad.data_ptr(), dx.data_ptr(), _ptr(mask), n, h, w, cin, cout, products_id(products), _stream())), "wsu_convt2x2_pl_bwd_data")
    return dx


def maxpool2x2_pl_bwd(skip_g: Optional[torch.Tensor], dy_pool: torch.Tensor, act: torch.Tensor, products: str = "f16f8") -> torch.Tensor:
    """(skip_g + routed dy_pool) * (act > 0) on planar tensors; writes into skip_g when given.  products 'f16': the gradient tensors carry no
    residual plane (wsu.h, K7p notes)."""
    lib = _lib.load()
    _dev_check(skip_g, dy_pool, act)
    n, nch, _, h, w, _ = act.shape
    g = skip_g if skip_g is not None else torch.empty_like(act)
    gb = 2 if products == "f16" else 3                     # bytes per gradient element
    meta = {"bytes": float(n * nch * 16 * h * w * (3 + gb + gb / 4 + (gb if skip_g is not None else 0)))}
    check(_launch("maxpool2x2_pl_bwd", meta, lambda: lib.wsu_maxpool2x2_pl_bwd(
        _ptr(skip_g), dy_pool.data_ptr(), act.data_ptr(), g.data_ptr(), n, h, w, nch * 16, products_id(products), _stream())), "wsu_maxpool2x2_pl_bwd")
    return g


def conv1x1_sigmoid_pl_bwd(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, products: str = "f16f8"):
    """Head backward on a planar input: returns g (planar gradient), dw (cout, C, 1, 1), db (cout)."""
    lib = _lib.load()
    w2 = w.detach().reshape(w.shape[0], -1).contiguous()
    _dev_check(x, w2, out, dout)
    n, nch, _, h, wd, _ = x.shape
    c, cout = nch * 16, w2.shape[0]
    g = torch.empty_like(x)
    dw = torch.empty((cout, c, 1, 1), dtype=torch.float32, device=x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device)
    ws = workspace(lib.wsu_head_pl_bwd_workspace_bytes(c, cout), x.device)
    meta = {"bytes": float(n * h * wd * (c * (5 if products == "f16" else 6) + cout * 8))}
    check(_launch("conv1x1_sigmoid_pl_bwd", meta, lambda: lib.wsu_conv1x1_sigmoid_pl_bwd(
        x.data_ptr(), w2.data_ptr(), out.data_ptr(), dout.data_ptr(), g.data_ptr(), dw.data_ptr(), db.data_ptr(),
        ws.data_ptr(), ws.numel() * 4, n, h, wd, c, cout, products_id(products), _stream())), "wsu_conv1x1_sigmoid_pl_bwd")
    return g, dw, db


def colsum_pl(g: torch.Tensor, products: str = "f16f8") -> torch.Tensor:
    """Per-channel sums of a planar gradient."""
    lib = _lib.load()
    _dev_check(g)
    n, nch, _, h, w, _ = g.shape
    c = nch * 16
    db = torch.empty(c, dtype=torch.float32, device=g.device)
    ws = workspace(lib.wsu_chansum_pl_workspace_bytes(c), g.device)
    check(_launch("colsum_pl", {"bytes": float(n * c * h * w * 3)}, lambda: lib.wsu_colsum_pl(
        g.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel() * 4, n, h, w, c, products_id(products), _stream())), "wsu_colsum_pl")
    return db


def conv3x3_first_pl_bwd_weight(g: torch.Tensor, x_nchw: torch.Tensor, want_bias: bool = True, products: str = "f16f8"):
    """First-layer weight / bias gradient from a planar gradient; single input plane."""
    lib = _lib.load()
    _dev_check(g, x_nchw)
    n, nch, _, h, w, _ = g.shape
    c = nch * 16
    if x_nchw.shape[1] != 1:
        raise ValueError("the planar training path handles single-plane inputs (in_channels = 1); use train_mode 'f32' / 'bf16x3' otherwise")
    dw = torch.empty((c, 1, 3, 3), dtype=torch.float32, device=g.device)
    db = torch.empty(c, dtype=torch.float32, device=g.device) if want_bias else None
    ws = workspace(lib.wsu_chansum_pl_workspace_bytes(c), g.device)
    check(_launch("conv3x3_first_pl_bwd_weight", {"bytes": float(n * h * w * (c * (2 if products == "f16" else 3) + 4))}, lambda: lib.wsu_conv3x3_first_pl_bwd_weight(
        g.data_ptr(), x_nchw.data_ptr(), dw.data_ptr(), _ptr(db), ws.data_ptr(), ws.numel() * 4, n, h, w, c, products_id(products), _stream())),
        "wsu_conv3x3_first_pl_bwd_weight")
    return dw, db


def conv3x3_first_pl_bwd_weight_planes(g: torch.Tensor, x_nchw: torch.Tensor, want_bias: bool = True, products: str = "f16f8"):
    """First-layer weight / bias gradient from a planar gradient for an input of 1..8 planes (wsu_conv3x3_first_pl_bwd_weight_planes):
    g planar (N, C/16, 3, H, W, 4), x_nchw (N, cin, H, W) fp32 -> dw (C, cin, 3, 3), db (C) or None."""
    lib = _lib.load()
    x_nchw = x_nchw.contiguous()
    _dev_check(g, x_nchw)
    n, nch, _, h, w, _ = g.shape
    c, cin = nch * 16, x_nchw.shape[1]
    if x_nchw.dtype != torch.float32 or tuple(x_nchw.shape) != (n, cin, h, w):
        raise ValueError(f"conv3x3_first_pl_bwd_weight_planes: x_nchw must be ({n}, cin, {h}, {w}) float32, got {tuple(x_nchw.shape)} {x_nchw.dtype}")
    dw = torch.empty((c, cin, 3, 3), dtype=torch.float32, device=g.device)
    db = torch.empty(c, dtype=torch.float32, device=g.device) if want_bias else None
    ws = workspace(lib.wsu_conv3x3_first_pl_bwd_weight_planes_workspace_bytes(cin, c), g.device)
    reads = 1 if cin <= 4 else 2                            # passes over g (4 planes each)
    meta = {"bytes": float(n * h * w * (reads * c * (2 if products == "f16" else 3) + 4 * cin))}
    check(_launch("conv3x3_first_pl_bwd_weight_planes", meta, lambda: lib.wsu_conv3x3_first_pl_bwd_weight_planes(
        g.data_ptr(), x_nchw.data_ptr(), dw.data_ptr(), _ptr(db), ws.data_ptr(), ws.numel() * 4, n, h, w, cin, c, products_id(products), _stream())),
        "wsu_conv3x3_first_pl_bwd_weight_planes")
    return dw, db


def conv3x3_first_pl_bwd_data(g: torch.Tensor, w: torch.Tensor, products: str = "f16f8") -> torch.Tensor:
    """Input gradient of the first layer from a planar gradient (wsu_conv3x3_first_pl_bwd_data): g planar (N, C/16, 3, H, W, 4), w (C, cin, 3, 3)
    -> dx (N, cin, H, W) fp32 in g's scale."""
    lib = _lib.load()
    w = w.detach().contiguous()
    _dev_check(g, w)
    n, nch, _, h, wd, _ = g.shape
    c, cin = nch * 16, w.shape[1]
    assert tuple(w.shape) == (c, cin, 3, 3)
    dx = torch.empty((n, cin, h, wd), dtype=torch.float32, device=g.device)
    check(_launch("conv3x3_first_pl_bwd_data", {"bytes": float(n * h * wd * (c * (2 if products == "f16" else 3) + 4 * cin))}, lambda: lib.wsu_conv3x3_first_pl_bwd_data(
        g.data_ptr(), w.data_ptr(), dx.data_ptr(), n, h, wd, cin, c, products_id(products), _stream())), "wsu_conv3x3_first_pl_bwd_data")
    return dx


def pack_conv3x3_wino(w: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 -> Winograd F(2,3) packed weights of wsu_conv3x3_wino_fwd (mode bf16x3)."""
    lib = _lib.load()
    w = w.detach().contiguous().float()
    _dev_check(w)
    cout, cin = w.shape[0], w.shape[1]
    nbytes = lib.wsu_conv3x3_wino_packed_bytes(cin, cout)
    if nbytes == 0:
        raise _lib.WsuError(f"Winograd packing needs cin % 16 == 0 and cout % 64 == 0 (got {cin}, {cout})")
    wp = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    check(lib.wsu_conv3x3_wino_pack(w.data_ptr(), wp.data_ptr(), cin, cout, _stream()), "wsu_conv3x3_wino_pack")
    return wp


def conv3x3_wino(x1: torch.Tensor, x2: Optional[torch.Tensor], w_packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
                 relu: bool = True, pool: bool = False, pool_idx: bool = False,
                 head_w: Optional[torch.Tensor] = None, head_b: Optional[torch.Tensor] = None, want_logit: bool = False, want_y: bool = True):
    """3x3 reflect conv (+ReLU, +pool, +head) in mode bf16x3 through the Winograd kernel.  Returns y [, y_pool [, idx]] or,
    with head_w, out [, logit][, y] like conv3x3_head."""
    lib = _lib.load()
    hw2 = None if head_w is None else head_w.detach().reshape(head_w.shape[0], -1)
    _dev_check(x1, x2, w_packed, bias, hw2, head_b)
    assert x1.dtype == torch.float32
    n, h, w, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[3]
    y = torch.empty((n, h, w, cout), dtype=torch.float32, device=x1.device) if (want_y or hw2 is None) else None
    yp = torch.empty((n, h // 2, w // 2, cout), dtype=torch.float32, device=x1.device) if pool else None
    idx = torch.empty((n, h // 2, w // 2, cout), dtype=torch.uint8, device=x1.device) if (pool and pool_idx) else None
    hc = 0 if hw2 is None else hw2.shape[0]
    out = torch.empty((n, hc, h, w), dtype=torch.float32, device=x1.device) if hc else None
    logit = torch.empty_like(out) if (hc and want_logit) else None
    meta = {"flops": 2.0 * 9 * (c1 + c2) * cout * n * h * w,
            "bytes": float(n * h * w * ((c1 + c2) * 4 + (cout * 4 if y is not None else hc * 4)) + 9 * (c1 + c2) * cout * 4
                           + (n * (h // 2) * (w // 2) * cout * 4 if pool else 0))}
    check(_launch("conv3x3", meta, lambda: lib.wsu_conv3x3_wino_fwd(
        x1.data_ptr(), _ptr(x2), w_packed.data_ptr(), _ptr(bias), _ptr(y), _ptr(yp), _ptr(idx),
        _ptr(hw2), _ptr(head_b), _ptr(out), _ptr(logit), hc, n, h, w, c1, c2, cout, int(relu), _stream())), "wsu_conv3x3_wino_fwd")
    if hc:
        res = [out] + ([logit] if want_logit else []) + ([y] if want_y else [])
        return res[0] if len(res) == 1 else tuple(res)
    if pool:
        return (y, yp, idx) if pool_idx else (y, yp)
    return y


def conv3x3_first(x_nchw: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], mode: int, relu: bool = True) -> torch.Tensor:
    lib = _lib.load()
    _dev_check(x_nchw, w, bias)
    n, cin, h, wd = x_nchw.shape
    cout = w.shape[0]
    assert x_nchw.dtype == torch.float32 and w.dtype == torch.float32 and w.shape[1] == cin
    y = torch.empty((n, h, wd, cout), dtype=act_dtype(mode), device=x_nchw.device)
    esz = 2 if mode == MODE_BF16 else 4
    meta = {"flops": 2.0 * 9 * cin * cout * n * h * wd, "bytes": float(n * h * wd * (cin * 4 + cout * esz))}
    check(_launch("conv3x3_first", meta, lambda: lib.wsu_conv3x3_first_fwd(
        x_nchw.data_ptr(), w.data_ptr(), _ptr(bias), y.data_ptr(), n, h, wd, cin, cout, mode, int(relu), _stream())),
        "wsu_conv3x3_first_fwd")
    return y


def maxpool2x2(x: torch.Tensor, mode: int, want_idx: bool = False):
    lib = _lib.load()
    _dev_check(x)
    n, h, w, c = x.shape
    y = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
    idx = torch.empty((n, h // 2, w // 2, c), dtype=torch.uint8, device=x.device) if want_idx else None
    check(lib.wsu_maxpool2x2_fwd(x.data_ptr(), y.data_ptr(), _ptr(idx), n, h, w, c, mode, _stream()), "wsu_maxpool2x2_fwd")
    return (y, idx) if want_idx else y


def convt2x2(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int, mode: int) -> torch.Tensor:
    lib = _lib.load()
    _dev_check(x, w_packed, bias)
    n, h, w = x.shape[:3]
    cin = logical_channels(x, mode)
    y = torch.empty((n, 2 * h, 2 * w, store_channels(cout, mode)), dtype=x.dtype, device=x.device)
    esz = _esz(mode)
    meta = {"flops": 2.0 * 4 * cin * cout * n * h * w, "bytes": float(n * h * w * (cin + 4 * cout) * esz + 4 * cin * cout * 4)}
    check(_launch("convt2x2", meta, lambda: lib.wsu_convt2x2_fwd(
        x.data_ptr(), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), n, h, w, cin, cout, mode, _stream())), "wsu_convt2x2_fwd")
    return y


def conv1x1_sigmoid(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], mode: int, want_logit: bool = False):
    """x: (N,H,W,C) NHWC; w: (Cout, C[,1,1]) fp32; returns NCHW fp32 (N,Cout,H,W)."""
    lib = _lib.load()
    w2 = w.detach().reshape(w.shape[0], -1)
    _dev_check(x, w2, bias)
    n, h, wd, c = x.shape
    cout = w2.shape[0]
    out = torch.empty((n, cout, h, wd), dtype=torch.float32, device=x.device)
    logit = torch.empty_like(out) if want_logit else None
    esz = 2 if mode == MODE_BF16 else 4
    meta = {"flops": 2.0 * c * cout * n * h * wd, "bytes": float(n * h * wd * (c * esz + cout * 4))}
    check(_launch("conv1x1_sigmoid", meta, lambda: lib.wsu_conv1x1_sigmoid_fwd(
        x.data_ptr(), w2.data_ptr(), _ptr(bias), out.data_ptr(), _ptr(logit), n, h, wd, c, cout, mode, _stream())),
        "wsu_conv1x1_sigmoid_fwd")
    return (out, logit) if want_logit else out


def uniform_dropout(x: torch.Tensor, mask: Optional[torch.Tensor], channel: int = 0, keep_prob: float = 1.0,
                    seed: int = 0, want_mask: bool = False):
    """Out of place: returns y (and the mask used)."""
    lib = _lib.load()
    _dev_check(x, mask)
    n, c, h, w = x.shape
    assert x.dtype == torch.float32
    y = torch.empty_like(x)
    mo = torch.empty((n, 1, h, w), dtype=torch.float32, device=x.device) if want_mask else None
    check(lib.wsu_uniform_dropout_fwd(x.data_ptr(), y.data_ptr(), _ptr(mask), _ptr(mo), n, c, h, w, channel,
                                      float(keep_prob), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()), "wsu_uniform_dropout_fwd")
    return (y, mo) if want_mask else y


def ws_residual_stats(x_u8: torch.Tensor, y01: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x_u8: (N,H,W) uint8; y01: (N,H,W) or (N,1,H,W) fp32 -> (beta_hat[N], l1[N]) fp32."""
    lib = _lib.load()
    _dev_check(x_u8, y01)
    n, h, w = x_u8.shape
    assert x_u8.dtype == torch.uint8 and y01.dtype == torch.float32 and y01.numel() == n * h * w
    beta = torch.empty(n, dtype=torch.float32, device=x_u8.device)
    l1 = torch.empty(n, dtype=torch.float32, device=x_u8.device)
    check(lib.wsu_ws_residual_stats(x_u8.data_ptr(), y01.data_ptr(), beta.data_ptr(), l1.data_ptr(), n, h, w, _stream()),
          "wsu_ws_residual_stats")
    return beta, l1


_RING = ((0, 0), (0, 1), (0, 2), (1, 2), (2, 2), (2, 1), (2, 0), (1, 0))     # neighbour order of the flattened 8-tap filters


def filter_taps(k, dtype, layout: str, allow: str = "2d") -> Optional[np.ndarray]:
    """A 3x3 linear predictor -> the 9 contiguous host values a C entry point wants, or None for None.  layout "kernel": K[a][b] of
    the reference's (3,3[,1]) NAMED_FILTERS_2D arrays, applied as a true convolution to x[r+1-a][c+1-b] (wsu_ws_attack,
    wsu_filter3x3_valid_f32, wsu_pair_correlation); layout "weights": the weight of x[r-1+a][c-1+b] at [a*3+b], the same numbers
    reversed (wsu_prediction_error, wsu_ae_values).  Always accepted: a (3,3) / (3,3,1) kernel array.  With "8" in `allow` also the
    reference's flattened 8-tap coefficients ((8,) / (8,1), NAMED_FILTERS, neighbour order x00 x01 x02 x12 x22 x21 x20 x10 of
    _defs/filters.py:57-67); with "9" also a (9,) array that is already in `layout`."""
    if k is None:
        return None
    k = np.asarray(k, dtype=dtype)
    if "9" in allow and k.shape == (9,):
        return np.ascontiguousarray(k)
    if "8" in allow and k.size == 8:
        wgt = np.zeros((3, 3), dtype=dtype)
        for tap, (a, b) in zip(k.reshape(8), _RING):
            wgt[a, b] = tap
    else:
        if k.ndim == 3 and k.shape[2] == 1:
            k = k[..., 0]
        if k.shape != (3, 3):
            raise ValueError(f"{'8 flattened taps or a ' if '8' in allow else ''}3x3 single-channel kernel expected, got shape {k.shape}")
        wgt = k[::-1, ::-1]
    return np.ascontiguousarray((wgt if layout == "weights" else wgt[::-1, ::-1]).reshape(9))


def _hat_full(x_hat: torch.Tensor, n: int, h: int, w: int, hat_full: Optional[bool] = None, *others: Optional[torch.Tensor]) -> int:
    """Validate a prediction (and tensors that must match it, such as x_bias): contiguous float32 of N*H*W values (full frames,
    returns 1) or N*(H-2)*(W-2) (interiors, returns 0).  `hat_full` says which one the caller requires; None infers it."""
    for t in (x_hat,) + tuple(o for o in others if o is not None):
        if t.dtype != torch.float32:
            raise ValueError(f"x_hat must be float32, got {t.dtype}")
        if not t.is_contiguous() or t.numel() != x_hat.numel():
            raise ValueError(f"x_hat must be contiguous and x_bias must match it, got {tuple(t.shape)} for {tuple(x_hat.shape)}")
    full, inner = n * h * w, n * (h - 2) * (w - 2)
    if hat_full is None and x_hat.numel() in (full, inner):
        return int(x_hat.numel() == full)
    if hat_full is not None and x_hat.numel() == (full if hat_full else inner):
        return int(bool(hat_full))
    raise ValueError(f"prediction of {tuple(x_hat.shape)} does not match pixels {(n, h, w)}"
                     + ("" if hat_full is None else f" (hat_full={bool(hat_full)})"))


class _CArguments(tuple):
    """C arguments that carry the arrays their pointers belong to (`keep`): those live as long as the arguments do."""


def _ws_source(who: str, x_u8, x_hat, x_bias, pixel_filter, mean_filter, hat_scale, weighted, what: Optional[str] = None, min_side: int = 0):
    """The ONE prediction source and the weights of a WS statistic entry (ws_attack, ws_sequential, ws_ordered*, ws_residual_accumulate),
    checked.  `what` names a statistic that is not defined for weighted=-1 and takes no x_bias (None: K11, which has both); min_side: the
    smallest plane side the wrapper itself refuses.  Returns ((n, h, w), (x_hat pointer, HOST pixel filter, DEVICE per-image filters, HOST
    mean filter, hat_full, hat_scale, weighted)): the order in which the C entries take them, as _CArguments that hold the filters' arrays,
    so they stay alive while the caller holds the arguments, which it does until the launch."""
    weights = (-1, 0, 1) if what is None else (0, 1)
    if int(weighted) not in weights:
        raise ValueError(f"{who}: weighted must be 0 or 1 (weighted=-1 is not defined for {what}), got {weighted}" if what is not None
                         else f"{who}: weighted={weighted} outside {{-1,0,1}}")
    per_image = pixel_filter is not None and np.ndim(pixel_filter) >= 3 and np.shape(pixel_filter)[1:3] == (3, 3)           # (N,3,3[,1])
    if (x_hat is None) == (pixel_filter is None) or (per_image and x_bias is not None):
        raise ValueError(f"{who}: give exactly one of x_hat / pixel_filter")
    _dev_check(x_hat, x_bias)
    n, h, w = _u8_planes(x_u8)
    if h < min_side or w < min_side:
        raise ValueError(f"{who}: planes of at least {min_side} x {min_side} pixels expected, got {h} x {w}")
    mt = filter_taps(mean_filter, np.float32, "kernel")
    pt = pts = None
    hat_full = 1
    if x_hat is not None:
        hat_full = _hat_full(x_hat, n, h, w, None, x_bias)
    elif per_image:
        if len(pixel_filter) != n:
            raise ValueError(f"{who}: {len(pixel_filter)} filters for {n} images")
        pts = torch.from_numpy(np.stack([filter_taps(f, np.float32, "kernel") for f in pixel_filter])).to(x_u8.device)
    else:
        pt = filter_taps(pixel_filter, np.float32, "kernel")
    host = lambda a: None if a is None else a.ctypes.data
    source = _CArguments((_ptr(x_hat), host(pt), _ptr(pts), host(mt), hat_full, float(hat_scale), int(weighted)))
    source.keep = (pt, pts, mt)
    return (n, h, w), source


def _changepoint_outputs(n: int, workspace_bytes: int, dev):
    """(k, t_max, t_all) int64 (N,) and the int64 workspace of a changepoint entry (K27, K33)."""
    k, t_max, t_all = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    return k, t_max, t_all, torch.empty(max(workspace_bytes // 8, 1), dtype=torch.int64, device=dev)


def ws_attack(x_u8: torch.Tensor, x_hat: Optional[torch.Tensor] = None, *, x_bias: Optional[torch.Tensor] = None,
              pixel_filter=None, mean_filter=None, hat_scale: float = 255.0, weighted: int = 1, correct_bias: bool = False,
              return_sums: bool = False):
    """Batched WS payload estimate (wsu_ws_attack, src/ws/estimate.py:55-136).  x_u8: (N,H,W) uint8.
    x_hat: (N,H,W)/(N,1,H,W) full-frame prediction or (N,H-2,W-2) interior prediction, multiplied by `hat_scale`;
    or `pixel_filter` (3,3[,1]) for an in-kernel linear predictor, (N,3,3[,1]) for one per image (wsu_ws_attack_taps).
    Returns beta_hat[N] (and the (N,3) fp64 sums)."""
    lib = _lib.load()
    (n, h, w), source = _ws_source("ws_attack", x_u8, x_hat, x_bias, pixel_filter, mean_filter, hat_scale, weighted)
    xh, pt, pts, mt, hat_full, scale, wgt = source
    beta = torch.empty(n, dtype=torch.float32, device=x_u8.device)
    sums = torch.empty((n, 3), dtype=torch.float64, device=x_u8.device) if return_sums else None
    ws = torch.empty(lib.wsu_ws_attack_workspace_bytes(n) // 8, dtype=torch.float64, device=x_u8.device)
    tail = (int(bool(correct_bias)), beta.data_ptr(), _ptr(sums), ws.data_ptr(), ws.numel() * 8, n, h, w, _stream())
    if pts is not None:
        check(_launch("ws_attack", {}, lambda: lib.wsu_ws_attack_taps(x_u8.data_ptr(), pts, mt, wgt, *tail)), "wsu_ws_attack_taps")
    else:
        check(_launch("ws_attack", {}, lambda: lib.wsu_ws_attack(x_u8.data_ptr(), xh, _ptr(x_bias), pt, mt, hat_full, scale, wgt, *tail)),
              "wsu_ws_attack")
    return (beta, sums) if return_sums else beta


ORDERS = ("rows", "rows_up")               # path orders of the sequential statistic and simulator: rows from the top / from the bottom


def order_id(order) -> int:
    """'rows' -> 0 (row by row from the top), 'rows_up' -> 1 (from the bottom row upwards); anything else raises ValueError."""
    if order not in ORDERS:
        raise ValueError(f"unknown order {order!r}; choose from {ORDERS}")
    return ORDERS.index(order)


def ws_sequential(x_u8: torch.Tensor, x_hat: Optional[torch.Tensor] = None, *, pixel_filter=None, mean_filter=None,
                  hat_scale: float = 255., weighted: int = 1, order: str = "rows", return_curve: bool = False):
    """The WS changepoint of a sequentially placed payload (wsu_ws_sequential, K27).  x_u8: (N,H,W) uint8; the prediction as for
    ws_attack: x_hat (N,H,W)/(N,1,H,W) full frames or (N,H-2,W-2) interiors, multiplied by `hat_scale`, or `pixel_filter` (3,3[,1]) for an
    in-kernel linear predictor, (N,3,3[,1]) for one per image.  weighted: 0 or 1.  order: 'rows' (the path takes the interior rows from
    the top) or 'rows_up' (from the bottom).  Returns int64 (N,) tensors (k, t_max, t_all[, curve (N,H-2)]): the first maximiser k in
    0..(H-2)(W-2) of the fixed-point cumulative statistic T (2^24 units), T(k), T at the path's end, and T at the end of every row."""
    oid = order_id(order)
    lib = _lib.load()
    (n, h, w), source = _ws_source("ws_sequential", x_u8, x_hat, None, pixel_filter, mean_filter, hat_scale, weighted,
                                         "the sequential statistic")
    k, t_max, t_all, ws = _changepoint_outputs(n, lib.wsu_ws_sequential_workspace_bytes(n, h), x_u8.device)
    curve = torch.empty((n, h - 2), dtype=torch.int64, device=x_u8.device) if return_curve else None
    check(_launch("ws_sequential", {"bytes": float(n * h * w * (1 if x_hat is None else 5))}, lambda: lib.wsu_ws_sequential(
        x_u8.data_ptr(), *source, oid, k.data_ptr(), t_max.data_ptr(), t_all.data_ptr(), _ptr(curve), ws.data_ptr(), ws.numel() * 8, n, h, w,
        _stream())), "wsu_ws_sequential")
    return (k, t_max, t_all, curve) if return_curve else (k, t_max, t_all)


def _flip_tau(who: str, flip_rate) -> float:
    """tau = (float32)(flip_rate / 2) of the ordered statistic; flip_rate outside (0, 1] raises ValueError."""
    f = float(flip_rate)
    if not 0.0 < f <= 1.0:
        raise ValueError(f"{who}: flip_rate must lie in (0, 1] (1: every used pixel flipped, 0.5: a real message), got {flip_rate!r}")
    return float(np.float32(f / 2.0))


def _ordered_path(who: str, path, n: int, m: int, dev) -> None:
    if not (isinstance(path, torch.Tensor) and path.dtype == torch.int32 and tuple(path.shape) == (n, m)):
        raise ValueError(f"{who}: path must be an int32 tensor of shape {(n, m)} (one permutation of the interior raster indices per image), "
                         f"got {tuple(path.shape) if isinstance(path, torch.Tensor) else type(path).__name__}"
                         f"{' ' + str(path.dtype) if isinstance(path, torch.Tensor) else ''}")
    _dev_check(path)
    if path.device != dev:
        raise ValueError(f"{who}: path lives on {path.device}, the pixels on {dev}")


def _ordered_arguments(who: str, x_u8, x_hat, pixel_filter, mean_filter, hat_scale, weighted, flip_rate):
    """The checked arguments kernel A of K33 takes: ((n, h, w), _ws_source's C arguments, tau)."""
    tau = _flip_tau(who, flip_rate)
    shape, source = _ws_source(who, x_u8, x_hat, None, pixel_filter, mean_filter, hat_scale, weighted, "the changepoint statistic", min_side=3)
    return shape, source, tau


def ws_ordered_terms(x_u8: torch.Tensor, x_hat: Optional[torch.Tensor] = None, *, pixel_filter=None, mean_filter=None,
                     hat_scale: float = 255., weighted: int = 1, flip_rate: float = 1.0) -> torch.Tensor:
    """Kernel A of K33 alone (wsu_ws_ordered_terms): the fixed-point terms q = ws_seq_term(wgt * (s * res - flip_rate / 2)) of every
    interior pixel, int64 (N, (H-2)(W-2)) in raster order.  Arguments as ws_ordered's."""
    lib = _lib.load()
    (n, h, w), source, tau = _ordered_arguments("ws_ordered_terms", x_u8, x_hat, pixel_filter, mean_filter, hat_scale, weighted, flip_rate)
    terms = torch.empty((n, (h - 2) * (w - 2)), dtype=torch.int64, device=x_u8.device)
    check(_launch("ws_ordered_terms", {"bytes": float(n * h * w * (9 if x_hat is None else 13))}, lambda: lib.wsu_ws_ordered_terms(
        x_u8.data_ptr(), *source, tau, terms.data_ptr(), n, h, w, _stream())), "wsu_ws_ordered_terms")
    return terms


def ws_ordered_fold(terms: torch.Tensor, path: torch.Tensor, h: int, w: int):
    """Kernels B and C of K33 alone (wsu_ws_ordered_fold): terms int64 (N,M) as ws_ordered_terms makes them, path int32 (N,M), M =
    (h-2)(w-2) -> int64 (N,) tensors (k, t_max, t_all) of the cumulative sums of terms[i, path[i, :]]."""
    who = "ws_ordered_fold"
    h, w = int(h), int(w)
    m = (h - 2) * (w - 2)
    if not (isinstance(terms, torch.Tensor) and terms.dtype == torch.int64 and terms.dim() == 2 and terms.shape[1] == m and h >= 3 and w >= 3):
        raise ValueError(f"{who}: terms must be an int64 (N,{m}) tensor for planes of {h} x {w}")
    _dev_check(terms)
    n, dev = terms.shape[0], terms.device
    _ordered_path(who, path, n, m, dev)
    lib = _lib.load()
    k, t_max, t_all, ws = _changepoint_outputs(n, lib.wsu_ws_ordered_fold_workspace_bytes(n, h, w), dev)
    check(_launch("ws_ordered_fold", {"bytes": float(n * m * 12)}, lambda: lib.wsu_ws_ordered_fold(
        terms.data_ptr(), path.data_ptr(), k.data_ptr(), t_max.data_ptr(), t_all.data_ptr(), ws.data_ptr(), ws.numel() * 8, n, h, w,
        _stream())), "wsu_ws_ordered_fold")
    return k, t_max, t_all


def ws_ordered(x_u8: torch.Tensor, path: torch.Tensor, x_hat: Optional[torch.Tensor] = None, *, pixel_filter=None, mean_filter=None,
               hat_scale: float = 255., weighted: int = 1, flip_rate: float = 1.0):
    """The WS changepoint along a given path (wsu_ws_ordered, K33), for payloads placed in the order of an adaptivity criterion.  x_u8:
    (N,H,W) uint8; path: int32 (N,M) on the same device, M = (H-2)(W-2): per image the interior raster indices (r-1)(W-2) + (c-1) in the
    order the path visits them (interior_order makes one from a key plane); an entry outside 0..M-1 contributes nothing.  The prediction
    as for ws_sequential: x_hat (N,H,W)/(N,1,H,W) full frames or (N,H-2,W-2) interiors, multiplied by `hat_scale`, or `pixel_filter`
    (3,3[,1]) for an in-kernel linear predictor, (N,3,3[,1]) for one per image.  weighted: 0 or 1.  flip_rate in (0, 1]: the probability
    that a used pixel was flipped (1: HILLR flips every used pixel; 0.5: a real message, ws_sequential's term).  Returns int64 (N,)
    tensors (k, t_max, t_all): the first maximiser k in 0..M of the fixed-point cumulative statistic T (2^24 units) along the path, T(k)
    and T(M).  The change rate is flip_rate * k / M (ws.adaptive.beta)."""
    lib = _lib.load()
    (n, h, w), source, tau = _ordered_arguments("ws_ordered", x_u8, x_hat, pixel_filter, mean_filter, hat_scale, weighted, flip_rate)
    _ordered_path("ws_ordered", path, n, (h - 2) * (w - 2), x_u8.device)
    k, t_max, t_all, ws = _changepoint_outputs(n, lib.wsu_ws_ordered_workspace_bytes(n, h, w), x_u8.device)
    check(_launch("ws_ordered", {"bytes": float(n * h * w * (29 if x_hat is None else 33))}, lambda: lib.wsu_ws_ordered(
        x_u8.data_ptr(), *source, tau, path.data_ptr(), k.data_ptr(), t_max.data_ptr(), t_all.data_ptr(), ws.data_ptr(), ws.numel() * 8,
        n, h, w, _stream())), "wsu_ws_ordered")
    return k, t_max, t_all


def interior_order(keys: torch.Tensor) -> torch.Tensor:
    """keys: (N,H,W) float32 on the device, e.g. hill_cost's output -> int32 (N,M), M = (H-2)(W-2): per image the interior raster indices
    in ascending order of keys[:, 1:-1, 1:-1], ties to the smaller index: the `path` of ws_ordered.  This is torch.sort(stable=True) on
    the device, not a kernel of this library: the sort is plumbing around K33, and a hand-written one is a follow-up."""
    if not (isinstance(keys, torch.Tensor) and keys.dtype == torch.float32 and keys.dim() == 3 and keys.shape[1] >= 3 and keys.shape[2] >= 3):
        raise ValueError(f"interior_order: an (N,H,W) float32 tensor with H, W >= 3 expected, got "
                         f"{tuple(keys.shape) if isinstance(keys, torch.Tensor) else type(keys).__name__}")
    if not keys.is_cuda:
        raise _lib.WsuError("interior_order sorts on the GPU: got a CPU tensor")
    n = keys.shape[0]
    order = torch.sort(keys[:, 1:-1, 1:-1].reshape(n, -1), dim=1, stable=True).indices
    return order.to(torch.int32).contiguous()


MAX_LOCATE_IMAGES = 65536                  # images one pair of accumulators may hold: |num| < 2^53 and den < 2^53 stay exact in float64


def ws_residual_accumulate(x_u8: torch.Tensor, num: torch.Tensor, den: torch.Tensor, x_hat: Optional[torch.Tensor] = None, *,
                           pixel_filter=None, mean_filter=None, hat_scale: float = 255., weighted: int = 1, parts: int = 0) -> None:
    """Adds a batch's per-pixel WS residual terms to two accumulators (wsu_ws_residual_accumulate, K29).  x_u8: (N,H,W) uint8; the
    prediction as for ws_sequential: x_hat (N,H,W)/(N,1,H,W) full frames or (N,H-2,W-2) interiors, multiplied by `hat_scale`, or
    `pixel_filter` (3,3[,1]) for an in-kernel linear predictor, (N,3,3[,1]) for one per image.  weighted: 0 or 1.  num, den: contiguous
    int64 (H-2,W-2) on x_u8's device; per interior pixel num gains the images' terms wgt * r in 2^-24 units, den their weights in 2^-32
    units, an image whose term is NaN adds to neither.  parts: workgroups sharing a pixel tile's images (0: chosen from the plane size);
    the sums are exact integers and do not depend on it."""
    who = "ws_residual_accumulate"
    lib = _lib.load()
    (n, h, w), source = _ws_source(who, x_u8, x_hat, None, pixel_filter, mean_filter, hat_scale, weighted, "the residual means")
    for name, t in (("num", num), ("den", den)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and tuple(t.shape) == (h - 2, w - 2) and t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be a contiguous int64 tensor of shape {(h - 2, w - 2)} for planes of "
                             f"{(h, w)}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    _dev_check(num, den)
    check(_launch(who, {"bytes": float(n * h * w * (1 if x_hat is None else 5) + 32 * (h - 2) * (w - 2))}, lambda: lib.wsu_ws_residual_accumulate(
        x_u8.data_ptr(), *source, int(parts), num.data_ptr(), den.data_ptr(), n, h, w, _stream())), "wsu_" + who)


MAX_KEY_SEARCH_KEYS = 2 ** 31 - 1          # keys one call of ws_key_search takes
KEY_SEARCH_SUM_LIMIT = 2 ** 62             # sum |num| and sum |den| stay below it, so no masked sum can wrap


def _abs_sum(t: torch.Tensor) -> int:
    """The exact sum of |t| of an int64 tensor as a Python int (the high and the low 32 bits are summed apart: no int64 sum can wrap)."""
    if bool((t == torch.iinfo(torch.int64).min).any()):
        return 2 ** 63 * int((t == torch.iinfo(torch.int64).min).sum())
    a = t.abs()
    return (int((a >> 32).sum()) << 32) + int((a & 0xFFFFFFFF).sum())


def ws_key_search(num: torch.Tensor, den: torch.Tensor, h: int, w: int, *, keys: Optional[torch.Tensor] = None, key_first: Optional[int] = None,
                  count: Optional[int] = None, alpha_threshold: int, rows: Optional[int] = None, parts: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The sums of K29's accumulators over the pixels each of many candidate stego keys selects (wsu_ws_key_search, K35).  num, den: the
    int64 (H-2,W-2) accumulators of ws_residual_accumulate for (h, w) planes; they are padded to zero-bordered (H,W) frames here, since a
    key selects by the pixel's linear index in the frame, exactly as lsbr_key_mask(key, alpha_threshold, h, w) does.  The candidates are
    EITHER `keys`, an int64 (K) device tensor holding 64-bit patterns (as seeds do), OR the range key_first + j, j = 0..count-1, wrapping
    mod 2^64.  alpha_threshold: 0..2^32 (lsbr_key_threshold); a threshold below the embedder's selects a subset of the used pixels.
    rows = R scans the first R frame rows only, a cheap prefilter.  parts: workgroups sharing a key's pixels (0: chosen from K) -- the
    sums are exact integers and do not depend on it.  -> (snum, sden), int64 (K).  Raises ValueError when sum |num| or sum |den| reaches
    2^62: below it no masked sum can wrap."""
    who = "ws_key_search"
    h, w = int(h), int(w)
    if h < 3 or w < 3:
        raise ValueError(f"{who}: a frame of at least 3 x 3 pixels expected, got {h} x {w}")
    for name, t in (("num", num), ("den", den)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and tuple(t.shape) == (h - 2, w - 2)):
            raise ValueError(f"{who}: {name} must be an int64 tensor of shape {(h - 2, w - 2)} for frames of {(h, w)}, got "
                             f"{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if (keys is None) == (key_first is None and count is None):
        raise ValueError(f"{who}: give exactly one of keys and (key_first, count)")
    if keys is None and (key_first is None or count is None):
        raise ValueError(f"{who}: a key range needs both key_first and count")
    thr = int(alpha_threshold)
    if not 0 <= thr <= 2 ** 32:
        raise ValueError(f"{who}: alpha_threshold {alpha_threshold!r} outside 0..2^32 (lsbr_key_threshold)")
    r = h if rows is None else int(rows)
    if not 1 <= r <= h:
        raise ValueError(f"{who}: rows={rows!r} outside 1..{h}")
    if not 0 <= int(parts) <= 65535:
        raise ValueError(f"{who}: parts={parts!r} outside 0 (automatic) .. 65535")
    if keys is not None:
        if not (isinstance(keys, torch.Tensor) and keys.dtype == torch.int64 and keys.dim() == 1 and 1 <= keys.shape[0] <= MAX_KEY_SEARCH_KEYS):
            raise ValueError(f"{who}: keys must be an int64 tensor of 1..2^31-1 64-bit patterns")
        keys = keys.contiguous()
        k, first = keys.shape[0], 0
        _dev_check(num, den, keys)
    else:
        k, first = int(count), int(key_first)
        if not 1 <= k <= MAX_KEY_SEARCH_KEYS:
            raise ValueError(f"{who}: count={count!r} keys outside 1..2^31-1")
        if not 0 <= first < 2 ** 64:
            raise ValueError(f"{who}: key_first {key_first!r} outside [0, 2^64)")
        _dev_check(num, den)
    for name, t in (("num", num), ("den", den)):
        if _abs_sum(t) >= KEY_SEARCH_SUM_LIMIT:
            raise ValueError(f"{who}: the sum of |{name}| is 2^62 or more: a masked sum could wrap")
    lib = _lib.load()
    frames = torch.zeros((2, h, w), dtype=torch.int64, device=num.device)
    frames[0, 1:-1, 1:-1] = num
    frames[1, 1:-1, 1:-1] = den
    snum = torch.empty(k, dtype=torch.int64, device=num.device)
    sden = torch.empty(k, dtype=torch.int64, device=num.device)
    check(_launch("ws_key_search", {"bytes": float(16 * r * w + 16 * k), "keys": float(k)}, lambda: lib.wsu_ws_key_search(
        frames[0].data_ptr(), frames[1].data_ptr(), r * w, keys.data_ptr() if keys is not None else None, first, 0 if keys is not None else 1,
        k, thr, int(parts), snum.data_ptr(), sden.data_ptr(), _stream())), "wsu_ws_key_search")
    return snum, sden


def _count_entry(entry: str, x_u8: torch.Tensor, tail_shape: Tuple[int, ...], *middle, out: Optional[torch.Tensor] = None, after=()) -> torch.Tensor:
    """wsu_<entry>(x, *middle, table, n, h, w, *after, stream), the form of every count entry -> the (N, *tail_shape) int64 table of exact
    sums, which the call zeroes first.  after: what an entry takes behind w (K36's order and T).  out: a tensor of that form to write into;
    it is NOT validated here, the caller has checked its dtype, shape and device."""
    n, h, w = _u8_planes(x_u8)
    if n == 0:
        raise ValueError(f"{entry}: no images")
    symbol = "wsu_" + entry
    fn = getattr(_lib.load(), symbol)
    table = torch.empty((n, *tail_shape), dtype=torch.int64, device=x_u8.device) if out is None else out
    check(_launch(entry, {"bytes": float(n * h * w)}, lambda: fn(
        x_u8.data_ptr(), *middle, table.data_ptr(), n, h, w, *after, _stream())), symbol)
    return table


def ols_moments(x_u8: torch.Tensor) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,45) int64: per image the exact sums of v_i * v_j, i <= j (row-major upper triangle), over the interior
    pixels, v = the eight neighbours in ring order (_RING) and the centre (wsu_ols_moments, K24; ws_unet_amd.ols unpacks and solves)."""
    return _count_entry("ols_moments", x_u8, (45,))


def ols_moments5(x_u8: torch.Tensor) -> torch.Tensor:
    """x_u8: (N,H,W) uint8, H, W >= 5 -> (N,325) int64: per image the exact sums of v_p * v_q, p <= q (row-major upper triangle), over the
    pixels with a full 5x5 window, v = the 24 neighbours in raster order and the centre (wsu_ols_moments5, K56; ws_unet_amd.ols5 unpacks
    and solves)."""
    return _count_entry("ols_moments5", x_u8, (325,))


def predict5x5(x_u8: torch.Tensor, taps: torch.Tensor, want_bias: bool = False):
    """The 5x5 linear prediction of every image as full frames in pixel units (wsu_predict5x5, K57).  x_u8: (N,H,W) uint8, H, W >= 3;
    taps: DEVICE float32 (24,) for every image or (N,24) for one row per image, in K56's variable order.  Returns x_hat float32 (N,H,W)
    -- 0 on the frame border, KB's prediction on the ring inside it, the 24 taps elsewhere -- and with want_bias (x_hat, x_bias), x_bias
    the predictor applied to x_bar - x: what ws_attack takes as x_hat / x_bias with hat_scale = 1."""
    n, h, w = _u8_planes(x_u8)
    if n == 0:
        raise ValueError("predict5x5: no images")
    if not (isinstance(taps, torch.Tensor) and taps.dtype == torch.float32 and tuple(taps.shape) in ((24,), (n, 24))):
        raise ValueError(f"predict5x5: taps must be a float32 tensor of shape (24,) or {(n, 24)}, got "
                         f"{tuple(taps.shape) if isinstance(taps, torch.Tensor) else type(taps).__name__}"
                         f"{' ' + str(taps.dtype) if isinstance(taps, torch.Tensor) else ''}")
    _dev_check(taps)
    if taps.device != x_u8.device:
        raise ValueError(f"predict5x5: taps live on {taps.device}, the pixels on {x_u8.device}")
    lib = _lib.load()
    x_hat = torch.empty((n, h, w), dtype=torch.float32, device=x_u8.device)
    x_bias = torch.empty_like(x_hat) if want_bias else None
    check(_launch("predict5x5", {"bytes": float(n * h * w * (5 + 4 * bool(want_bias)))}, lambda: lib.wsu_predict5x5(
        x_u8.data_ptr(), taps.data_ptr(), int(taps.dim() == 2), x_hat.data_ptr(), _ptr(x_bias), n, h, w, _stream())), "wsu_predict5x5")
    return (x_hat, x_bias) if want_bias else x_hat


def spa_tables(x_u8: torch.Tensor) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,3,128) int64: per image the sample-pairs table over all horizontally and vertically adjacent pixel pairs
    (u,v), indexed by m = |u-v| >> 1: [0] E, |u-v| even; [1] X, odd with max(u,v) even; [2] Y, odd with max(u,v) odd (wsu_spa_tables, K25;
    ws_unet_amd.ws.structural.spa solves)."""
    return _count_entry("spa_tables", x_u8, (3, 128))


def rs_counts(x_u8: torch.Tensor) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,8) int64: per image R_M, S_M, R_-M, S_-M over the groups of 4 consecutive pixels of every row with the
    mask (0,1,1,0), then the same four on the plane with every LSB flipped (wsu_rs_counts, K26; ws_unet_amd.ws.structural.rs solves)."""
    return _count_entry("rs_counts", x_u8, (8,))


HIST_MAX_SEGMENTS = 4096


def hist_segments(x_u8: torch.Tensor, segments: int = 1, order="rows") -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,S,256) int64, S = segments in 1..4096: the histogram of every one of S consecutive segments of the path.
    The path position of pixel (r,c) is t = r W + c for order 'rows' and t = (H-1-r) W + c for 'rows_up' (ORDERS, as in the sequential
    WS statistic); the pixel belongs to segment floor(t S / (H W)), so segment s holds the positions ceil(s H W / S) ..
    ceil((s+1) H W / S) - 1 and is empty where S > H W leaves it none.  segments=1 is the plain histogram; a prefix histogram is
    `.cumsum(1)` (wsu_hist_segments, K58; ws_unet_amd.histogram makes the chi-square curve)."""
    if isinstance(segments, bool) or int(segments) != segments or not 1 <= segments <= HIST_MAX_SEGMENTS:
        raise ValueError(f"hist_segments: segments={segments!r} outside 1..{HIST_MAX_SEGMENTS}")
    return _count_entry("hist_segments", x_u8, (int(segments), 256), after=(int(segments), order_id(order)))


def adjacency_hist(x_u8: torch.Tensor) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,256,256) int64: A[u][v] = the number of (r,c) with c + 1 < W, x[r,c] = u and x[r,c+1] = v, the
    horizontally adjacent pairs only (Ker's adjacency histogram); H (W-1) pairs per image, all zero for W = 1 (wsu_adjacency_hist, K59)."""
    return _count_entry("adjacency_hist", x_u8, (256, 256))


def downsample2x2(x_u8: torch.Tensor) -> torch.Tensor:
    """x_u8: (N,H,W) uint8, H, W >= 2 -> (N,H//2,W//2) uint8: every output pixel is the sum of its 2 x 2 block divided by 4 and rounded
    down; an odd last row or column is dropped (wsu_downsample2x2, K60: Ker's calibration image)."""
    n, h, w = _u8_planes(x_u8)
    if n == 0:
        raise ValueError("downsample2x2: no images")
    if h < 2 or w < 2:
        raise ValueError(f"downsample2x2: planes of {h} x {w} pixels are too small (H, W >= 2)")
    lib = _lib.load()
    y = torch.empty((n, h // 2, w // 2), dtype=torch.uint8, device=x_u8.device)
    check(_launch("downsample2x2", {"bytes": float(n * h * w + y.numel())}, lambda: lib.wsu_downsample2x2(
        x_u8.data_ptr(), y.data_ptr(), n, h, w, _stream())), "wsu_downsample2x2")
    return y


def spam_bins(order: int, T: int) -> int:
    """B^(order+1), B = 2T + 1: the bins of one direction of the SPAM counts; the (order, T) that K36 takes, else ValueError."""
    if order not in (1, 2) or isinstance(T, bool) or int(T) != T or not 1 <= T <= (8 if order == 1 else 4):
        raise ValueError(f"spam: order={order!r} T={T!r}: order must be 1 (T in 1..8) or 2 (T in 1..4)")
    return (2 * int(T) + 1) ** (order + 1)


def spam_counts(x_u8: torch.Tensor, order: int = 2, T: int = 3, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,4,B^(order+1)) int64, B = 2T + 1: per image and direction (right, down, down-right, down-left) the counts of
    the runs of order + 1 clipped differences clip(x[p + k s] - x[p + (k+1) s], -T, T), k = 0..order, along the step s, over every position
    whose order + 2 pixels lie in the image; bin = the differences + T as base-B digits, the first one most significant (wsu_spam_counts,
    K36; ws_unet_amd.spam makes the features).  The defaults are SPAM-686.  `out`: an int64 tensor of that shape to write into (the call
    zeroes it)."""
    bins = spam_bins(order, T)
    n = _u8_planes(x_u8)[0]
    if out is not None and n:
        _dev_check(out)
        if out.dtype != torch.int64 or tuple(out.shape) != (n, 4, bins) or out.device != x_u8.device:
            raise ValueError(f"spam_counts: out must be an int64 tensor of shape {(n, 4, bins)} on {x_u8.device}, got {tuple(out.shape)} {out.dtype}")
    return _count_entry("spam_counts", x_u8, (4, bins), out=out, after=(int(order), int(T)))


# The tables of K49 as data.  SRM_Q2: per residual class its quantisation steps as q2 = 2q, ascending.  SRM_REACH: per class and
# (residual, scan) the (a, b) of the table's total max(H - a, 0) max(W - b, 0).  SRM_TABLES: the 44 tables in the order of the counts,
# (class, q2, residual, scan, a, b): for class; for q ascending; for residual in (h, v) or the one n; for scan in (h, v).
SRM_T, SRM_ORDER, SRM_BINS = 2, 4, 625
SRM_Q2 = {"S1": (2, 4), "S2": (4, 6, 8), "S3": (6, 9, 12), "S3x3": (8, 12, 16), "S5x5": (24, 36, 48)}
SRM_REACH = {"S1": {("h", "h"): (0, 4), ("h", "v"): (3, 1), ("v", "h"): (1, 3), ("v", "v"): (4, 0)},
             "S2": {("h", "h"): (0, 5), ("h", "v"): (3, 2), ("v", "h"): (2, 3), ("v", "v"): (5, 0)},
             "S3": {("h", "h"): (0, 6), ("h", "v"): (3, 3), ("v", "h"): (3, 3), ("v", "v"): (6, 0)},
             "S3x3": {("n", "h"): (2, 5), ("n", "v"): (5, 2)},
             "S5x5": {("n", "h"): (4, 7), ("n", "v"): (7, 4)}}
SRM_TABLES = tuple((cls, q2, res, scan, *ab) for cls, steps in SRM_Q2.items() for q2 in steps for (res, scan), ab in SRM_REACH[cls].items())


def _set_counts(entry: str, tables, x_u8: torch.Tensor, out: Optional[torch.Tensor], *middle) -> torch.Tensor:
    """the count entry `entry` of the SRM, one row of SRM_BINS per table of `tables`, with `out` validated; middle: as _count_entry's"""
    n = _u8_planes(x_u8)[0]
    shape = (n, len(tables), SRM_BINS)
    if out is not None and n:
        _dev_check(out)
        if out.dtype != torch.int64 or tuple(out.shape) != shape or out.device != x_u8.device:
            raise ValueError(f"{entry}: out must be an int64 tensor of shape {shape} on {x_u8.device}, got {tuple(out.shape)} {out.dtype}")
    return _count_entry(entry, x_u8, shape[1:], *middle, out=out)


def _set_tables(q2, sets):
    """the tables of a min/max count kernel in the order of its counts, (class, q2, set, scan, a, b) with the table's total
    2 max(H - a, 0) max(W - b, 0): for class; for q2 ascending; for set; for scan in (h, v)"""
    return tuple((cls, q, name, scan, u + dn + (3 if scan == "v" else 0), l + rt + (3 if scan == "h" else 0))
                 for cls, steps in q2.items() for q in steps for name, (u, dn, l, rt) in sets[cls].items() for scan in "hv")


def srm_counts(x_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,44,625) int64: per image the co-occurrence counts of the linear submodels of the spatial rich model, table
    by table as SRM_TABLES lists them: the runs of four digits -2..2 of one linear residual at one quantisation step along a row or down
    a column, over every run whose pixels all lie in the image; bin = the digits + 2 in base 5, the first one most significant
    (wsu_srm_counts, K49, which include/wsu.h defines; ws_unet_amd.srm makes the features).  `out`: an int64 tensor of that shape to write
    into (the call zeroes it)."""
    return _set_counts("srm_counts", SRM_TABLES, x_u8, out)


def srm_weighted_counts(x_u8: torch.Tensor, weights: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x_u8: (N,H,W) uint8, weights: (N,H,W) uint16 -> (N,44,625) int64: the tables of srm_counts with every counted run adding the
    largest of the weights at its four residual positions instead of 1 (wsu_srm_weighted_counts, K52, which include/wsu.h defines: the
    integer half of the selection-channel-aware features of ws_unet_amd.srm; change_weights makes a sender's weights).  Weights all 1
    give srm_counts.  `out`: an int64 tensor of that shape to write into (the call zeroes it)."""
    _u8_planes(x_u8)
    _dev_check(weights)
    if weights.dtype != torch.uint16 or weights.shape != x_u8.shape or weights.device != x_u8.device:
        raise ValueError(f"srm_weighted_counts: weights must be uint16 of shape {tuple(x_u8.shape)} on {x_u8.device}, got "
                         f"{tuple(weights.shape)} {weights.dtype} on {weights.device}")
    return _set_counts("srm_weighted_counts", SRM_TABLES, x_u8, out, weights.data_ptr())


SUBSPACE_GRAM_MAX_BYTES = 1 << 30         # default output budget of one K53 launch: memory, not a tuned number
SUBSPACE_GRAM_MAX_LEARNERS = 65535        # learners one K53 launch takes (its grid's second dimension)
SUBSPACE_GRAM_TILE, SUBSPACE_GRAM_KC, SUBSPACE_GRAM_MFMA = 64, 32, 16     # K53's geometry (csrc/ensemble.hip: SG_TILE, SG_KC, the MFMA tile), for tests


def subspace_gram(zt: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor, out: Optional[torch.Tensor] = None,
                  max_bytes: int = SUBSPACE_GRAM_MAX_BYTES) -> torch.Tensor:
    """zt: (d, n_rows) float64, contiguous, feature-major; idx: (L, d_sub) int32, every entry in [0, d); weights: (L, n_rows) int32 >= 0
    -> G (L, d_sub, d_sub) float64, G[l, a, b] = sum_i weights[l, i] zt[idx[l, a], i] zt[idx[l, b], i]: the bootstrap-weighted scatter of
    every base learner of ws_unet_amd.ensemble in float64 on the matrix pipe (wsu_subspace_gram_f64, K53, which include/wsu.h defines).
    G[l] is symmetric bit for bit.  L is split into launches whose output stays under `max_bytes` (one learner at least); a learner's
    bits do not depend on the split.  `out`: a float64 tensor of that shape to write into.  ValueError, before anything is launched, for
    a wrong dtype, shape, device, a tensor that is not contiguous, a negative weight or an index outside [0, d) (one reduction each on
    the device).  The input must be finite; the callers check that once."""
    for name, t, dtype, dim in (("zt", zt, torch.float64, 2), ("idx", idx, torch.int32, 2), ("weights", weights, torch.int32, 2)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dim:
            raise ValueError(f"subspace_gram: {name} must be a {dim}-d {dtype} tensor, got "
                             f"{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if not t.is_cuda or t.device != zt.device:
            raise ValueError(f"subspace_gram: {name} must be on the GPU, on zt's device: got {t.device} (no CPU fallback exists)")
        if not t.is_contiguous():
            raise ValueError(f"subspace_gram: {name} must be contiguous" + (" (feature-major: pass Z.T.contiguous())" if name == "zt" else ""))
    (d, n_rows), (L, d_sub) = zt.shape, idx.shape
    if min(d, n_rows, L, d_sub) < 1 or tuple(weights.shape) != (L, n_rows):
        raise ValueError(f"subspace_gram: zt {tuple(zt.shape)}, idx {tuple(idx.shape)}, weights {tuple(weights.shape)}: expected (d, n_rows), "
                         f"(L, d_sub), (L, n_rows), all sizes positive")
    if d_sub > 1 << 20:
        raise ValueError(f"subspace_gram: d_sub={d_sub} above 2^20")
    if isinstance(max_bytes, bool) or int(max_bytes) != max_bytes or max_bytes < 1:
        raise ValueError(f"subspace_gram: max_bytes={max_bytes!r} must be a positive integer")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (L, d_sub, d_sub)
                            or out.device != zt.device or not out.is_contiguous()):
        raise ValueError(f"subspace_gram: out must be a contiguous float64 tensor of shape {(L, d_sub, d_sub)} on {zt.device}")
    lo, hi, wmin = (int(v) for v in torch.stack([idx.min(), idx.max(), weights.min()]).tolist())
    if lo < 0 or hi >= d:
        raise ValueError(f"subspace_gram: idx holds {lo if lo < 0 else hi}, outside [0, {d}); nothing was launched")
    if wmin < 0:
        raise ValueError(f"subspace_gram: weights hold {wmin}: multiplicities must not be negative")
    G = torch.empty((L, d_sub, d_sub), dtype=torch.float64, device=zt.device) if out is None else out
    per = max(1, min(SUBSPACE_GRAM_MAX_LEARNERS, int(max_bytes) // (8 * d_sub * d_sub)))
    fn = _lib.load().wsu_subspace_gram_f64
    for l0 in range(0, L, per):
        m = min(per, L - l0)
        check(_launch("subspace_gram", {"flops": float(m) * n_rows * d_sub * (d_sub + 1)}, lambda: fn(
            zt.data_ptr(), idx[l0:l0 + m].data_ptr(), weights[l0:l0 + m].data_ptr(), G[l0:l0 + m].data_ptr(), n_rows, d, d_sub, m,
            _stream())), "wsu_subspace_gram_f64")
    return G


# The tables of K50 as data.  SRM_MINMAX_Q2: the q2 of its three classes.  SRM_MINMAX_SETS: per class its sets in order, name -> how far the
# union of the members' taps reaches (up, down, left, right).  SRM_MINMAX_TABLES: the 118 tables in the order of the counts, (class, q2,
# set, scan, a, b) with the table's total 2 max(H - a, 0) max(W - b, 0): for class; for q ascending; for set; for scan in (h, v).
SRM_MINMAX_Q2 = {cls: SRM_Q2[cls] for cls in ("S1", "S2", "S3")}
SRM_MINMAX_SETS = {
    "S1": {"WE": (0, 0, 1, 1), "NS": (1, 1, 0, 0), "WENS": (1, 1, 1, 1), "WNE": (1, 0, 1, 1), "ESW": (0, 1, 1, 1), "SWN": (1, 1, 1, 0), "NES": (1, 1, 0, 1)},
    "S2": {name: (1, 1, 1, 1) for name in ("hv", "hvdm", "hvd", "hvm", "hd", "hm", "vd", "vm")},
    "S3": {"WE": (0, 0, 2, 2), "NS": (2, 2, 0, 0), "WENS": (2, 2, 2, 2), "WNE": (2, 1, 2, 2), "ESW": (1, 2, 2, 2), "SWN": (2, 2, 2, 1), "NES": (2, 2, 1, 2)}}
SRM_MINMAX_TABLES = _set_tables(SRM_MINMAX_Q2, SRM_MINMAX_SETS)


def srm_minmax_counts(x_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,118,625) int64: per image the co-occurrence counts of the min/max submodels of the spatial rich model on
    the directional residuals of the first three orders, table by table as SRM_MINMAX_TABLES lists them: per run of four positions
    along a row or down a column the minimum digits of a set of residuals at their bin and its maximum digits, negated, at theirs, over
    every run whose taps all lie in the image (wsu_srm_minmax_counts, K50, which include/wsu.h defines; ws_unet_amd.srm.features_minmax
    makes the features).  `out`: an int64 tensor of that shape to write into (the call zeroes it)."""
    return _set_counts("srm_minmax_counts", SRM_MINMAX_TABLES, x_u8, out)


def _fan_sets(along, against):
    """name -> (up, down, left, right) of the 20 sets of K54, whose member residuals reach `along` pixels along their direction and
    `against` against it"""
    step = {"E": (0, 1), "NE": (-1, 1), "N": (-1, 0), "NW": (-1, -1), "W": (0, -1), "SW": (1, -1), "S": (1, 0), "SE": (1, 1)}

    def side(members, axis, sign):
        return max(along if step[m][axis] * sign > 0 else against if step[m][axis] * sign < 0 else 0 for m in members)
    return {name: (side(m, 0, -1), side(m, 0, 1), side(m, 1, -1), side(m, 1, 1)) for name in SRM_FAN_SET_NAMES for m in [name.split("+")]}


# The tables of K54 as data, as K50's above.  SRM_FAN_SET_NAMES: the 20 sets in order, named by their members: the perpendicular pairs, the
# 3-fans, the "vertical" and the "horizontal" 4-fans, the 5-fans.  SRM_FAN_TABLES: the 200 tables.
SRM_FAN_Q2 = {cls: SRM_Q2[cls] for cls in ("S1", "S3")}
SRM_FAN_SET_NAMES = ("E+N", "N+W", "W+S", "S+E", "E+NE+N", "N+NW+W", "W+SW+S", "S+SE+E",
                     "E+NE+N+NW", "NE+N+NW+W", "W+SW+S+SE", "SW+S+SE+E", "N+NW+W+SW", "NW+W+SW+S", "S+SE+E+NE", "SE+E+NE+N",
                     "SE+E+NE+N+NW", "NE+N+NW+W+SW", "NW+W+SW+S+SE", "SW+S+SE+E+NE")
SRM_FAN_SETS = {"S1": _fan_sets(1, 0), "S3": _fan_sets(2, 1)}
SRM_FAN_TABLES = _set_tables(SRM_FAN_Q2, SRM_FAN_SETS)
# The tables of K55: the classes E3 and E5 at the steps of S3x3 and S5x5, their eleven sets with the reach k = 1 or 2, the 132 tables.
SRM_EDGE_Q2 = {"E3": SRM_Q2["S3x3"], "E5": SRM_Q2["S5x5"]}
SRM_EDGE_SETS = {cls: {"U": (k, 0, k, k), "D": (0, k, k, k), "L": (k, k, k, 0), "R": (k, k, 0, k),
                       **{name: (k, k, k, k) for name in ("UL", "UR", "DL", "DR", "UD", "LR", "UDLR")}} for cls, k in (("E3", 1), ("E5", 2))}
SRM_EDGE_TABLES = _set_tables(SRM_EDGE_Q2, SRM_EDGE_SETS)


def srm_fan_counts(x_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,200,625) int64: per image the co-occurrence counts of the first- and third-order min/max submodels of
    the spatial rich model over perpendicular pairs and 3-, 4- and 5-fans of the eight directional residuals, table by table as
    SRM_FAN_TABLES lists them; the two updates per run and the condition for a run to count are srm_minmax_counts's
    (wsu_srm_fan_counts, K54, which include/wsu.h defines; ws_unet_amd.srm.features_fans makes the features).  `out`: an int64 tensor of
    that shape to write into (the call zeroes it)."""
    return _set_counts("srm_fan_counts", SRM_FAN_TABLES, x_u8, out)


def srm_edge_counts(x_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,132,625) int64: per image the co-occurrence counts of the EDGE3x3 and EDGE5x5 classes of the spatial rich
    model, table by table as SRM_EDGE_TABLES lists them: the four half-kernel residuals U, D, L, R and the min/max tables of eleven sets
    of them, a singleton's table being its plain table plus the negated one (wsu_srm_edge_counts, K55, which include/wsu.h defines;
    ws_unet_amd.srm.features_edge makes the features).  `out`: an int64 tensor of that shape to write into (the call zeroes it)."""
    return _set_counts("srm_edge_counts", SRM_EDGE_TABLES, x_u8, out)


# IJG luminance base table (the JPEG standard's Annex K.1), row-major by frequency [u][v]
_IJG_LUMINANCE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
    [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92], [49, 64, 78, 87, 103, 121, 120, 101],
    [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.int64)


def jpeg_tables(qualities) -> np.ndarray:
    """IJG qualities (each in 1..100) -> HOST int32 (M,8,8) luminance quantisation tables: Q = clip((T s + 50) // 100, 1, 255) with
    s = 5000 // q for q < 50, 200 - 2 q otherwise."""
    q = np.atleast_1d(np.asarray(qualities))
    if q.ndim != 1 or q.dtype.kind not in "iu" or (q.size and (q.min() < 1 or q.max() > 100)):
        raise ValueError(f"jpeg_tables: integer qualities in 1..100 expected, got {qualities!r}")
    q = q.astype(np.int64)
    s = np.where(q < 50, 5000 // q, 200 - 2 * q)
    return np.clip((_IJG_LUMINANCE[None] * s[:, None, None] + 50) // 100, 1, 255).astype(np.int32)


def _jpeg_args(who: str, x_u8: torch.Tensor, tables, rows: Optional[int]) -> Tuple[int, int, int, np.ndarray]:
    n, h, w = _u8_planes(x_u8)
    if n == 0:
        raise ValueError(f"{who}: no images")
    if h % 8 or w % 8 or h * w > 1 << 24:
        raise ValueError(f"{who}: planes of h={h} w={w}: h and w must be multiples of 8 and h * w at most 2^24")
    t = np.asarray(tables)
    if t.dtype.kind not in "iu" or t.ndim != 3 or t.shape[1:] != (8, 8) or t.shape[0] == 0 or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{who}: integer tables of shape ({'M' if rows is None else rows},8,8) expected, got {t.dtype} {t.shape}")
    if t.min() < 1 or t.max() > 255:
        raise ValueError(f"{who}: table entries must lie in 1..255")
    return n, h, w, np.ascontiguousarray(t, dtype=np.int32)


def jpeg_energies(x_u8: torch.Tensor, tables) -> torch.Tensor:
    """x_u8: (N,H,W) uint8, H and W multiples of 8; tables: HOST integer (M,8,8), entries 1..255 -> int64 (N,M): the residual energy of
    every image's 8x8 DCT coefficients against every table, in 2^-20 units (wsu_jpeg_energies, K31; ws_unet_amd.ws.jpeg reads the
    compression history from it).  Exact integers."""
    t = _jpeg_args("jpeg_energies", x_u8, tables, None)[3]
    return _count_entry("jpeg_energies", x_u8, (t.shape[0],), t.ctypes.data, t.shape[0])


def jpeg_predict(x_u8: torch.Tensor, tables, use=None, want_u8: bool = False, want_hat: bool = True):
    """The images after quantisation with their own table and the way back (wsu_jpeg_predict, K32).  x_u8: (N,H,W) uint8; tables: HOST
    integer (N,8,8), one per image; use: HOST (N,) booleans or None (all): an image with use = 0 gets the KB filter's prediction in the place
    of the round trip (its table is ignored).  Returns x_hat float32 (N,H,W) in pixel units (hat_scale = 1 for the WS statistics);
    with want_u8 (x_hat, the recompressed uint8 planes -- the input where use = 0); without want_hat x_hat is None and not computed."""
    lib = _lib.load()
    n, h, w = _u8_planes(x_u8)
    u = np.ones(n, dtype=np.uint8) if use is None else np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8)
    if u.shape != (n,):
        raise ValueError(f"jpeg_predict: use of shape {u.shape} for {n} images")
    t = np.asarray(tables)
    if t.ndim == 3 and t.shape[0] == n and t.dtype.kind in "iu":
        t = np.where(u[:, None, None] != 0, t, 1)                      # (an unused table is not read)
    n, h, w, t = _jpeg_args("jpeg_predict", x_u8, t, n)
    x_hat = torch.empty((n, h, w), dtype=torch.float32, device=x_u8.device) if want_hat else None
    out = torch.empty_like(x_u8) if want_u8 else None
    check(_launch("jpeg_predict", {"bytes": float(n * h * w * (1 + 4 * want_hat + want_u8))}, lambda: lib.wsu_jpeg_predict(
        x_u8.data_ptr(), t.ctypes.data, u.ctypes.data, _ptr(x_hat), _ptr(out), n, h, w, _stream())), "wsu_jpeg_predict")
    return (x_hat, out) if want_u8 else x_hat


def jpeg_recompress(x_u8: torch.Tensor, quality: int) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> the planes after a round trip through the IJG luminance table of `quality` (K32's uint8 output): a
    JPEG-precompressed twin made without any JPEG library."""
    n = _u8_planes(x_u8)[0]
    return jpeg_predict(x_u8, np.repeat(jpeg_tables([int(quality)]), max(n, 1), axis=0), want_u8=True, want_hat=False)[1]


def hill_cost(x_u8: torch.Tensor, clamp: float = 1e10) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,H,W) fp32 HILL cost with cost[inf | nan | > clamp] = clamp (wsu_hill_cost, K12)."""
    lib = _lib.load()
    _dev_check(x_u8)
    assert x_u8.dtype == torch.uint8 and x_u8.dim() == 3
    n, h, w = x_u8.shape
    cost = torch.empty((n, h, w), dtype=torch.float32, device=x_u8.device)
    check(_launch("hill_cost", {"bytes": float(n * h * w * 5)}, lambda: lib.wsu_hill_cost(
        x_u8.data_ptr(), cost.data_ptr(), float(clamp), n, h, w, _stream())), "wsu_hill_cost")
    return cost


def hill_threshold(cost: torch.Tensor, quantile: float = 0.1) -> torch.Tensor:
    """cost: (N,H,W) fp32 -> q[N] fp64 = numpy.quantile(cost[i, 1:-1, 1:-1], quantile) ('linear'), by an exact radix select (K13)."""
    from .hill import quantile_index
    lib = _lib.load()
    _dev_check(cost)
    assert cost.dtype == torch.float32 and cost.dim() == 3
    n, h, w = cost.shape
    k, g = quantile_index((h - 2) * (w - 2), quantile)
    q = torch.empty(n, dtype=torch.float64, device=cost.device)
    ws = torch.empty(lib.wsu_hill_threshold_workspace_bytes(n) // 4, dtype=torch.int32, device=cost.device)
    check(_launch("hill_threshold", {"bytes": float(n * h * w * 16)}, lambda: lib.wsu_hill_threshold(
        cost.data_ptr(), k, g, q.data_ptr(), ws.data_ptr(), ws.numel() * 4, n, h, w, _stream())), "wsu_hill_threshold")
    return q


def _u8_planes(x_u8: torch.Tensor) -> Tuple[int, int, int]:
    _dev_check(x_u8)
    if x_u8.dtype != torch.uint8 or x_u8.dim() != 3:
        raise ValueError(f"expected an (N,H,W) uint8 tensor, got {tuple(x_u8.shape)} {x_u8.dtype}")
    return tuple(x_u8.shape)


def hill_cost_f64(x_u8: torch.Tensor, clamp: float = 1e10) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,H,W) fp64 HILL cost, bit-identical to numpy's float64 restatement (wsu_hill_cost_f64, K20): the
    ranking key of the HILLR simulator."""
    lib = _lib.load()
    n, h, w = _u8_planes(x_u8)
    key = torch.empty((n, h, w), dtype=torch.float64, device=x_u8.device)
    check(_launch("hill_cost_f64", {"bytes": float(n * h * w * 9)}, lambda: lib.wsu_hill_cost_f64(
        x_u8.data_ptr(), key.data_ptr(), float(clamp), n, h, w, _stream())), "wsu_hill_cost_f64")
    return key


WAVELET_COST_KINDS = {"suniward": 0, "wow": 1}                      # WSU_COST_* of include/wsu.h
WAVELET_COST_CLAMPS = {"suniward": 1e8, "wow": 1e10}


def wavelet_cost_f64(x_u8: torch.Tensor, kind: str, sigma: float = 1.0, clamp: Optional[float] = None) -> torch.Tensor:
    """x_u8: (N,H,W) uint8 -> (N,H,W) fp64 S-UNIWARD (`kind` 'suniward') or WOW ('wow') cost, bit-identical to numpy's float64
    restatement (wsu_wavelet_cost_f64, K48).  sigma: S-UNIWARD's stabilising constant; clamp: None takes the kind's default (1e8, 1e10)."""
    lib = _lib.load()
    n, h, w = _u8_planes(x_u8)
    if kind not in WAVELET_COST_KINDS:
        raise ValueError(f"kind must be one of {' / '.join(WAVELET_COST_KINDS)}, got {kind!r}")
    rho = torch.empty((n, h, w), dtype=torch.float64, device=x_u8.device)
    check(_launch("wavelet_cost_f64", {"bytes": float(n * h * w * 9)}, lambda: lib.wsu_wavelet_cost_f64(
        x_u8.data_ptr(), rho.data_ptr(), WAVELET_COST_KINDS[kind], float(sigma), float(WAVELET_COST_CLAMPS[kind] if clamp is None else clamp),
        n, h, w, _stream())), "wsu_wavelet_cost_f64")
    return rho


def rank_select_f64(key: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """key: (N,H,W) fp64, positive and finite; k: (N) int64 ranks on the device -> (N) int64 holding the uint64 pattern of each
    image's key of rank k (0-based, ascending; negative: the pattern 0, below every key), by an exact radix select (K21)."""
    lib = _lib.load()
    _dev_check(key, k)
    assert key.dtype == torch.float64 and key.dim() == 3 and k.dtype == torch.int64 and k.shape == (key.shape[0],)
    n, h, w = key.shape
    bits = torch.empty(n, dtype=torch.int64, device=key.device)
    ws = torch.empty(lib.wsu_rank_select_f64_workspace_bytes(n) // 8, dtype=torch.int64, device=key.device)
    check(_launch("rank_select_f64", {"bytes": float(n * h * w * 48)}, lambda: lib.wsu_rank_select_f64(
        key.data_ptr(), k.data_ptr(), bits.data_ptr(), ws.data_ptr(), ws.numel() * 8, n, h, w, _stream())), "wsu_rank_select_f64")
    return bits


def _f64_planes(who: str, x_u8: torch.Tensor, rho: torch.Tensor, name: str = "rho") -> Tuple[int, int, int]:
    """(N,H,W) uint8 planes with a float64 plane (a cost, a key) for every one of them."""
    n, h, w = _u8_planes(x_u8)
    _dev_check(rho)
    if rho.dtype != torch.float64 or rho.shape != x_u8.shape:
        raise ValueError(f"{who}: {name} must be float64 of shape {tuple(x_u8.shape)}, got {tuple(rho.shape)} {rho.dtype}")
    return n, h, w


def _vector(who: str, name: str, t: torch.Tensor, n: int, dtype) -> int:
    """An (N) device vector of `dtype`, one entry per image -> its pointer."""
    if not (t.is_cuda and t.is_contiguous()):
        _dev_check(t)                                               # (raises; asked inline first because these wrappers are host-bound)
    if t.dtype != dtype or t.shape != (n,):
        raise ValueError(f"{who}: {name} must be {str(dtype).replace('torch.', '')} of shape ({n},), got {tuple(t.shape)} {t.dtype}")
    return t.data_ptr()


def _embed_entry(entry: str, cover_u8: torch.Tensor, bytes_per_pixel: int, *middle) -> Tuple[torch.Tensor, torch.Tensor]:
    """wsu_<entry>(cover, *middle, stego, changes, n, h, w, stream), the form of every simulator entry -> (stego (N,H,W) uint8, changes
    (N) int64).  The caller has checked the cover (_u8_planes / _f64_planes) and `middle`; bytes_per_pixel: the timer's traffic figure."""
    n, h, w = cover_u8.shape
    symbol = "wsu_" + entry
    fn = getattr(_lib.load(), symbol)
    stego = torch.empty_like(cover_u8)
    changes = torch.empty(n, dtype=torch.int64, device=cover_u8.device)
    check(_launch(entry, {"bytes": float(n * h * w * bytes_per_pixel)}, lambda: fn(
        cover_u8.data_ptr(), *middle, stego.data_ptr(), changes.data_ptr(), n, h, w, _stream())), symbol)
    return stego, changes


def embed_threshold(cover_u8: torch.Tensor, key: torch.Tensor, bits: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """stego = cover ^ (key <= the key whose pattern is bits[i]), every tie flipped (K22) -> (stego (N,H,W) uint8, changes (N) int64)."""
    who = "embed_threshold"
    n = _f64_planes(who, cover_u8, key, "key")[0]
    return _embed_entry(who, cover_u8, 10, key.data_ptr(), _vector(who, "bits", bits, n, torch.int64))


def lsbr_threshold(alpha: float) -> int:
    """T = floor(alpha / 2 * 2^32) of wsu_embed_lsbr (a pixel flips iff its generator word < T); alpha outside [0, 1] raises."""
    import ctypes
    t = ctypes.c_uint32(0)
    check(_lib.load().wsu_lsbr_threshold(float(alpha), ctypes.byref(t)), "wsu_lsbr_threshold")
    return t.value


def embed_lsbr(cover_u8: torch.Tensor, seeds: torch.Tensor, thresholds: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """LSB replacement with Philox4x32-10 (K23).  seeds: (N) int64 holding the images' 64-bit seeds; thresholds: (N) int32 holding
    the uint32 lsbr_threshold of each image's alpha -> (stego (N,H,W) uint8, changes (N) int64)."""
    who = "embed_lsbr"
    n = _u8_planes(cover_u8)[0]
    return _embed_entry(who, cover_u8, 2, _vector(who, "seeds", seeds, n, torch.int64), _vector(who, "thresholds", thresholds, n, torch.int32))


def embed_lsbr_seq(cover_u8: torch.Tensor, seeds: torch.Tensor, counts: torch.Tensor, order="rows") -> Tuple[torch.Tensor, torch.Tensor]:
    """Sequential LSB replacement (K28): the first counts[i] pixels of the path over the whole plane ('rows': row by row from the top,
    'rows_up': from the bottom row upwards) flip as under embed_lsbr at alpha = 1.  seeds: (N) int64 holding the 64-bit seeds; counts:
    (N) int64 -> (stego (N,H,W) uint8, changes (N) int64)."""
    who, oid = "embed_lsbr_seq", order_id(order)
    n = _u8_planes(cover_u8)[0]
    return _embed_entry(who, cover_u8, 2, _vector(who, "seeds", seeds, n, torch.int64), _vector(who, "counts", counts, n, torch.int64), oid)


def embed_threshold_lsbr(cover_u8: torch.Tensor, key: torch.Tensor, bits: torch.Tensor, seeds: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """HILLR's selection with a real message (K34): a pixel with key <= the key whose pattern is bits[i] is used, and a used pixel flips as
    under embed_lsbr at alpha = 1 with the image's seed.  key: (N,H,W) float64; bits, seeds: (N) int64 -> (stego (N,H,W) uint8, changes
    (N) int64)."""
    who = "embed_threshold_lsbr"
    n = _f64_planes(who, cover_u8, key, "key")[0]
    return _embed_entry(who, cover_u8, 10, key.data_ptr(), _vector(who, "bits", bits, n, torch.int64), _vector(who, "seeds", seeds, n, torch.int64))


def lsbr_key_threshold(alpha: float) -> int:
    """T = floor(alpha * 2^32) in 0..2^32 of wsu_embed_lsbr_keyed (a pixel is used iff its key word < T, compared in 64 bits, so alpha = 1
    uses every pixel); alpha outside [0, 1] raises."""
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise ValueError(f"lsbr_key_threshold: alpha={alpha!r} outside [0, 1]")
    return int(np.floor(np.float64(a) * 4294967296.0))


def _key_args(who: str, key_seed, alpha_threshold) -> Tuple[int, int]:
    key, thr = int(key_seed), int(alpha_threshold)
    if not 0 <= key < 2 ** 64:
        raise ValueError(f"{who}: key_seed {key_seed!r} outside [0, 2^64)")
    if not 0 <= thr <= 2 ** 32:
        raise ValueError(f"{who}: alpha_threshold {alpha_threshold!r} outside 0..2^32 (lsbr_key_threshold)")
    return key, thr


def embed_lsbr_keyed(cover_u8: torch.Tensor, seeds: torch.Tensor, key_seed: int, alpha_threshold: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """LSB replacement at the positions one stego key selects in every image (K30): pixel i is used iff its Philox word under `key_seed`
    is below `alpha_threshold` (lsbr_key_threshold) and a used pixel flips as under embed_lsbr at alpha = 1 with the image's seed.  seeds:
    (N) int64 holding the 64-bit seeds -> (stego (N,H,W) uint8, changes (N) int64)."""
    who = "embed_lsbr_keyed"
    key, thr = _key_args(who, key_seed, alpha_threshold)
    n = _u8_planes(cover_u8)[0]
    return _embed_entry(who, cover_u8, 2, _vector(who, "seeds", seeds, n, torch.int64), key, thr)


def lsbr_key_mask(key_seed: int, alpha_threshold: int, h: int, w: int, device=None) -> torch.Tensor:
    """The positions embed_lsbr_keyed uses under (key_seed, alpha_threshold) in an (H,W) plane: (H,W) uint8 of 1 / 0 on `device` (the
    current GPU by default)."""
    key, thr = _key_args("lsbr_key_mask", key_seed, alpha_threshold)
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"lsbr_key_mask: bad shape {h} x {w}")
    lib = _lib.load()
    mask = torch.empty((h, w), dtype=torch.uint8, device=torch.device("cuda") if device is None else device)
    _dev_check(mask)
    check(_launch("lsbr_key_mask", {"bytes": float(h * w)}, lambda: lib.wsu_lsbr_key_mask(key, thr, mask.data_ptr(), h, w, _stream())),
          "wsu_lsbr_key_mask")
    return mask


# ---- the +-1 simulators (K37-K39) ---------------------------------------------------------------------------------------------------

TERNARY_MAX_LAMBDAS = 16                                            # multipliers per wsu_ternary_entropy launch
# ternary_lambda: 2^-50, 2^-45, .., 2^25, then 8 times the 16 inner points that cut the bracket into 17 geometric steps: 9 launches and
# lam_hi / lam_lo = 2^(5 / 17^8) = 1 + 5.0e-10.  HILL's costs lie between 9 / (9 * 16 * 255) = 2.5e-4 and the clamp 1e10: at 2^-50 every a
# is below 1e-5 (h is log2 3, or 1 at a wet end, to 11 digits) and at 2^25 every a exceeds 8000 (exp underflows: h = 0).
TERNARY_LADDER = tuple(2.0 ** e for e in range(-50, 26, 5))
TERNARY_REFINEMENTS = 8


def ternary_entropy(x_u8: torch.Tensor, rho: torch.Tensor, lambdas: torch.Tensor) -> torch.Tensor:
    """The bits a +-1 sender with change probabilities exp(-lambda rho) / Z embeds (K37).  x_u8: (N,H,W) uint8; rho: (N,H,W) float64,
    positive, +inf = wet; lambdas: (N,L) float64, positive, 1 <= L <= 16 -> (N,L) float64.  The +1 change is wet at 255, the -1 change at
    0.  Same bits on every call and in every batch."""
    lib = _lib.load()
    n, h, w = _f64_planes("ternary_entropy", x_u8, rho)
    _dev_check(lambdas)
    if lambdas.dtype != torch.float64 or lambdas.dim() != 2 or lambdas.shape[0] != n or not 1 <= lambdas.shape[1] <= TERNARY_MAX_LAMBDAS:
        raise ValueError(f"ternary_entropy: lambdas must be float64 of shape ({n}, 1..{TERNARY_MAX_LAMBDAS}), got {tuple(lambdas.shape)} {lambdas.dtype}")
    nl = lambdas.shape[1]
    out = torch.empty((n, nl), dtype=torch.float64, device=x_u8.device)
    ws = torch.empty(lib.wsu_ternary_entropy_workspace_bytes(n) // 8, dtype=torch.float64, device=x_u8.device)
    check(_launch("ternary_entropy", {"bytes": float(n * h * w * 9)}, lambda: lib.wsu_ternary_entropy(
        x_u8.data_ptr(), rho.data_ptr(), lambdas.data_ptr(), nl, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, n, h, w, _stream())),
        "wsu_ternary_entropy")
    return out


def _last_true(flags: torch.Tensor) -> torch.Tensor:
    """(N,K) bool -> (N,1) int64: the largest index that holds True (0 where none does)."""
    idx = torch.arange(flags.shape[1], device=flags.device)
    return (flags.to(torch.int64) * idx).amax(dim=1, keepdim=True)


def ternary_lambda(x_u8: torch.Tensor, rho: torch.Tensor, message_bits: torch.Tensor):
    """The multiplier at which ternary_entropy equals the payload, per image: (lam_lo, lam_hi, ok), all (N) on the device, with
    H(lam_lo) >= message_bits >= H(lam_hi) and lam_hi / lam_lo - 1 <= 2^-29; embed with lam_lo, whose capacity is not short.  message_bits:
    (N) float64 on the device, not negative.  ok[i] is False where even the lowest multiplier of TERNARY_LADDER carries less than the
    payload (lam_lo = lam_hi = that multiplier then).  Where the highest still carries it (a payload of 0) lam_lo = lam_hi = the highest.
    Nine K37 launches; the bracket is chosen between them on the device, nothing waits for the GPU."""
    n, h, w = _f64_planes("ternary_lambda", x_u8, rho)
    _vector("ternary_lambda", "message_bits", message_bits, n, torch.float64)
    dev = x_u8.device
    m = message_bits[:, None]
    ladder = torch.tensor(TERNARY_LADDER, dtype=torch.float64, device=dev).expand(n, -1).contiguous()
    ge = ternary_entropy(x_u8, rho, ladder) >= m
    ok = ge[:, 0].clone()
    k = _last_true(ge)
    lo = ladder.gather(1, k)
    hi = ladder.gather(1, (k + 1).clamp_max(ladder.shape[1] - 1))
    hi = torch.where(ok[:, None], hi, lo)
    steps = torch.arange(1, TERNARY_MAX_LAMBDAS + 1, dtype=torch.float64, device=dev) / (TERNARY_MAX_LAMBDAS + 1)
    true, false = torch.ones((n, 1), dtype=torch.bool, device=dev), torch.zeros((n, 1), dtype=torch.bool, device=dev)
    for _ in range(TERNARY_REFINEMENTS):
        inner = torch.minimum(torch.maximum(lo * torch.exp2(torch.log2(hi / lo) * steps), lo), hi)
        ge = ternary_entropy(x_u8, rho, inner.contiguous()) >= m
        points = torch.cat([lo, inner, hi], dim=1)
        k = _last_true(torch.cat([true, ge, false], dim=1))
        lo, hi = points.gather(1, k), points.gather(1, k + 1)
    return lo[:, 0], hi[:, 0], ok


def embed_ternary(cover_u8: torch.Tensor, rho: torch.Tensor, lambdas: torch.Tensor, seeds: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The +-1 sender's draw (K38): pixel i becomes x + 1 with probability exp(-lambda rho) / Z, x - 1 with the same (never out of 0..255:
    that direction is wet), from the generator word embed_lsbr gives it.  rho: (N,H,W) float64; lambdas: (N) float64, positive (+inf: the
    cover); seeds: (N) int64 holding the 64-bit seeds -> (stego (N,H,W) uint8, changes (N) int64)."""
    who = "embed_ternary"
    n = _f64_planes(who, cover_u8, rho)[0]
    return _embed_entry(who, cover_u8, 10, rho.data_ptr(), _vector(who, "lambdas", lambdas, n, torch.float64),
                        _vector(who, "seeds", seeds, n, torch.int64))


def change_weights(x_u8: torch.Tensor, rho: torch.Tensor, lambdas: torch.Tensor) -> torch.Tensor:
    """The change probability of embed_ternary's sender per pixel as a 16-bit weight (K51): floor((p+ + p-) * 65536), at most 43 690;
    0 where rho or lambda is +inf.  rho: (N,H,W) float64; lambdas: (N) float64, given by the caller (ternary_lambda finds a payload's)
    -> (N,H,W) uint16, the weights of srm_weighted_counts."""
    who = "change_weights"
    n, h, w = _f64_planes(who, x_u8, rho)
    if n == 0:
        raise ValueError(f"{who}: no images")
    lam = _vector(who, "lambdas", lambdas, n, torch.float64)
    weights = torch.empty((n, h, w), dtype=torch.uint16, device=x_u8.device)
    check(_launch(who, {"bytes": float(n * h * w * 11)}, lambda: _lib.load().wsu_change_weights(
        x_u8.data_ptr(), rho.data_ptr(), lam, weights.data_ptr(), n, h, w, _stream())), "wsu_change_weights")
    return weights


def lsbm_threshold(alpha: float) -> int:
    """T = floor(alpha / 4 * 2^32) of wsu_embed_lsbm (a pixel goes up iff its generator word < T, down iff it is in [T, 2T)); alpha
    outside [0, 1] raises."""
    import ctypes
    t = ctypes.c_uint32(0)
    check(_lib.load().wsu_lsbm_threshold(float(alpha), ctypes.byref(t)), "wsu_lsbm_threshold")
    return t.value


def embed_lsbm(cover_u8: torch.Tensor, seeds: torch.Tensor, thresholds: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """LSB matching with Philox4x32-10 (K39): a fraction alpha / 2 of the pixels changes by +-1, the sign random, inwards at 0 and 255.
    seeds: (N) int64 holding the images' 64-bit seeds; thresholds: (N) int32 holding the uint32 lsbm_threshold of each image's alpha ->
    (stego (N,H,W) uint8, changes (N) int64)."""
    who = "embed_lsbm"
    n = _u8_planes(cover_u8)[0]
    return _embed_entry(who, cover_u8, 2, _vector(who, "seeds", seeds, n, torch.int64), _vector(who, "thresholds", thresholds, n, torch.int32))


# ---- syndrome-trellis codes (K40-K42) ----------------------------------------------------------------------------------------------

STC_MAX_H = 10                                                      # constraint heights 1..10: up to 1024 states, one thread each
STC_CHANGES = ("flip", "pm1")
# stc_embed's take bits need pixels * max(2^h, 64) / 8 bytes per image (32 MiB at 512 x 512, h = 10); a batch is embedded in slices whose
# workspace stays under this many bytes (at least one image per slice).  8 GiB: 256 such images, one workgroup for each compute unit
STC_WORKSPACE_CAP = 8 << 30


def philox_words(seeds: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """The generator word embed_lsbr gives every pixel (K40): seeds: (N) int64 holding the images' 64-bit seeds -> (N,H,W) int32 holding
    the uint32 words."""
    lib = _lib.load()
    _dev_check(seeds)
    h, w = int(h), int(w)
    if seeds.dtype != torch.int64 or seeds.dim() != 1 or h < 1 or w < 1:
        raise ValueError(f"philox_words: (N) int64 seeds and a shape expected, got {tuple(seeds.shape)} {seeds.dtype}, {h} x {w}")
    n = seeds.shape[0]
    words = torch.empty((n, h, w), dtype=torch.int32, device=seeds.device)
    check(_launch("philox_words", {"bytes": float(n * h * w * 4)}, lambda: lib.wsu_philox_words(
        seeds.data_ptr(), words.data_ptr(), n, h, w, _stream())), "wsu_philox_words")
    return words


def _stc_height(who: str, h) -> int:
    h = int(h)
    if not 1 <= h <= STC_MAX_H:
        raise ValueError(f"{who}: constraint height h={h} outside 1..{STC_MAX_H}")
    return h


def _stc_table(who: str, n: int, hw: int, cols: torch.Tensor, path: Optional[torch.Tensor], least: int, least_what: str) -> None:
    """The column table (at least `least` entries, which the message calls `least_what`) and the paths of a uniform or a ragged code."""
    _dev_check(cols, path)
    if cols.dtype != torch.int32 or cols.dim() != 1 or cols.shape[0] < least:
        raise ValueError(f"{who}: cols must be int32 with at least {least_what}, got {tuple(cols.shape)} {cols.dtype}")
    if path is not None and (path.dtype != torch.int32 or path.shape != (n, hw)):
        raise ValueError(f"{who}: path must be int32 of shape ({n}, {hw}), got {tuple(path.shape)} {path.dtype}")


def _stc_code(who: str, n: int, hw: int, h, k, cols: torch.Tensor, path: Optional[torch.Tensor]) -> Tuple[int, int]:
    h, k = _stc_height(who, h), int(k)
    if not 1 <= k <= hw:
        raise ValueError(f"{who}: k={k} message bits outside 1..{hw} (the pixels of an image)")
    wmax = -(-hw // k)
    _stc_table(who, n, hw, cols, path, wmax, f"ceil(n / k) = {wmax} entries")
    return h, k


def stc_workspace_bytes(pixels: int, h: int) -> int:
    """Bytes of take bits stc_embed needs per image of `pixels` pixels at constraint height h (wsu_stc_workspace_bytes)."""
    b = _lib.load().wsu_stc_workspace_bytes(int(pixels), int(h))
    if b == 0:
        raise ValueError(f"stc_workspace_bytes: pixels={pixels}, h={h}: a positive pixel count and h in 1..{STC_MAX_H} expected")
    return b


def _stc_slices(who: str, n: int, hw: int, h: int, workspace_cap, workspace: Optional[torch.Tensor], dev):
    """(bytes of take bits per image, images per slice, the slices' workspace): the caller's `workspace` holds the whole batch, else one
    of at most `workspace_cap` bytes (at least one image) is made."""
    per = stc_workspace_bytes(hw, h)
    cap = STC_WORKSPACE_CAP if workspace_cap is None else int(workspace_cap)
    if cap < 1:
        raise ValueError(f"{who}: workspace_cap={workspace_cap!r} is not a positive byte count")
    if workspace is not None:
        _dev_check(workspace)
        if workspace.dtype != torch.uint8 or workspace.numel() < n * per:
            raise ValueError(f"{who}: workspace must be uint8 with at least {n * per} bytes")
        return per, n, workspace
    step = max(1, min(n, cap // per))
    return per, step, torch.empty(step * per, dtype=torch.uint8, device=dev)


def _stc_embed_slices(who: str, cover_u8: torch.Tensor, seeds: torch.Tensor, change: str, h: int, workspace_cap, workspace, call, phases: int = 3):
    """What stc_embed and stc_embed_ragged share: the seeds, the change and the phases, the outputs, and the loop over the slices of the
    batch.  call(a, b, change id, tail) runs wsu_<who> on images a .. b - 1; `tail` is what both entries end with, from `stego` on."""
    n, hh, ww = cover_u8.shape
    _vector(who, "seeds", seeds, n, torch.int64)
    if change not in STC_CHANGES:
        raise ValueError(f"{who}: change {change!r} is not one of {' / '.join(STC_CHANGES)}")
    if phases not in (1, 3) or (phases == 1 and workspace is None):
        raise ValueError(f"{who}: phases is 1 (forward only, into the caller's workspace) or 3 (both)")
    dev = cover_u8.device
    per, step, ws = _stc_slices(who, n, hh * ww, h, workspace_cap, workspace, dev)
    stego = torch.empty_like(cover_u8)
    cost = torch.empty(n, dtype=torch.float64, device=dev)
    changes = torch.zeros(n, dtype=torch.int64, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    cid = STC_CHANGES.index(change)
    for a in range(0, n, step):
        b = min(n, a + step)
        tail = (stego[a:b].data_ptr(), cost[a:b].data_ptr(), changes[a:b].data_ptr(), ok[a:b].data_ptr(), ws.data_ptr(), ws.numel(), b - a, hh, ww,
                _stream())
        check(_launch(who, {"bytes": float((b - a) * (hh * ww * 14 + 2 * per))}, lambda: call(a, b, cid, tail)), "wsu_" + who)
    return stego, cost, changes, ok


def stc_embed(cover_u8: torch.Tensor, rho: torch.Tensor, message: torch.Tensor, cols: torch.Tensor, seeds: torch.Tensor, *, h: int = 10,
              path: Optional[torch.Tensor] = None, change: str = "flip", workspace_cap: Optional[int] = None, phases: int = 3,
              workspace: Optional[torch.Tensor] = None):
    """Embeds a message with a binary syndrome-trellis code (K41): the Viterbi pass over 2^h states per pixel and the walk back.  cover_u8:
    (N,H,W) uint8; rho: (N,H,W) float64 costs, >= 0, +inf = wet; message: (N,k) uint8 of 0 / 1, 1 <= k <= H W; cols: int32 column table
    with at least ceil(H W / k) entries (stc.columns); seeds: (N) int64 holding the 64-bit seeds (they choose the sign of a 'pm1' change);
    path: (N, H W) int32, per image a permutation of the raster indices, or None for raster order; change: 'flip' (x ^ 1) or 'pm1' (x +- 1,
    inwards at 0 and 255) where the coded LSB differs from the cover's -> (stego (N,H,W) uint8, cost (N) float64, changes (N) int64, ok (N)
    uint8).  cost is the least total cost of a stego with this syndrome; where it is +inf (too many wet pixels) ok is 0 and the stego is
    the cover.  Bit for bit a numpy restatement.  The batch is cut into slices whose take bits fit `workspace_cap` bytes
    (STC_WORKSPACE_CAP by default; a slice holds at least one image).  phases=1 runs only the forward pass: cost and ok are final, stego
    and changes are not written, and the take bits stay in the caller's `workspace` (uint8, N * stc_workspace_bytes(H W, h) bytes, which
    also turns the slicing off) for a later walk back through the C entry (phases 2 there reads cost and ok as arguments)."""
    lib = _lib.load()
    n, hh, ww = _f64_planes("stc_embed", cover_u8, rho)
    if not (isinstance(message, torch.Tensor) and message.dtype == torch.uint8 and message.dim() == 2 and message.shape[0] == n):
        raise ValueError(f"stc_embed: message must be an ({n}, k) uint8 tensor of 0 / 1")
    h, k = _stc_code("stc_embed", n, hh * ww, h, message.shape[1], cols, path)
    _dev_check(message)
    return _stc_embed_slices("stc_embed", cover_u8, seeds, change, h, workspace_cap, workspace, lambda a, b, cid, tail: lib.wsu_stc_embed(
        cover_u8[a:b].data_ptr(), rho[a:b].data_ptr(), message[a:b].data_ptr(), cols.data_ptr(), _ptr(path[a:b] if path is not None else None),
        seeds[a:b].data_ptr(), cid, h, k, phases, *tail), phases)


def stc_extract(stego_u8: torch.Tensor, cols: torch.Tensor, k: int, *, h: int = 10, path: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Reads the k message bits a syndrome-trellis code left in the LSBs (K42): stego_u8: (N,H,W) uint8; cols, h, path as stc_embed was
    given them -> (N,k) uint8 of 0 / 1."""
    lib = _lib.load()
    n, hh, ww = _u8_planes(stego_u8)
    h, k = _stc_code("stc_extract", n, hh * ww, h, k, cols, path)
    message = torch.empty((n, k), dtype=torch.uint8, device=stego_u8.device)
    check(_launch("stc_extract", {"bytes": float(n * hh * ww * 5)}, lambda: lib.wsu_stc_extract(
        stego_u8.data_ptr(), cols.data_ptr(), _ptr(path), h, k, message.data_ptr(), n, hh, ww, _stream())), "wsu_stc_extract")
    return message


# ---- ragged codes and the two-layer planes (K43-K47) ---------------------------------------------------------------------------------

def _stc_ragged(who: str, n: int, hw: int, h, message: torch.Tensor, ks: torch.Tensor, first: Optional[torch.Tensor], cols: torch.Tensor,
                path: Optional[torch.Tensor]) -> Tuple[int, torch.Tensor]:
    """The checks of _stc_code for per-image lengths; what ks and first hold stays on the device, where the kernels check it."""
    h = _stc_height(who, h)
    if not (isinstance(message, torch.Tensor) and message.dtype == torch.uint8 and message.dim() == 2 and message.shape[0] == n
            and message.shape[1] >= 1):
        raise ValueError(f"{who}: message must be an ({n}, bits) uint8 tensor of 0 / 1")
    if not (isinstance(ks, torch.Tensor) and ks.dtype == torch.int32 and ks.shape == (n,)):
        raise ValueError(f"{who}: ks must be an int32 tensor of shape ({n},): the message bits of each image")
    if first is None:
        first = torch.zeros(n, dtype=torch.int32, device=ks.device)
    if not (isinstance(first, torch.Tensor) and first.dtype == torch.int32 and first.shape == (n,)):
        raise ValueError(f"{who}: first must be an int32 tensor of shape ({n},): the first bit of each row that is used")
    _dev_check(message, ks, first)
    _stc_table(who, n, hw, cols, path, 1, "ceil(n / k) entries for the smallest positive k")
    return h, first


def stc_embed_ragged(cover_u8: torch.Tensor, rho: torch.Tensor, message: torch.Tensor, cols: torch.Tensor, seeds: torch.Tensor, *,
                     ks: torch.Tensor, first: Optional[torch.Tensor] = None, h: int = 10, path: Optional[torch.Tensor] = None,
                     change: str = "flip", workspace_cap: Optional[int] = None):
    """stc_embed with a message length per image (K43): image i embeds the ks[i] bits message[i, first[i] : first[i] + ks[i]].  message:
    (N,B) uint8; ks, first: (N) int32 on the device, 0 <= ks[i] <= H W, first[i] + ks[i] <= B (first:
    zeros when None); cols: at least ceil(H W / k) entries for the smallest positive k -> (stego, cost, changes, ok) as stc_embed.
    ks[i] == 0 copies the image: cost 0, ok 1.  Nothing is read back, so values of ks / first outside these ranges are found by the
    kernel: such an image is copied and has cost +inf and ok 0.  With all ks equal the results are stc_embed's bit for bit."""
    lib = _lib.load()
    n, hh, ww = _f64_planes("stc_embed_ragged", cover_u8, rho)
    h, first = _stc_ragged("stc_embed_ragged", n, hh * ww, h, message, ks, first, cols, path)
    bits, stride = message.shape[1], message.stride(0)
    return _stc_embed_slices("stc_embed_ragged", cover_u8, seeds, change, h, workspace_cap, None, lambda a, b, cid, tail: lib.wsu_stc_embed_ragged(
        cover_u8[a:b].data_ptr(), rho[a:b].data_ptr(), message[a:b].data_ptr(), stride, ks[a:b].data_ptr(), first[a:b].data_ptr(), bits,
        cols.data_ptr(), cols.shape[0], _ptr(path[a:b] if path is not None else None), seeds[a:b].data_ptr(), cid, h, *tail))


def stc_extract_ragged(stego_u8: torch.Tensor, cols: torch.Tensor, *, ks: torch.Tensor, first: Optional[torch.Tensor] = None, bits: Optional[int] = None,
                       bit: int = 0, h: int = 10, path: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """stc_extract with a message length per image (K44): reads ks[i] bits of image i from bit `bit` (0..7) of its bytes into
    out[i, first[i] : first[i] + ks[i]].  out: (N,B) uint8 on the device, written only there (several calls can fill one row); when None a
    zeroed (N, bits) tensor is made.  ks, first, cols, h, path as stc_embed_ragged was given them; an image with ks[i] == 0 or with
    values out of range writes nothing."""
    lib = _lib.load()
    n, hh, ww = _u8_planes(stego_u8)
    if out is None:
        if bits is None or int(bits) < 1:
            raise ValueError("stc_extract_ragged: give `out`, or `bits` >= 1 for the width of a new one")
        out = torch.zeros((n, int(bits)), dtype=torch.uint8, device=stego_u8.device)
    h, first = _stc_ragged("stc_extract_ragged", n, hh * ww, h, out, ks, first, cols, path)
    bit = int(bit)
    if not 0 <= bit <= 7:
        raise ValueError(f"stc_extract_ragged: bit={bit} outside 0..7")
    check(_launch("stc_extract_ragged", {"bytes": float(n * hh * ww * 5)}, lambda: lib.wsu_stc_extract_ragged(
        stego_u8.data_ptr(), cols.data_ptr(), cols.shape[0], _ptr(path), h, bit, ks.data_ptr(), first.data_ptr(), out.shape[1], out.data_ptr(),
        out.stride(0), n, hh, ww, _stream())), "wsu_stc_extract_ragged")
    return out


def _layer_workspace(n: int, dev) -> torch.Tensor:
    return torch.empty(_lib.load().wsu_stc_layer_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)


def _layer_plane(who: str, name: str, t: torch.Tensor, like: torch.Tensor) -> None:
    _dev_check(t)
    if t.dtype != torch.uint8 or t.shape != like.shape:
        raise ValueError(f"{who}: {name} must be uint8 of shape {tuple(like.shape)}, got {tuple(t.shape)} {t.dtype}")


def stc_layer_high(x_u8: torch.Tensor, rho: torch.Tensor, lambdas: torch.Tensor):
    """The high layer of the two-layer +-1 code (K45): x_u8: (N,H,W) uint8; rho: (N,H,W) float64, >= 0, +inf = wet; lambdas: (N) float64
    (ternary_lambda's lam_lo) -> (u1 (N,H,W) uint8 = bit 1 of the pixels, rho1 (N,H,W) float64 = the cost of changing it, H1 (N) float64 =
    the layer's entropy in bits).  include/wsu.h has the formulas.  The same bits in every batch."""
    lib = _lib.load()
    n, h, w = _f64_planes("stc_layer_high", x_u8, rho)
    _vector("stc_layer_high", "lambdas", lambdas, n, torch.float64)
    dev = x_u8.device
    u1 = torch.empty_like(x_u8)
    rho1 = torch.empty_like(rho)
    ent = torch.empty(n, dtype=torch.float64, device=dev)
    ws = _layer_workspace(n, dev)
    check(_launch("stc_layer_high", {"bytes": float(n * h * w * 18)}, lambda: lib.wsu_stc_layer_high(
        x_u8.data_ptr(), rho.data_ptr(), lambdas.data_ptr(), u1.data_ptr(), rho1.data_ptr(), ent.data_ptr(), ws.data_ptr(), ws.numel() * 8,
        n, h, w, _stream())), "wsu_stc_layer_high")
    return u1, rho1, ent


def stc_layer_low(x_u8: torch.Tensor, rho: torch.Tensor, lambdas: torch.Tensor, y1: torch.Tensor, k1: torch.Tensor):
    """The low layer's planes (K46): y1: (N,H,W) uint8, the high layer's solution (bit 0 of each byte; not read where k1[i] <= 0); k1: (N)
    int32 -> (u0 (N,H,W) uint8, rho0 (N,H,W) float64): a pixel whose bit 1 changed is decided (u0 = the other LSB, rho0 = +inf), every
    other keeps its LSB at cost lambda rho."""
    lib = _lib.load()
    n, h, w = _f64_planes("stc_layer_low", x_u8, rho)
    _vector("stc_layer_low", "lambdas", lambdas, n, torch.float64)
    _layer_plane("stc_layer_low", "y1", y1, x_u8)
    _vector("stc_layer_low", "k1", k1, n, torch.int32)
    u0 = torch.empty_like(x_u8)
    rho0 = torch.empty_like(rho)
    check(_launch("stc_layer_low", {"bytes": float(n * h * w * 19)}, lambda: lib.wsu_stc_layer_low(
        x_u8.data_ptr(), rho.data_ptr(), lambdas.data_ptr(), y1.data_ptr(), k1.data_ptr(), u0.data_ptr(), rho0.data_ptr(),
        n, h, w, _stream())), "wsu_stc_layer_low")
    return u0, rho0


def stc_layer_compose(cover_u8: torch.Tensor, rho: torch.Tensor, y1: torch.Tensor, y0: torch.Tensor, k1: torch.Tensor, ok1: torch.Tensor,
                      ok0: torch.Tensor):
    """The stego image of the two layers' solutions (K47): x + d where bit 1 changed (d: +1 for odd x, -1 for even x), x - d where only
    the LSB did, in images whose ok1 and ok0 (N, uint8) are both set; every other image is copied -> (stego (N,H,W) uint8, changes (N)
    int64, distortion (N) float64 = the sum of rho over the changed pixels in a fixed order, ok (N) uint8)."""
    lib = _lib.load()
    n, h, w = _f64_planes("stc_layer_compose", cover_u8, rho)
    _layer_plane("stc_layer_compose", "y1", y1, cover_u8)
    _layer_plane("stc_layer_compose", "y0", y0, cover_u8)
    _vector("stc_layer_compose", "k1", k1, n, torch.int32)
    _vector("stc_layer_compose", "ok1", ok1, n, torch.uint8)
    _vector("stc_layer_compose", "ok0", ok0, n, torch.uint8)
    dev = cover_u8.device
    stego = torch.empty_like(cover_u8)
    changes = torch.empty(n, dtype=torch.int64, device=dev)
    dist = torch.empty(n, dtype=torch.float64, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = _layer_workspace(n, dev)
    check(_launch("stc_layer_compose", {"bytes": float(n * h * w * 12)}, lambda: lib.wsu_stc_layer_compose(
        cover_u8.data_ptr(), rho.data_ptr(), y1.data_ptr(), y0.data_ptr(), k1.data_ptr(), ok1.data_ptr(), ok0.data_ptr(),
        stego.data_ptr(), changes.data_ptr(), dist.data_ptr(), ok.data_ptr(), ws.data_ptr(), ws.numel() * 8, n, h, w, _stream())),
        "wsu_stc_layer_compose")
    return stego, changes, dist, ok


def prediction_error(x_u8: torch.Tensor, x_hat: Optional[torch.Tensor] = None, *, pixel_filter=None, hat_scale: float = 255.,
                     quantile: float = 0.1, cost: Optional[torch.Tensor] = None, return_threshold: bool = False):
    """Per-image MAE and HILL-cost weighted MAE of a pixel prediction on the interior [1:-1,1:-1] (K12-K14).
    x_u8: (N,H,W) uint8.  x_hat: (N,H,W)/(N,1,H,W) full-frame prediction or (N,H-2,W-2) interior prediction, multiplied by
    `hat_scale` (255 for a network output in [0,1]); or `pixel_filter` (8 flattened taps or a (3,3[,1]) kernel, see filter_taps)
    evaluated in float64 inside the kernel.  `cost` reuses a hill_cost() map.  Returns (mae[N], wmae[N]) fp64 on the device,
    plus (q[N] fp64, selected[N] int64) with return_threshold=True."""
    lib = _lib.load()
    _dev_check(x_u8, x_hat, cost)
    assert x_u8.dtype == torch.uint8 and x_u8.dim() == 3
    n, h, w = x_u8.shape
    if (x_hat is None) == (pixel_filter is None):
        raise ValueError("give exactly one of x_hat / pixel_filter")
    hat_full = _hat_full(x_hat, n, h, w) if x_hat is not None else 1
    pt = filter_taps(pixel_filter, np.float64, "weights", "2d 8")
    if cost is None:
        cost = hill_cost(x_u8)
    assert cost.dtype == torch.float32 and cost.shape == x_u8.shape
    q = hill_threshold(cost, quantile)
    mae = torch.empty(n, dtype=torch.float64, device=x_u8.device)
    wmae = torch.empty(n, dtype=torch.float64, device=x_u8.device)
    sel = torch.empty(n, dtype=torch.int64, device=x_u8.device)
    ws = torch.empty(lib.wsu_prediction_error_workspace_bytes(n) // 8, dtype=torch.float64, device=x_u8.device)
    check(_launch("prediction_error", {"bytes": float(n * h * w * (9 if x_hat is not None else 5))}, lambda: lib.wsu_prediction_error(
        x_u8.data_ptr(), x_hat.data_ptr() if x_hat is not None else None, pt.ctypes.data if pt is not None else None,
        hat_full, float(hat_scale), cost.data_ptr(), q.data_ptr(), mae.data_ptr(), wmae.data_ptr(), sel.data_ptr(),
        ws.data_ptr(), ws.numel() * 8, n, h, w, _stream())), "wsu_prediction_error")
    return (mae, wmae, q, sel) if return_threshold else (mae, wmae)


def pair_correlation(xc_u8: torch.Tensor, xs_u8: torch.Tensor, x_hat: Optional[torch.Tensor] = None, *, pixel_filter=None,
                     hat_full: bool = True, hat_scale: float = 255., moments: bool = False):
    """Per-pair correlation of a cover estimate made from the stego plane with the embedding change (K15, src/correlation.py:22-59):
    cor = (sum((dhat - mean dhat)(d - mean d)) / (n-1)) / std(xhat) / std(d) on the interior, d = x_s - x_c, dhat = xhat - x_c.
    xc_u8, xs_u8: (N,H,W) uint8.  x_hat: (N,H,W) / (N,1,H,W) full-frame prediction (hat_full=True; a network output in [0,1], scaled by
    `hat_scale` in float32) or (N,H-2,W-2) interior prediction in grey levels (hat_full=False, hat_scale=1.); or `pixel_filter`, a
    (3,3[,1]) kernel array in K11's layout, evaluated on the stego plane in float64 inside the kernel.  Returns cor[N] fp64 on the
    device, plus the (N,6) fp64 moments {mean xhat, mean dhat, mean d, S_hd, S_hh, S_dd} with moments=True."""
    lib = _lib.load()
    _dev_check(xc_u8, xs_u8, x_hat)
    if xc_u8.dtype != torch.uint8 or xs_u8.dtype != torch.uint8 or xc_u8.dim() != 3 or xs_u8.shape != xc_u8.shape:
        raise ValueError(f"cover / stego planes must be two (N,H,W) uint8 tensors of one shape, got {tuple(xc_u8.shape)} {xc_u8.dtype} "
                         f"and {tuple(xs_u8.shape)} {xs_u8.dtype}")
    n, h, w = xc_u8.shape
    if (x_hat is None) == (pixel_filter is None):
        raise ValueError("give exactly one of x_hat / pixel_filter")
    if x_hat is not None:
        _hat_full(x_hat, n, h, w, bool(hat_full))
    pt = filter_taps(pixel_filter, np.float64, "kernel")           # K11's layout, kept in float64 (no float32 rounding of the taps)
    cor = torch.empty(n, dtype=torch.float64, device=xc_u8.device)
    mom = torch.empty((n, 6), dtype=torch.float64, device=xc_u8.device) if moments else None
    ws = torch.empty(lib.wsu_pair_correlation_workspace_bytes(n) // 8, dtype=torch.float64, device=xc_u8.device)
    check(_launch("pair_correlation", {"bytes": float(n * h * w * (2 if x_hat is None else 6) * 2)}, lambda: lib.wsu_pair_correlation(
        xc_u8.data_ptr(), xs_u8.data_ptr(), x_hat.data_ptr() if x_hat is not None else None, pt.ctypes.data if pt is not None else None,
        int(bool(hat_full)), float(hat_scale), cor.data_ptr(), mom.data_ptr() if mom is not None else None, ws.data_ptr(), ws.numel() * 8,
        n, h, w, _stream())), "wsu_pair_correlation")
    return (cor, mom) if moments else cor


def ae_values(x_u8: torch.Tensor, keys: torch.Tensor, offset: int, flag: torch.Tensor, x_hat: Optional[torch.Tensor] = None, *,
              pixel_filter=None, hat_scale: float = 255., idx: Optional[torch.Tensor] = None) -> None:
    """K16: the float32 absolute error of one predictor on the interior of (N,H,W) uint8 planes, written into the 1-D float32 `keys`
    at `offset` + i*per + j (per = idx.shape[1], or (H-2)(W-2)).  The predictor is a full-frame `x_hat` ((N,H,W) / (N,1,H,W) fp32,
    times `hat_scale`: |x - x_hat*255| in float32) or `pixel_filter` (9 weights of x[r-1+a][c-1+b], 8 flattened taps or a
    (3,3[,1]) kernel, see filter_taps; |y - x @ f| in float64).  idx: optional
    (N,m) int64 interior indices.  flag: a 1-element int32 device tensor, OR-ed with 1 on NaN / inf, 2 on a bad index."""
    lib = _lib.load()
    _dev_check(x_u8, keys, flag, x_hat, idx)
    if x_u8.dtype != torch.uint8 or x_u8.dim() != 3 or keys.dtype != torch.float32 or keys.dim() != 1 or not keys.is_contiguous():
        raise ValueError(f"(N,H,W) uint8 planes and a contiguous 1-D float32 key array expected, got {tuple(x_u8.shape)} {x_u8.dtype}, "
                         f"{tuple(keys.shape)} {keys.dtype}")
    n, h, w = x_u8.shape
    if (x_hat is None) == (pixel_filter is None):
        raise ValueError("give exactly one of x_hat / pixel_filter")
    if x_hat is not None:
        _hat_full(x_hat, n, h, w, True)
    m = 0
    if idx is not None:
        if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != n or not idx.is_contiguous():
            raise ValueError(f"idx must be a contiguous (N,m) int64 tensor, got {tuple(idx.shape)} {idx.dtype}")
        m = int(idx.shape[1])
    pt = filter_taps(pixel_filter, np.float64, "weights", "2d 8 9")
    per = m if m else (h - 2) * (w - 2)
    check(_launch("ae_values", {"bytes": float(n * (h * w * (5 if x_hat is not None else 1) + per * 4))}, lambda: lib.wsu_ae_values(
        x_u8.data_ptr(), x_hat.data_ptr() if x_hat is not None else None, pt.ctypes.data if pt is not None else None, float(hat_scale),
        idx.data_ptr() if idx is not None else None, m, keys.data_ptr(), int(offset), keys.numel(), flag.data_ptr(), n, h, w,
        _stream())), "wsu_ae_values")


def ae_slices(anchor_keys: torch.Tensor, edges, count: Optional[int] = None) -> torch.Tensor:
    """K17 over the first `count` (default: all) anchor keys: a (len(edges)+1, 3) uint64-valued int64 device tensor, row j
    {#(a <= e_j), float32 bits of max{a <= e_j}, largest index holding it + 1}, last row {0, bits of max a, its largest index + 1}."""
    lib = _lib.load()
    _dev_check(anchor_keys)
    if anchor_keys.dtype != torch.float32 or anchor_keys.dim() != 1 or not anchor_keys.is_contiguous():
        raise ValueError(f"a contiguous 1-D float32 key array expected, got {tuple(anchor_keys.shape)} {anchor_keys.dtype}")
    count = anchor_keys.numel() if count is None else int(count)
    if not 0 < count <= anchor_keys.numel():
        raise ValueError(f"count={count} outside (0, {anchor_keys.numel()}] of the anchor keys")
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
    out = torch.empty((len(e) + 1, 3), dtype=torch.int64, device=anchor_keys.device)
    check(_launch("ae_slices", {"bytes": float(count * 8)}, lambda: lib.wsu_ae_slices(
        anchor_keys.data_ptr(), count, e.ctypes.data, len(e), out.data_ptr(), _stream())), "wsu_ae_slices")
    return out


def ae_select(keys: torch.Tensor, anchor: int, slices, count: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """K18: exact order statistics per (predictor, slice).  keys: (P, stride) float32 device tensor (the first `count` of each row);
    slices: host int64 (S, 10) descriptors (include/wsu.h).  Returns (out (P,S,8) int32 device tensor of float32 bit patterns
    {min, max, c_(k0), c_(k0+1), c_(k1), c_(k1+1), c_(k2), c_(k2+1)}, flags (P,) int32: 1 where a key is negative or not finite)."""
    lib = _lib.load()
    _dev_check(keys)
    if keys.dtype != torch.float32 or keys.dim() != 2 or not keys.is_contiguous():
        raise ValueError(f"a contiguous (P, N) float32 key array expected, got {tuple(keys.shape)} {keys.dtype}")
    p, stride = keys.shape
    count = stride if count is None else int(count)
    sl = np.ascontiguousarray(np.asarray(slices, dtype=np.int64))
    if sl.ndim != 2 or sl.shape[1] != 10:
        raise ValueError(f"(S, 10) slice descriptors expected, got {sl.shape}")
    out = torch.empty((p, sl.shape[0], 8), dtype=torch.int32, device=keys.device)
    flags = torch.empty(p, dtype=torch.int32, device=keys.device)
    ws = torch.empty(lib.wsu_ae_select_workspace_bytes(p) // 8, dtype=torch.int64, device=keys.device)
    check(_launch("ae_select", {"bytes": float(p * count * 8 * 8)}, lambda: lib.wsu_ae_select(
        keys.data_ptr(), stride, p, int(anchor), count, sl.ctypes.data, sl.shape[0], out.data_ptr(), flags.data_ptr(), ws.data_ptr(),
        ws.numel() * 8, _stream())), "wsu_ae_select")
    return out, flags


def roc_counts(scores: torch.Tensor, labels: torch.Tensor, offsets, taus) -> torch.Tensor:
    """K19: exact confusion counts of a threshold sweep over G groups of scores (include/wsu.h).  scores: contiguous 1-D float64 device
    tensor; labels: contiguous 1-D int8 device tensor of the same length (1 positive, 0 negative, -1 neither); offsets: host int64 (G+1,)
    group bounds (offsets[0] = 0, non-decreasing, offsets[-1] = len(scores)); taus: host float64 (T,), finite, strictly ascending,
    T <= 4096.  Returns a (G, T, 4) int64 device tensor {TP, FP, TN, FN}: a score counts as above tau_j iff s > tau_j in float64, a NaN
    score or a -1 label in none of the four."""
    lib = _lib.load()
    for name, t, dt in (("scores", scores, torch.float64), ("labels", labels, torch.int8)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-D {dt} tensor, got {getattr(t, 'dtype', type(t))} of shape {tuple(getattr(t, 'shape', ()))}")
        if not t.is_cuda:
            raise ValueError(f"{name} must be on the GPU (no CPU fallback exists)")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if labels.numel() != scores.numel() or labels.device != scores.device:
        raise ValueError(f"labels ({labels.numel()} on {labels.device}) must match scores ({scores.numel()} on {scores.device})")
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    tau = np.ascontiguousarray(np.asarray(taus, dtype=np.float64).reshape(-1))
    if off.size < 2 or off[-1] != scores.numel():
        raise ValueError(f"offsets must hold G+1 >= 2 bounds ending at len(scores)={scores.numel()}, got {off.tolist()[:8]}")
    groups = off.size - 1
    counts = torch.empty((groups, tau.size, 4), dtype=torch.int64, device=scores.device)
    nbytes = lib.wsu_roc_counts_workspace_bytes(groups, tau.size)
    ws = torch.empty(max(1, nbytes // 8), dtype=torch.int64, device=scores.device)
    check(_launch("roc_counts", {"bytes": float(scores.numel() * 9)}, lambda: lib.wsu_roc_counts(
        scores.data_ptr() or None, labels.data_ptr() or None, off.ctypes.data, groups, tau.ctypes.data, tau.size, counts.data_ptr(),
        ws.data_ptr(), nbytes, _stream())), "wsu_roc_counts")
    return counts


def filter3x3_valid(x: torch.Tensor, kernel) -> torch.Tensor:
    """x: (N,H,W) fp32 -> (N,H-2,W-2) fp32 = convolve(x/255., K, 'valid')*255. (wsu_filter3x3_valid_f32)."""
    lib = _lib.load()
    _dev_check(x)
    assert x.dtype == torch.float32 and x.dim() == 3
    n, h, w = x.shape
    k = filter_taps(kernel, np.float32, "kernel")
    y = torch.empty((n, h - 2, w - 2), dtype=torch.float32, device=x.device)
    check(lib.wsu_filter3x3_valid_f32(x.data_ptr(), k.ctypes.data, y.data_ptr(), n, h, w, _stream()), "wsu_filter3x3_valid_f32")
    return y


def lsb_delta_unit(x_u8: torch.Tensor) -> torch.Tensor:
    """((x ^ 1) - x) / 255. as fp32, same shape."""
    lib = _lib.load()
    _dev_check(x_u8)
    y = torch.empty(x_u8.shape, dtype=torch.float32, device=x_u8.device)
    check(lib.wsu_lsb_delta_unit_f32(x_u8.data_ptr(), y.data_ptr(), x_u8.numel(), _stream()), "wsu_lsb_delta_unit_f32")
    return y


def ws_meter_beta(x01: torch.Tensor, y01: torch.Tensor) -> torch.Tensor:
    """WSMeter's per-image beta_hat (fp64, interior crop) from float inputs / outputs of shape (N,1,H,W) or (N,H,W)."""
    lib = _lib.load()
    _dev_check(x01, y01)
    assert x01.dtype == torch.float32 and y01.dtype == torch.float32 and x01.numel() == y01.numel()
    n, h, w = x01.shape[0], x01.shape[-2], x01.shape[-1]
    assert x01.numel() == n * h * w, "single-plane images expected"
    beta = torch.empty(n, dtype=torch.float64, device=x01.device)
    check(lib.wsu_ws_meter_beta(x01.data_ptr(), y01.data_ptr(), beta.data_ptr(), n, h, w, _stream()), "wsu_ws_meter_beta")
    return beta


def u8_to_unit(x_u8: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _dev_check(x_u8)
    y = torch.empty(x_u8.shape, dtype=torch.float32, device=x_u8.device)
    check(lib.wsu_u8_to_unit_f32(x_u8.data_ptr(), y.data_ptr(), x_u8.numel(), _stream()), "wsu_u8_to_unit_f32")
    return y


def _pair_batch_args(who: str, planes_u8: torch.Tensor, idx_in, idx_cov, op):
    """Validation shared by pair_batch and pair_batch_planes -> (files, h, w, n, device block [idx_in int32 | idx_cov int32 | op uint8] or None
    for n == 0).  ValueError for an index outside [0, files), an op outside 0..7 or an op >= 4 on non-square planes; one upload."""
    _dev_check(planes_u8)
    if planes_u8.dim() != 3 or planes_u8.dtype != torch.uint8:
        raise ValueError(f"{who}: planes_u8 must be a (files,H,W) uint8 tensor")
    files, h, w = planes_u8.shape
    ii, ic, o = (np.asarray(v).reshape(-1) for v in (idx_in, idx_cov, op))
    n = ii.shape[0]
    if ic.shape[0] != n or o.shape[0] != n:
        raise ValueError(f"{who}: {n} input indices, {ic.shape[0]} cover indices and {o.shape[0]} ops")
    if n == 0:
        return files, h, w, 0, None
    for name, v in (("idx_in", ii), ("idx_cov", ic)):
        if not np.issubdtype(v.dtype, np.integer) or v.min() < 0 or v.max() >= files:
            raise ValueError(f"{who}: {name} outside [0, {files})")
    if not np.issubdtype(o.dtype, np.integer) or o.min() < 0 or o.max() > 7:
        raise ValueError(f"{who}: op outside 0..7")
    if h != w and o.max() >= 4:
        raise ValueError(f"{who}: transposing ops (op >= 4) need square planes, got {h}x{w}")
    host = np.empty(9 * n, dtype=np.uint8)
    host[:4 * n].view(np.int32)[:] = ii
    host[4 * n:8 * n].view(np.int32)[:] = ic
    host[8 * n:] = o
    return files, h, w, n, torch.from_numpy(host).to(planes_u8.device)


def pair_batch(planes_u8: torch.Tensor, idx_in, idx_cov, op) -> Tuple[torch.Tensor, torch.Tensor]:
    """One training batch in one launch (wsu_pair_batch_f32): planes_u8 (files,H,W) uint8 on the device; idx_in, idx_cov, op: HOST sequences
    or arrays, one entry per sample -> (inputs, covers), both (n,1,H,W) fp32 with inputs[s] = D(op[s])(planes[idx_in[s]]) / 255 and
    covers[s] = D(op[s])(planes[idx_cov[s]]) / 255.  op: bit 0 mirrors the columns, bit 1 the rows, bit 2 transposes last (include/wsu.h).
    ValueError for an index outside [0, files), an op outside 0..7 or an op >= 4 on non-square planes; the three arrays go up in one copy."""
    lib = _lib.load()
    files, h, w, n, args = _pair_batch_args("pair_batch", planes_u8, idx_in, idx_cov, op)
    inputs = torch.empty((n, 1, h, w), dtype=torch.float32, device=planes_u8.device)
    covers = torch.empty((n, 1, h, w), dtype=torch.float32, device=planes_u8.device)
    if n == 0:
        return inputs, covers
    p = args.data_ptr()
    check(lib.wsu_pair_batch_f32(planes_u8.data_ptr(), files, h, w, p, p + 4 * n, p + 8 * n, n, int(h == w), inputs.data_ptr(),
                                 covers.data_ptr(), _stream()), "wsu_pair_batch_f32")
    return inputs, covers


def side_plane_count(parity: bool = False, demosaic: bool = False) -> int:
    """Planes of a network input with the given side information: the image, the parity plane, the three demosaic planes."""
    return 1 + int(bool(parity)) + 3 * int(bool(demosaic))


def _pair_batch_planes(planes_u8: torch.Tensor, idx_in, idx_cov, op, side: int, want_covers: bool):
    lib = _lib.load()
    if not 0 <= int(side) <= 3:
        raise ValueError(f"pair_batch_planes: side={side} outside 0..3")
    files, h, w, n, args = _pair_batch_args("pair_batch_planes", planes_u8, idx_in, idx_cov if want_covers else idx_in, op)
    inputs = torch.empty((n, side_plane_count(side & 1, side & 2), h, w), dtype=torch.float32, device=planes_u8.device)
    covers = torch.empty((n, 1, h, w), dtype=torch.float32, device=planes_u8.device) if want_covers else None
    if n == 0:
        return inputs, covers
    p = args.data_ptr()
    check(lib.wsu_pair_batch_planes_f32(planes_u8.data_ptr(), files, h, w, p, p + 4 * n if want_covers else None, p + 8 * n, n, int(h == w),
                                        int(side), inputs.data_ptr(), _ptr(covers), _stream()), "wsu_pair_batch_planes_f32")
    return inputs, covers


def pair_batch_planes(planes_u8: torch.Tensor, idx_in, idx_cov, op, parity: bool = False, demosaic: bool = False):
    """ops.pair_batch with side-information planes behind the image, still one launch (wsu_pair_batch_planes_f32): inputs (n,P,H,W) with
    P = 1 + parity + 3 * demosaic planes in the reference's transform order -- image / 255, the LSB plane (ParityOracle), the R, G, B site
    indicators of the RGGB grid (DemosaicOracle) -- and covers (n,1,H,W).  The side planes are functions of the SOURCE pixel, i.e. they are
    transformed with the image as the reference's are (include/wsu.h).  Plane 0 and covers are ops.pair_batch's, bit for bit; so is the
    validation.  idx_cov=None: no covers are made (returns (inputs, None))."""
    return _pair_batch_planes(planes_u8, idx_in, idx_cov, op, int(bool(parity)) + 2 * int(bool(demosaic)), idx_cov is not None)


def side_planes(x_u8: torch.Tensor, parity: bool, demosaic: bool) -> torch.Tensor:
    """(N,H,W) uint8 device planes -> the network input (N,P,H,W) fp32 with the side-information planes (pair_batch_planes with identity
    indices, op 0 and no covers output)."""
    n = x_u8.shape[0]
    return pair_batch_planes(x_u8, np.arange(n, dtype=np.int32), None, np.zeros(n, dtype=np.uint8), parity, demosaic)[0]


# ---- backward ops (fp32 storage; g = pre-activation gradient, NHWC) -------------------------------------

_ws_cache = {}


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer per device (fp32 view), reused by all backward reductions on the stream."""
    key = str(device)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        _ws_cache[key] = buf
    return buf


def pack_convt2x2_dgrad(w: torch.Tensor, mode: int) -> torch.Tensor:
    lib = _lib.load()
    w = w.detach()
    _dev_check(w)
    cin, cout = w.shape[:2]
    out = torch.empty(lib.wsu_convt2x2_packed_dgrad_bytes(cin, cout, mode), dtype=torch.uint8, device=w.device)
    check(lib.wsu_convt2x2_pack_dgrad(w.data_ptr(), out.data_ptr(), cin, cout, mode, _stream()), "wsu_convt2x2_pack_dgrad")
    return out


def conv3x3_bwd_data(g: torch.Tensor, w_packed_dgrad: torch.Tensor, w_oihw: torch.Tensor, csplit: int,
                     mask1: Optional[torch.Tensor], mask2: Optional[torch.Tensor], mode: int):
    """Returns dx1 (N,H,W,csplit) and dx2 (N,H,W,cin-csplit) or None."""
    lib = _lib.load()
    w_oihw = w_oihw.detach()
    _dev_check(g, w_packed_dgrad, w_oihw, mask1, mask2)
    n, h, w, cout = g.shape
    cin = w_oihw.shape[1]
    assert g.dtype == torch.float32 and w_oihw.shape[0] == cout
    dx1 = torch.empty((n, h, w, csplit), dtype=torch.float32, device=g.device)
    dx2 = torch.empty((n, h, w, cin - csplit), dtype=torch.float32, device=g.device) if csplit < cin else None
    meta = {"flops": 2.0 * 9 * cin * cout * n * h * w}
    nbytes = lib.wsu_conv3x3_bwd_data_workspace_bytes(n, h, w, cin, cout, mode)
    ws = workspace(nbytes, g.device)                          # border strips + tap-swapped weights (fp32 view, grow-only)
    check(_launch("conv3x3_bwd_data", meta, lambda: lib.wsu_conv3x3_bwd_data(
        g.data_ptr(), w_packed_dgrad.data_ptr(), w_oihw.data_ptr(), ws.data_ptr(), ws.numel() * 4, dx1.data_ptr(), _ptr(dx2), csplit,
        _ptr(mask1), _ptr(mask2), n, h, w, cin, cout, mode, _stream())), "wsu_conv3x3_bwd_data")
    return dx1, dx2


def conv3x3_bwd_weight(g: torch.Tensor, x1: torch.Tensor, x2: Optional[torch.Tensor], want_bias: bool = True, mode: int = 0):
    lib = _lib.load()
    _dev_check(g, x1, x2)
    n, h, w, cout = g.shape
    c1 = x1.shape[3]
    c2 = 0 if x2 is None else x2.shape[3]
    dw = torch.empty((cout, c1 + c2, 3, 3), dtype=torch.float32, device=g.device)
    db = torch.empty(cout, dtype=torch.float32, device=g.device) if want_bias else None
    nbytes = max(lib.wsu_wgrad_workspace_bytes(cout, c1 + c2, 9), (n * h * w + 4095) // 4096 * cout * 4)
    ws = workspace(nbytes, g.device)
    meta = {"flops": 2.0 * 9 * (c1 + c2) * cout * n * h * w}
    check(_launch("conv3x3_bwd_weight", meta, lambda: lib.wsu_conv3x3_bwd_weight(
        g.data_ptr(), x1.data_ptr(), _ptr(x2), dw.data_ptr(), _ptr(db), ws.data_ptr(), ws.numel() * 4,
        n, h, w, c1, c2, cout, mode, _stream())), "wsu_conv3x3_bwd_weight")
    return dw, db


def conv3x3_first_bwd_weight(g: torch.Tensor, x_nchw: torch.Tensor, want_bias: bool = True):
    lib = _lib.load()
    _dev_check(g, x_nchw)
    n, h, w, cout = g.shape
    cin = x_nchw.shape[1]
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=g.device)
    db = torch.empty(cout, dtype=torch.float32, device=g.device) if want_bias else None
    ws = workspace(lib.wsu_first_bwd_workspace_bytes(n, h, w, cin, cout), g.device)
    check(_launch("conv3x3_first_bwd_weight", {}, lambda: lib.wsu_conv3x3_first_bwd_weight(
        g.data_ptr(), x_nchw.data_ptr(), dw.data_ptr(), _ptr(db), ws.data_ptr(), ws.numel() * 4, n, h, w, cin, cout, _stream())),
        "wsu_conv3x3_first_bwd_weight")
    return dw, db


def conv3x3_first_bwd_data(g: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """g: (N,H,W,cout) pre-activation gradient of the first layer -> dx (N,cin,H,W)."""
    lib = _lib.load()
    w = w.detach()
    _dev_check(g, w)
    n, h, wd, cout = g.shape
    cin = w.shape[1]
    dx = torch.empty((n, cin, h, wd), dtype=torch.float32, device=g.device)
    check(lib.wsu_conv3x3_first_bwd_data(g.data_ptr(), w.data_ptr(), dx.data_ptr(), n, h, wd, cin, cout, _stream()),
          "wsu_conv3x3_first_bwd_data")
    return dx


def convt2x2_bwd_weight(x: torch.Tensor, dy: torch.Tensor, want_bias: bool = True, mode: int = 0):
    lib = _lib.load()
    _dev_check(x, dy)
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    assert dy.shape == (n, 2 * h, 2 * w, cout)
    dw = torch.empty((cin, cout, 2, 2), dtype=torch.float32, device=x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if want_bias else None
    nbytes = max(lib.wsu_wgrad_workspace_bytes(cin, cout, 4), (n * h * w * 4 + 4095) // 4096 * cout * 4)
    ws = workspace(nbytes, x.device)
    meta = {"flops": 2.0 * 4 * cin * cout * n * h * w}
    check(_launch("convt2x2_bwd_weight", meta, lambda: lib.wsu_convt2x2_bwd_weight(
        x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _ptr(db), ws.data_ptr(), ws.numel() * 4, n, h, w, cin, cout, mode, _stream())),
        "wsu_convt2x2_bwd_weight")
    return dw, db


def convt2x2_bwd_data(dy: torch.Tensor, w_packed_dgrad: torch.Tensor, cin: int, mask: Optional[torch.Tensor], mode: int) -> torch.Tensor:
    lib = _lib.load()
    _dev_check(dy, w_packed_dgrad, mask)
    n, oh, ow, cout = dy.shape
    h, w = oh // 2, ow // 2
    dx = torch.empty((n, h, w, cin), dtype=torch.float32, device=dy.device)
    meta = {"flops": 2.0 * 4 * cin * cout * n * h * w}
    check(_launch("convt2x2_bwd_data", meta, lambda: lib.wsu_convt2x2_bwd_data(
        dy.data_ptr(), w_packed_dgrad.data_ptr(), dx.data_ptr(), _ptr(mask), n, h, w, cin, cout, mode, _stream())),
        "wsu_convt2x2_bwd_data")
    return dx


def maxpool2x2_bwd(g_full: Optional[torch.Tensor], dy_pool: torch.Tensor, idx: torch.Tensor, xp_mask: Optional[torch.Tensor]) -> torch.Tensor:
    """Adds the routed pooled gradient into ``g_full`` (allocated zero-initialised when None)."""
    lib = _lib.load()
    _dev_check(g_full, dy_pool, idx, xp_mask)
    n, hp, wp, c = dy_pool.shape
    accumulate = g_full is not None
    if g_full is None:
        g_full = torch.empty((n, 2 * hp, 2 * wp, c), dtype=torch.float32, device=dy_pool.device)
    h, w = g_full.shape[1:3]
    check(_launch("maxpool2x2_bwd", {}, lambda: lib.wsu_maxpool2x2_bwd(
        g_full.data_ptr(), dy_pool.data_ptr(), idx.data_ptr(), _ptr(xp_mask), n, h, w, c, int(accumulate), _stream())),
        "wsu_maxpool2x2_bwd")
    return g_full


def conv1x1_sigmoid_bwd(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, relu_mask: bool = True):
    """x: (N,H,W,C) saved input of the head; out/dout: (N,cout,H,W).  Returns gx (N,H,W,C), dw (cout,C,1,1), db (cout)."""
    lib = _lib.load()
    w2 = w.detach().reshape(w.shape[0], -1)
    _dev_check(x, w2, out, dout)
    n, h, wd, c = x.shape
    cout = w2.shape[0]
    gx = torch.empty_like(x)
    dw = torch.empty((cout, c, 1, 1), dtype=torch.float32, device=x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device)
    ws = workspace(lib.wsu_head_bwd_workspace_bytes(c, cout), x.device)
    check(_launch("conv1x1_sigmoid_bwd", {}, lambda: lib.wsu_conv1x1_sigmoid_bwd(
        x.data_ptr(), w2.data_ptr(), out.data_ptr(), dout.data_ptr(), gx.data_ptr(), dw.data_ptr(), db.data_ptr(),
        ws.data_ptr(), ws.numel() * 4, n, h, wd, c, cout, int(relu_mask), _stream())), "wsu_conv1x1_sigmoid_bwd")
    return gx, dw, db


def l1ws_loss_fwd_bwd(out: torch.Tensor, covers: torch.Tensor, inputs: torch.Tensor, alphas: torch.Tensor,
                      use_l1: int = 1, use_ws: bool = True):
    """Returns (loss scalar tensor, dLoss/dout, parts[l1, ws], beta_hat[N])."""
    lib = _lib.load()
    _dev_check(out, covers, inputs, alphas)
    assert out.shape == covers.shape == inputs.shape and out.dtype == torch.float32
    n = out.shape[0]
    per = out.numel() // n
    loss = torch.empty((), dtype=torch.float32, device=out.device)
    parts = torch.empty(2, dtype=torch.float32, device=out.device)
    beta = torch.empty(n, dtype=torch.float32, device=out.device)
    dout = torch.empty_like(out)
    ws = torch.empty((lib.wsu_l1ws_loss_workspace_bytes(n) + 7) // 8, dtype=torch.float64, device=out.device)
    alphas = alphas.to(torch.float32).contiguous()
    check(lib.wsu_l1ws_loss_fwd_bwd(out.data_ptr(), covers.data_ptr(), inputs.data_ptr(), alphas.data_ptr(), loss.data_ptr(),
                                    parts.data_ptr(), dout.data_ptr(), beta.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                    n, per, int(use_l1), int(use_ws), _stream()), "wsu_l1ws_loss_fwd_bwd")
    return loss, dout, parts, beta


class AdamWTable:
    """Device-side descriptor table for wsu_adamw_multi_tensor over a fixed list of (param, grad, m, v)."""

    def __init__(self, params, grads, exp_avg, exp_avg_sq):
        import numpy as np
        rows, first = [], 0
        for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq):
            _dev_check(p, g, m, v)
            assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float32 and p.numel() == g.numel()
            rows.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), first])
            first += (p.numel() + 1023) // 1024
        self.total_blocks = first
        self.ntensors = len(rows)
        self.table = torch.from_numpy(np.array(rows, dtype=np.int64)).to(params[0].device)
        self.ptrs = [r[:4] for r in rows]

    def matches(self, params, grads):
        return all(p.data_ptr() == r[0] and g.data_ptr() == r[1] for p, g, r in zip(params, grads, self.ptrs))

    def step(self, step: int, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0,
             skip_flag: Optional[torch.Tensor] = None):
        lib = _lib.load()
        check(lib.wsu_adamw_multi_tensor(self.table.data_ptr(), self.ntensors, self.total_blocks, lr, betas[0], betas[1],
                                         eps, weight_decay, step, grad_scale, _ptr(skip_flag), _stream()), "wsu_adamw_multi_tensor")


def pow2_grad_scale(x: torch.Tensor) -> torch.Tensor:
    """Device-side {scale, 1/scale} with scale = 2^floor(2 - log2 max|x|) (wsu_pow2_grad_scale): no host sync, no ATen arithmetic."""
    lib = _lib.load()
    _dev_check(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    ws = workspace(16, x.device)
    check(lib.wsu_pow2_grad_scale(x.data_ptr(), x.numel(), out.data_ptr(), ws.data_ptr(), _stream()), "wsu_pow2_grad_scale")
    return out


def scale_by(x: torch.Tensor, factor: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x * factor[0] with the factor on the device (wsu_scale_f32); ``out`` may be ``x`` itself."""
    lib = _lib.load()
    _dev_check(x, factor)
    assert x.dtype == torch.float32 and x.is_contiguous() and factor.dtype == torch.float32
    y = torch.empty_like(x) if out is None else out
    check(lib.wsu_scale_f32(x.data_ptr(), y.data_ptr(), x.numel(), factor.data_ptr(), _stream()), "wsu_scale_f32")
    return y


def scale_many_(tensors, factor: torch.Tensor) -> None:
    """In-place multiplication of every tensor by factor[0] in ONE launch (wsu_scale_multi_tensor)."""
    import numpy as np
    lib = _lib.load()
    tensors = [t for t in tensors if t is not None]
    if not tensors:
        return
    rows, first = [], 0
    for t in tensors:
        _dev_check(t)
        assert t.dtype == torch.float32 and t.is_contiguous()
        rows.append([t.data_ptr(), t.numel(), first])
        first += (t.numel() + 1023) // 1024
    table = torch.from_numpy(np.array(rows, dtype=np.int64)).to(tensors[0].device, non_blocking=True)
    check(lib.wsu_scale_multi_tensor(table.data_ptr(), len(rows), first, factor.data_ptr(), _stream()), "wsu_scale_multi_tensor")


def nonfinite_flag(g: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """flag[0] = 1 if ``g`` holds an inf / NaN else 0, flag[1] += flag[0] (int32[2] on the device; wsu_nonfinite_flag)."""
    lib = _lib.load()
    _dev_check(g, flag)
    assert g.dtype == torch.float32 and g.is_contiguous() and flag.dtype == torch.int32 and flag.numel() >= 2
    check(lib.wsu_nonfinite_flag(g.data_ptr(), g.numel(), flag.data_ptr(), _stream()), "wsu_nonfinite_flag")
    return flag
