"""The three-term arithmetic of the planar training kernels with products 'f16f8', restated on the CPU in float64 from include/wsu.h and
ws_unet_amd/csrc/wsu_device.h.  Nothing here calls the library.

A stored planar value is  f16 part + residual  (plane 2: e4m3(residual * lo_scale), lo_scale = 2^12 for activations, 2^14 for gradients).
The matrix kernels multiply two operands u, v as

    hi_u * hi_v  +  copy_u * res_v  +  res_u * copy_v          (res_u * res_v is not computed)

where `copy` is an e4m3 copy of the value.  For planar operands the consumer's loader lanes derive it from the STORED f16 part:
activations e4m3(hi / 4) * 4 with hi clamped to +-1792 (wsu_f16x8_to_fp8), gradients e4m3(hi * 4) / 4 with hi clamped to +-112
(wsu_f16x8_to_fp8_grad).  Weights are packed from fp32 by the library (every f16f8 packer goes through wsu_split4_f16f8 with the same two
divisors): f16(w), e4m3((w - f16 w) * 2^18) / 2^18 and e4m3(w * 2^6) / 2^6, residual and copy clamped to the e4m3 range first.

`op` below is always an exact float64 bilinear operation op(u, v) (the F.conv2d adjoints); outputs written as planar tensors are compared
after the store encoding (encode / decode: f16 round to nearest even, residual clamped and rounded to e4m3).
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

X_LO = 4096.0                  # residual scaling of activations (WSU_F8_XLO_DIV)
G_LO = 16384.0                 # ... of gradients (WSU_F8_GLO_DIV)
W_LO = 2.0 ** 18               # ... of packed weights (WSU_F8_WLO_DIV)
W_COPY = 2.0 ** 6              # weights' e4m3 copy is e4m3(w * 2^6) (WSU_F8_W_DIV)

Parts = namedtuple("Parts", "hi res copy")          # float64, NCHW (weights: their own shape)


def e4m3(v: torch.Tensor) -> torch.Tensor:
    """nearest e4m3 value (round to nearest even, subnormals down to 2^-9, saturating at +-448) of values that are exact in fp32"""
    assert torch.equal(v.double(), v.float().double()), "e4m3: the argument must be exact in fp32 (one rounding only)"
    return v.clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn).double()


def _bytes(planes: torch.Tensor) -> torch.Tensor:
    raw = planes.detach().cpu().contiguous().view(torch.uint8)                              # (n, chunk, 3, h, w, 16)
    assert raw.dim() == 6 and raw.shape[2] == 3 and raw.shape[5] == 16, raw.shape
    return raw


def _nchw(t: torch.Tensor) -> torch.Tensor:
    n, nch, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, nch * 16, h, w).contiguous()


def _chunked(t: torch.Tensor) -> torch.Tensor:
    n, c, h, w = t.shape
    return t.reshape(n, c // 16, 16, h, w).permute(0, 1, 3, 4, 2).contiguous()            # (n, chunk, h, w, 16)


def copy_of(hi: torch.Tensor, lo_scale: float) -> torch.Tensor:
    """the e4m3 copy the kernels derive from a stored f16 part"""
    if lo_scale == X_LO:
        return e4m3(hi.clamp(-1792.0, 1792.0) / 4.0) * 4.0
    assert lo_scale == G_LO
    return e4m3(hi.clamp(-112.0, 112.0) * 4.0) / 4.0


def parts(planes: torch.Tensor, lo_scale: float) -> Parts:
    """planar storage (the bytes, any device) -> what the kernels multiply"""
    raw = _bytes(planes)
    n, nch, _, h, w, _ = raw.shape
    hi = torch.stack([raw[:, :, 0], raw[:, :, 1]], dim=-2).contiguous().view(torch.float16).reshape(n, nch, h, w, 16).double()
    res = raw[:, :, 2].contiguous().view(torch.float8_e4m3fn).double() / lo_scale
    hi, res = _nchw(hi), _nchw(res)
    return Parts(hi, res, copy_of(hi, lo_scale))


def make_planes(hi: torch.Tensor, res_codes: torch.Tensor) -> torch.Tensor:
    """planar bytes from f16 parts and residual CODE VALUES (the e4m3 number stored in plane 2, i.e. residual * lo_scale), both NCHW and
    both exactly representable -- crafted operands, not encodings of real numbers"""
    h16, r8 = hi.to(torch.float16), res_codes.float().to(torch.float8_e4m3fn)
    assert torch.equal(h16.double(), hi.double()) and torch.equal(r8.double(), res_codes.double())
    hc, rc = _chunked(h16), _chunked(r8)
    n, nch, h, w, _ = hc.shape
    hb = hc.view(torch.uint8).reshape(n, nch, h, w, 2, 16)
    return torch.stack([hb[..., 0, :], hb[..., 1, :], rc.view(torch.uint8)], dim=2).contiguous()


def encode(x: torch.Tensor, lo_scale: float) -> torch.Tensor:
    """the store encoding (wsu_split4_f16r8): fp32 NCHW -> planar bytes on the CPU; gpu_util.planar_encode gives the same bytes"""
    xc = _chunked(x.float())
    hi = xc.to(torch.float16)
    lo = ((xc - hi.float()) * lo_scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    n, nch, h, w, _ = xc.shape
    hb = hi.view(torch.uint8).reshape(n, nch, h, w, 2, 16)
    return torch.stack([hb[..., 0, :], hb[..., 1, :], lo.view(torch.uint8)], dim=2).contiguous()


def decode(planes: torch.Tensor, lo_scale: float) -> torch.Tensor:
    """planar bytes -> float64 NCHW: f16 part + residual"""
    p = parts(planes, lo_scale)
    return p.hi + p.res


def store(v: torch.Tensor, lo_scale: float) -> torch.Tensor:
    """what a planar tensor holds for the fp32 value v"""
    return decode(encode(v, lo_scale), lo_scale)


def as_device_planar(planes: torch.Tensor, device) -> torch.Tensor:
    """bytes -> the float32-typed tensor the ops take"""
    return planes.contiguous().to(device).view(torch.float32)


def weight_parts(w: torch.Tensor) -> Parts:
    """fp32 weights -> the three parts every f16f8 packer writes (wsu_split4_f16f8 with WSU_F8_WLO_DIV, WSU_F8_W_DIV)"""
    w = w.float()
    hi = w.to(torch.float16).float()
    res = e4m3((w - hi) * W_LO) / W_LO                 # w - f16 w is exact in fp32; the clamp at 448 * 2^-18 is e4m3()'s
    copy = e4m3(w * W_COPY) / W_COPY                   # from the fp32 value, clamped at +-7
    return Parts(hi.double(), res, copy)


# ---- the exact bilinear operations ---------------------------------------------------------------------------------------------------------
def conv_wgrad(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """dW[co, ci, u, v] = sum g[n, co, y, x] * reflectpad(x)[n, ci, y + u, x + v]"""
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect")
    return F.conv2d(xp.transpose(0, 1), g.transpose(0, 1)).transpose(0, 1).contiguous()


def convt_wgrad(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dW[ci, co, a, b] = sum x[n, ci, i, j] * dy[n, co, 2i + a, 2j + b]"""
    return torch.stack([torch.stack([torch.einsum("nihw,nohw->io", x, dy[:, :, a::2, b::2]) for b in range(2)], dim=-1) for a in range(2)], dim=-2)


def conv_dgrad(pad_zero: bool):
    """adjoint of conv2d(pad(x), w) in x, applied to g: op(g, w), w (cout, cin, 3, 3)"""
    def op(g, w):
        x = torch.zeros((g.shape[0], w.shape[1], g.shape[2], g.shape[3]), dtype=torch.float64, requires_grad=True)
        F.conv2d(F.pad(x, (1, 1, 1, 1), mode="constant" if pad_zero else "reflect"), w).backward(g)
        return x.grad.detach()
    return op


def reflect_pieces(g: torch.Tensor, w: torch.Tensor):
    """The reflect adjoint as the kernels stage it (wsu_conv3x3_pl_bwd_data): the zero-padding adjoint Z (n, cin, h, w) and what the four padded
    border lines receive -- top / bottom (n, cin, w + 2), corners included; left / right (n, cin, h) -- each bilinear in (g, w)."""
    n, _, h, wd = g.shape
    cin = w.shape[1]
    mk = lambda *s: torch.zeros(s, dtype=torch.float64, requires_grad=True)
    x, pt, pb, pl, pr = mk(n, cin, h, wd), mk(n, cin, 1, wd + 2), mk(n, cin, 1, wd + 2), mk(n, cin, h, 1), mk(n, cin, h, 1)
    F.conv2d(torch.cat([pt, torch.cat([pl, x, pr], dim=3), pb], dim=2), w).backward(g)
    return x.grad, pt.grad[:, :, 0], pb.grad[:, :, 0], pl.grad[..., 0], pr.grad[..., 0]


def fold_order(h: int, w: int):
    """(strip, strip index, target row, target column) in the order ring_fold_pl_kernel adds them: top (centre, left corner, right corner),
    bottom (same), left, right; slices are whole lines"""
    a = slice(None)
    return [(1, slice(1, w + 1), 1, a), (1, 0, 1, 1), (1, w + 1, 1, w - 2), (2, slice(1, w + 1), h - 2, a), (2, 0, h - 2, 1), (2, w + 1, h - 2, w - 2),
            (3, a, a, 1), (4, a, a, w - 2)]


def reflect_staged(u: Parts, v: Parts, products: str = "f16f8", mask=None) -> torch.Tensor:
    """What wsu_conv3x3_pl_bwd_data stores under reflect padding: the masked zero-padding adjoint, stored; the four strips' 1x3 convolutions,
    stored WITH their residual plane for either `products`; on the border ring (rows 1, h-2, columns 1, w-2) the decoded strips summed in
    fp32 in the fold's fixed order, added to the decoded main value where the mask is set, and stored again.  'f16': first term only and a
    gradient tensor is an f16 tensor (no residual plane).  Returns the fp32 values that go into the LAST store encoding of every pixel (off
    the ring the adjoint itself): the bytes are encode() of it."""
    pieces = list(reflect_pieces(u.hi, v.hi))
    if products == "f16f8":
        for a, b in ((u.copy, v.res), (u.res, v.copy)):
            pieces = [p + q for p, q in zip(pieces, reflect_pieces(a, b))]
    keep = (lambda t: store(t, G_LO)) if products == "f16f8" else (lambda t: t.float().half().double())
    z = pieces[0] if mask is None else pieces[0] * mask
    main = keep(z).float()
    n, c, h, w = main.shape
    strips = [None] + [store(p.reshape(n, c, 1, -1), G_LO).reshape(p.shape).float() for p in pieces[1:]]
    add = torch.zeros_like(main)
    for s, si, ty, tx in fold_order(h, w):
        add[:, :, ty, tx] = add[:, :, ty, tx] + strips[s][:, :, si]                                # fp32, one addition at a time
    if mask is not None:
        add = add * mask
    ring = ~off_ring(h, w)
    return torch.where(ring, main + add, z.float()).double()                                    # fp32; the caller applies the (last) store encoding


def convt_dgrad(dy: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """dx[n, ci, i, j] = sum dy[n, co, 2i + a, 2j + b] * w[ci, co, a, b]"""
    return F.conv2d(dy, w, stride=2)


def conv_fwd(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w)


def convt_fwd(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return F.conv_transpose2d(x, w, stride=2)


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------------
def f16_only(op, u: Parts, v: Parts) -> torch.Tensor:
    return op(u.hi, v.hi)


def cross_terms(op, u: Parts, v: Parts):
    return op(u.copy, v.res), op(u.res, v.copy)


def three_term(op, u: Parts, v: Parts) -> torch.Tensor:
    a, b = cross_terms(op, u, v)
    return op(u.hi, v.hi) + a + b


def abs_sum(op, u: Parts, v: Parts) -> torch.Tensor:
    """sum of |term| per output entry (op has non-negative coefficients)"""
    return op(u.hi.abs(), v.hi.abs()) + op(u.copy.abs(), v.res.abs()) + op(u.res.abs(), v.copy.abs())


def in_window(op, u: Parts, v: Parts, q: float, extra: float = 0.0) -> bool:
    """The exactness window of family A: every product is a multiple of the quantum q (checked on the operands' parts: then every term is)
    and sum |terms| (+ extra, e.g. |bias|) < 2^24 q for every output entry -- any summation order and any rounding mode of the matrix unit
    then give the same fp32 value."""
    prods = [(u.hi, v.hi), (u.copy, v.res), (u.res, v.copy)]
    for a, b in prods:
        pa, pb = a.abs()[a != 0], b.abs()[b != 0]
        if pa.numel() and pb.numel():
            for x in pa.unique():
                t = x * pb.unique() / q
                if not torch.equal(t, t.round()):
                    return False
    return float(abs_sum(op, u, v).max()) + extra < 2.0 ** 24 * q


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


# ---- the comparisons the GPU tests use (tests/test_f16f8_terms_host.py feeds them wrong results) ---------------------------------------------
def exact_equal(got: torch.Tensor, want: torch.Tensor) -> bool:
    """family A, fp32 outputs: bit for bit (as values: -0 == +0)"""
    return got.shape == want.shape and bool(torch.equal(got.detach().cpu().double(), want.double()))


def planar_equal(got_planes: torch.Tensor, want: torch.Tensor, lo_scale: float, where=None, residual: bool = True) -> bool:
    """family A, planar outputs: the f16 planes and the residual plane hold the store encoding of the exact value `want` (where: only at
    these (h, w) pixels; residual=False: a gradient written with products 'f16' has no residual plane)"""
    g, e = parts(got_planes, lo_scale), parts(encode(want, lo_scale), lo_scale)
    if g.hi.shape != e.hi.shape:
        return False
    sel = torch.ones(g.hi.shape[2:], dtype=torch.bool) if where is None else where
    return bool(torch.equal(g.hi[..., sel], e.hi[..., sel])) and (not residual or bool(torch.equal(g.res[..., sel], e.res[..., sel])))


def off_ring(h: int, w: int) -> torch.Tensor:
    """(h, w) pixels that the reflect adjoint's border fold does not touch (rows 1, h-2 and columns 1, w-2 are re-encoded after the fold)"""
    m = torch.ones((h, w), dtype=torch.bool)
    m[[1, h - 2], :] = False
    m[:, [1, w - 2]] = False
    return m


RATIO_BOUND = 0.25             # family B: a kernel without cross terms sits at 1.0, one term missing at ~0.7, one term off by 2 at ~0.35 .. 0.7
E1_MIN = 1e-4                  # ... and the operands must really carry residuals


def ratio(got: torch.Tensor, want: torch.Tensor, e1: float) -> float:
    return rel_l2(got, want) / e1


def ratio_ok(got: torch.Tensor, want: torch.Tensor, e1: float) -> bool:
    return e1 >= E1_MIN and ratio(got, want, e1) <= RATIO_BOUND


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def hashed(shape, seed: int, table) -> torch.Tensor:
    """table[hash(seed, index)]: a value per element that depends on every index through an integer hash (no period in 8, 16, 32, 64)"""
    idx = np.indices(shape).astype(np.uint64)
    ks = [0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x27D4EB2F165667C5, 0x85EBCA77C2B2AE63]
    with np.errstate(over="ignore"):
        h = np.full(shape, (seed + 1) * 0xD6E8FEB86659FD93 % 2 ** 64, dtype=np.uint64)
        for d in range(len(shape)):
            h = (h ^ (idx[d] + np.uint64(1)) * np.uint64(ks[d])) * np.uint64(0xFF51AFD7ED558CCD)
            h ^= h >> np.uint64(33)
        h = h * np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(29)
    t = np.asarray(table, dtype=np.float64)
    return torch.from_numpy(t[(h % np.uint64(len(t))).astype(np.int64)])


ACT_A = [0, 4, 0, 4, 0, 0, 4]                          # f16 parts whose e4m3 copies are exact, about half zero
ACT_A3 = [0, 4, 0, 8, 0, 4, 0]
GRAD_A = [0, 0.25, 0, -0.25, 0, 0, 0.25, -0.25, 0]
RES_A = [0, 1, 0, -1, 0, 2, 0, -2, 0, 0, 1]            # residual code values (times 1 / lo_scale)


def crafted(shape, seed: int, hi_table, res_table=RES_A, zero_hi: bool = False, zero_res: bool = False):
    """family A planar operand: (bytes, Parts-relevant lo_scale is the caller's)"""
    hi = torch.zeros(shape, dtype=torch.float64) if zero_hi else hashed(shape, seed, hi_table)
    res = torch.zeros(shape, dtype=torch.float64) if zero_res else hashed(shape, seed + 1000, res_table)
    return make_planes(hi, res)


def crafted_weights(shape, seed: int, hi_table, zero_res: bool = False) -> torch.Tensor:
    """fp32 weights  hi + k 2^-18  (k from RES_A, 0 where hi is 0: a value below the f16 grid has no residual) that the packers decompose into
    exactly these parts; the caller asserts it with weight_parts."""
    hi = hashed(shape, seed, hi_table)
    k = torch.zeros(shape, dtype=torch.float64) if zero_res else hashed(shape, seed + 1000, RES_A)
    return (hi + torch.where(hi != 0, k, torch.zeros_like(k)) / W_LO).float()


def rand_act(shape, seed: int) -> torch.Tensor:
    """family B: relu(randn) times per-channel powers of two 2^-3 .. 2^3"""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(shape, generator=g))
    e = torch.randint(-3, 4, (shape[1],), generator=g).float()
    return x * torch.exp2(e)[None, :, None, None]


def rand_grad(shape, seed: int) -> torch.Tensor:
    """family B: randn scaled by a power of two so that the largest magnitude lies in (2, 4]"""
    g = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    m = float(g.abs().max())
    return g * 2.0 ** (2 - int(np.ceil(np.log2(m))))


def rand_weight(shape, seed: int, fan_in: int) -> torch.Tensor:
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * (2.0 / fan_in) ** 0.5
