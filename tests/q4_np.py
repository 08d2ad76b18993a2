"""The arithmetic and the storage formats of the default inference mode 'f16f4p' (and of its one-product sibling 'f16p'), restated on the CPU in
float64 from include/wsu.h (K1q, K1u, K1h, K0p) and ws_unet_amd/csrc/wsu_device.h.  Nothing here calls the library or tests/gpu_util.py.

A planar Q tensor holds, per image and 16-channel chunk, the planes  f16 ch 0-7 | f16 ch 8-15 | Q  as [H][W][16 B] and then one scale byte
E + 127 per pixel in 16 x 32-pixel tile blocks [ceil(H/16)][ceil(W/32)][16][32].  Q = 32 fp4 (e2m1) nibbles per pixel, low nibble first:
nibble i = copy of channel i over 2^E, nibble 16 + i = residual of channel i times 2^11 over 2^E.  What a consumer multiplies is what is
STORED, so `q_parts` reads bytes:

    hi = the f16 planes,   copy = nibble(0-15) * 2^E,   res = nibble(16-31) * 2^(E - 11),   E = scale byte - 127

and a product w * x is   hi_w * hi_x  +  res_w * copy_x  +  copy_w * res_x      (res_w * res_x is not computed).

Weights are packed from fp32 per block of 16 input channels of one (output channel, tap): f16(w), then with 2^E the smallest power of two
that does not saturate fp4 on the block's largest |f16 part| (block_exp),  res_w = fp4((w - f16 w) * 2^11 / 2^E) * 2^(E - 11)  and
copy_w = fp4(f16 w / 2^E) * 2^E.  The fused decoder entry (K1u) first combines its transposed conv into parity-class 2 x 2-tap weights Wc in
fp32 (combined_weights) and splits those the same way per (co, class, dy, dx, 16 c); the H packers round to f16 once.

A producer writes a Q tensor from its fp32 values (q_encode): f16 round to nearest even, E from the chunk's 16 f16 parts, both nibble sets
rounded to nearest even, saturating, the residual nibble from the EXACT residual.  Formats A (e4m3 residual * 2^12, a_encode) and H (the
two f16 planes, h_encode) are the other two store encodings of the same kernels.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

Parts = namedtuple("Parts", "hi res copy")            # float64, NCHW (weights: their own shape)
QT = namedtuple("QT", "data n c h w")                 # planar Q / H bytes: uint8 (n, c / 16, chunk bytes)

FP4 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)        # e2m1 magnitudes by code; bit 3 of a nibble is the sign
A_LO = 4096.0                                         # format A: plane 2 = e4m3((x - f16 x) * 2^12)


# ---- fp4 and the block scale ---------------------------------------------------------------------------------------------------------------
def fp4_codes(v: torch.Tensor, truncate: bool = False) -> torch.Tensor:
    """float64 -> e2m1 nibbles: round to nearest, ties to the even code (even mantissa), saturating at 6; the sign bit follows the value's.
    truncate=True rounds toward zero instead (a wrong producer, for tests/test_q4_terms_host.py)."""
    a = v.double().abs()
    idx = torch.zeros(a.shape, dtype=torch.long)
    for i in range(7):
        if truncate:
            up = a >= FP4[i + 1]
        else:
            mid = (FP4[i] + FP4[i + 1]) / 2
            up = (a > mid) | ((a == mid) & (i % 2 == 1))
        idx = torch.where(up & (idx == i), torch.full_like(idx, i + 1), idx)
    return (idx | (torch.signbit(v.double()).long() << 3)).to(torch.uint8)


def fp4_values(codes: torch.Tensor) -> torch.Tensor:
    mag = torch.tensor(FP4, dtype=torch.float64)[(codes & 7).long()]
    return torch.where((codes & 8) != 0, -mag, mag)


def f16_round(v: torch.Tensor) -> torch.Tensor:
    """nearest f16 (ties to even) of values exact in fp32, as float64"""
    assert torch.equal(v.double(), v.float().double()), "one rounding only: the argument must be exact in fp32"
    return v.float().to(torch.float16).double()


def block_exp(amax: torch.Tensor) -> torch.Tensor:
    """E of a block whose largest |f16 part| is amax (wsu_q4_block_exp, on the f16 bit pattern): exponent field - 16, and one less when the
    mantissa is <= 1.5 (the largest element then lands in [4, 6] instead of [2, 3))"""
    b = amax.to(torch.float16).contiguous().view(torch.int16).long() & 0x7FFF
    ef, man = b >> 10, b & 0x3FF
    return ef - 16 - ((ef > 0) & (man <= 0x200)).long()


def _chunked(t: torch.Tensor) -> torch.Tensor:
    n, c, h, w = t.shape
    return t.reshape(n, c // 16, 16, h, w).permute(0, 1, 3, 4, 2).contiguous()             # (n, chunk, h, w, 16)


def _nchw(t: torch.Tensor) -> torch.Tensor:
    n, nch, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, nch * 16, h, w).contiguous()


# ---- planar Q bytes ------------------------------------------------------------------------------------------------------------------------
def q_chunk_bytes(h: int, w: int) -> int:
    return 48 * h * w + 512 * ((h + 15) // 16) * ((w + 31) // 32)


def scale_index(h: int, w: int) -> torch.Tensor:
    """(h, w) -> offset of a pixel's scale byte inside a chunk's scale plane"""
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return ((yy // 16) * ((w + 31) // 32) + xx // 32) * 512 + (yy % 16) * 32 + xx % 32


def make_q(hi: torch.Tensor, copy_codes: torch.Tensor, res_codes: torch.Tensor, e: torch.Tensor, fill: int = 0) -> QT:
    """planar Q bytes from f16 parts (NCHW, exact in f16), nibbles (NCHW uint8) and E (n, chunk, h, w): crafted operands are made of
    bytes, they need not be the encoding of any real number.  The scale plane's padding slots hold `fill`."""
    n, c, h, w = hi.shape
    h16 = hi.to(torch.float16)
    assert torch.equal(h16.double(), hi.double())
    hb = _chunked(h16).view(torch.uint8).reshape(n, c // 16, h, w, 2, 16)
    cc, rc = _chunked(copy_codes), _chunked(res_codes)
    nib = torch.cat([cc, rc], dim=-1)                                                      # 32 nibbles per (pixel, chunk)
    qb = (nib[..., 0::2] | (nib[..., 1::2] << 4)).to(torch.uint8)
    hw = h * w
    data = torch.full((n, c // 16, q_chunk_bytes(h, w)), fill, dtype=torch.uint8)
    data[:, :, 0:16 * hw] = hb[..., 0, :].reshape(n, c // 16, -1)
    data[:, :, 16 * hw:32 * hw] = hb[..., 1, :].reshape(n, c // 16, -1)
    data[:, :, 32 * hw:48 * hw] = qb.reshape(n, c // 16, -1)
    data[:, :, 48 * hw + scale_index(h, w).reshape(-1)] = (e + 127).to(torch.uint8).reshape(n, c // 16, -1)
    return QT(data, n, c, h, w)


def q_fields(t: QT, neighbour_scale: bool = False):
    """the bytes of a planar Q tensor -> (f16 parts, copy nibble values, residual nibble values: NCHW float64; E: (n, chunk, h, w) long).
    neighbour_scale=True takes every pixel's scale byte from its right-hand neighbour (a wrong consumer, for the host tests)."""
    n, c, h, w = t.n, t.c, t.h, t.w
    nch, hw = c // 16, h * w
    raw = t.data.detach().cpu()
    assert raw.shape == (n, nch, q_chunk_bytes(h, w)), (raw.shape, (n, c, h, w))
    planes = torch.stack([raw[:, :, 0:16 * hw].reshape(n, nch, h, w, 16), raw[:, :, 16 * hw:32 * hw].reshape(n, nch, h, w, 16)], dim=-2)
    hi = planes.contiguous().view(torch.float16).reshape(n, nch, h, w, 16).double()
    qb = raw[:, :, 32 * hw:48 * hw].reshape(n, nch, h, w, 16)
    nib = torch.stack([qb & 15, qb >> 4], dim=-1).reshape(n, nch, h, w, 32)
    e = raw[:, :, 48 * hw + scale_index(h, w).reshape(-1)].reshape(n, nch, h, w).long() - 127
    if neighbour_scale:
        e = e[..., torch.arange(w).add(1).clamp_max(w - 1)]
    return _nchw(hi), _nchw(fp4_values(nib[..., :16])), _nchw(fp4_values(nib[..., 16:])), e


def _per_channel(e: torch.Tensor) -> torch.Tensor:
    return e.repeat_interleave(16, dim=1)                                                  # (n, chunk, h, w) -> (n, c, h, w)


def q_parts(t: QT, neighbour_scale: bool = False) -> Parts:
    """what a consumer of the planar Q tensor multiplies"""
    hi, cv, rv, e = q_fields(t, neighbour_scale)
    sc = torch.exp2(_per_channel(e).double())
    return Parts(hi, rv * sc / 2048.0, cv * sc)


def q_encode(v: torch.Tensor, truncate_residual: bool = False, fill: int = 0) -> QT:
    """the store encoding of format Q: what a producer writes for the fp32 values v (NCHW)"""
    hi = f16_round(v)
    e = block_exp(_chunked(hi).abs().amax(dim=-1))
    sc = torch.exp2(_per_channel(e).double())
    return make_q(hi, fp4_codes(hi / sc), fp4_codes((v.double() - hi) * 2048.0 / sc, truncate=truncate_residual), e, fill)


def q_decode(t: QT) -> torch.Tensor:
    """planar Q bytes -> float64 NCHW: f16 part + residual"""
    p = q_parts(t)
    return p.hi + p.res


# ---- formats A and H -----------------------------------------------------------------------------------------------------------------------
def a_encode(v: torch.Tensor) -> torch.Tensor:
    """format A: uint8 (n, chunk, 3, h, w, 16) = f16 ch 0-7 | f16 ch 8-15 | e4m3((v - f16 v) * 2^12), the residual clamped to +-448 first"""
    xc = _chunked(v.float())
    hi = xc.to(torch.float16)
    lo = ((xc - hi.float()) * A_LO).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    n, nch, h, w, _ = xc.shape
    hb = hi.view(torch.uint8).reshape(n, nch, h, w, 2, 16)
    return torch.stack([hb[..., 0, :], hb[..., 1, :], lo.view(torch.uint8)], dim=2).contiguous()


def a_fields(planes: torch.Tensor):
    """format A bytes (any dtype view, any device) -> (f16 parts, residuals) float64 NCHW"""
    raw = planes.detach().cpu().contiguous().view(torch.uint8)
    assert raw.dim() == 6 and raw.shape[2] == 3 and raw.shape[5] == 16, raw.shape
    n, nch, _, h, w, _ = raw.shape
    hi = torch.stack([raw[:, :, 0], raw[:, :, 1]], dim=-2).contiguous().view(torch.float16).reshape(n, nch, h, w, 16).double()
    res = raw[:, :, 2].contiguous().view(torch.float8_e4m3fn).double() / A_LO
    return _nchw(hi), _nchw(res)


def a_decode(planes: torch.Tensor) -> torch.Tensor:
    hi, res = a_fields(planes)
    return hi + res


def h_encode(v: torch.Tensor) -> QT:
    """format H: uint8 (n, chunk, 32 h w) = the two f16 planes of a Q chunk"""
    n, c, h, w = v.shape
    hb = _chunked(v.float().to(torch.float16)).view(torch.uint8).reshape(n, c // 16, h, w, 2, 16)
    return QT(torch.cat([hb[..., 0, :].reshape(n, c // 16, -1), hb[..., 1, :].reshape(n, c // 16, -1)], dim=2).contiguous(), n, c, h, w)


def h_decode(t: QT) -> torch.Tensor:
    n, c, h, w = t.n, t.c, t.h, t.w
    raw = t.data.detach().cpu()
    assert raw.shape == (n, c // 16, 32 * h * w), raw.shape
    planes = torch.stack([raw[:, :, :16 * h * w].reshape(n, c // 16, h, w, 16), raw[:, :, 16 * h * w:].reshape(n, c // 16, h, w, 16)], dim=-2)
    return _nchw(planes.contiguous().view(torch.float16).reshape(n, c // 16, h, w, 16).double())


def h_parts(t: QT) -> Parts:
    hi = h_decode(t)
    return Parts(hi, torch.zeros_like(hi), torch.zeros_like(hi))


def cat_parts(a: Parts, b) -> Parts:
    return a if b is None else Parts(*(torch.cat([p, q], dim=1) for p, q in zip(a, b)))


# ---- weights as the packers make them ------------------------------------------------------------------------------------------------------
def weight_parts(w: torch.Tensor) -> Parts:
    """fp32 weights (cout, cin, ...) -> the three parts wsu_conv3x3_pack_f4 writes: one block = 16 consecutive input channels of one
    (output channel, trailing index)"""
    w = w.float()
    hi = w.to(torch.float16).float()
    r = (w - hi).double() * 2048.0                                           # exact in fp32, as in the packer
    co, ci = w.shape[:2]
    blk = lambda t: t.reshape(co, ci // 16, 16, -1)
    e = block_exp(blk(hi).abs().amax(dim=2, keepdim=True))
    sc = torch.exp2(e.double())
    res = fp4_values(fp4_codes(blk(r) / sc)) * sc / 2048.0
    copy = fp4_values(fp4_codes(blk(hi).double() / sc)) * sc
    return Parts(hi.double(), res.reshape(w.shape), copy.reshape(w.shape))


def weight_parts_h(w: torch.Tensor) -> Parts:
    hi = w.float().to(torch.float16).double()
    return Parts(hi, torch.zeros_like(hi), torch.zeros_like(hi))


def combined_weights(w3: torch.Tensor, wt: torch.Tensor, cup: int, swap_px: bool = False) -> torch.Tensor:
    """K1u: Wc[co][c][py][px][dy][dx] = sum_ci sum_{(ky, kx) -> (dy, dx)} w3[co][ci][ky][kx] wt[c][ci][sy][sx] in float64.  Tap ky of output row
    2 i + py lies on row 2 i + py + ky - 1 of the upsampled tensor = low row i - 1 + py + dy at sub-row sy.  swap_px: the column-parity
    classes exchanged (a wrong packer, for the host tests)."""
    cout, cl = w3.shape[0], wt.shape[0]
    wc = torch.zeros((cout, cl, 2, 2, 2, 2), dtype=torch.float64)
    for py in range(2):
        for ky in range(3):
            r = py + ky - 1
            dy, sy = r // 2 + 1 - py, r % 2
            for px in range(2):
                for kx in range(3):
                    q = px + kx - 1
                    dx, sx = q // 2 + 1 - px, q % 2
                    wc[:, :, py, 1 - px if swap_px else px, dy, dx] += torch.einsum("oi,ci->oc", w3[:, :cup, ky, kx].double(), wt[:, :, sy, sx].double())
    return wc


def combined_bias(w3: torch.Tensor, bt, b3, cup: int) -> torch.Tensor:
    """K1u: b3[co] + sum_ci bt[ci] * sum_taps w3[co][ci][tap] (under reflect padding every output pixel has all nine taps)"""
    s = torch.zeros(w3.shape[0], dtype=torch.float64) if b3 is None else b3.double().clone()
    return s if bt is None else s + torch.einsum("oikl,i->o", w3[:, :cup].double(), bt.double())


def class_weight_parts(wc: torch.Tensor, fmt_h: bool = False) -> Parts:
    """the parts of the parity-class weights: blocks of 16 low channels per (co, class, dy, dx); wc must be exact in fp32"""
    assert torch.equal(wc.double(), wc.float().double())
    return weight_parts_h(wc) if fmt_h else weight_parts(wc)


# ---- the operations, exact in float64 ------------------------------------------------------------------------------------------------------
def conv_reflect(x: torch.Tensor, w: torch.Tensor, pad_mode: str = "reflect") -> torch.Tensor:
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode=pad_mode), w)


def conv_up_low(xl: torch.Tensor, wc: torch.Tensor, pad_mode: str = "replicate") -> torch.Tensor:
    """K1u's upsampled half: output pixel (2 i + py, 2 j + px) = the 2 x 2-tap conv of class (py, px) on low rows i - 1 + py + dy, columns
    j - 1 + px + dx, clamped at the border"""
    n, _, hl, wl = xl.shape
    y = torch.zeros((n, wc.shape[0], 2 * hl, 2 * wl), dtype=torch.float64)
    xp = F.pad(xl, (1, 1, 1, 1), mode=pad_mode)
    for py in range(2):
        for px in range(2):
            t = F.conv2d(xp, wc[:, :, py, px])                                 # (n, co, hl + 1, wl + 1): entry (a, b) reads padded rows a, a + 1
            y[:, :, py::2, px::2] = t[:, :, py:py + hl, px:px + wl]
    return y


def first_layer(img: torch.Tensor, w1: torch.Tensor, b1, relu: bool = True) -> torch.Tensor:
    """K0p: the bias, then the taps of the 3 x 3 reflect window added one at a time, row-major, input plane outermost -- the order of
    wsu_conv3x3_first_pl_fwd.  In float64; the family A cases keep every partial sum exact in fp32, where no order can matter."""
    n, cin, h, w = img.shape
    xp = F.pad(img.double(), (1, 1, 1, 1), mode="reflect")
    acc = torch.zeros((n, w1.shape[0], h, w), dtype=torch.float64) + (0.0 if b1 is None else b1.double()[None, :, None, None])
    for ci in range(cin):
        for ky in range(3):
            for kx in range(3):
                acc = acc + w1[:, ci, ky, kx].double()[None, :, None, None] * xp[:, ci:ci + 1, ky:ky + h, kx:kx + w]
    return acc.clamp_min(0.0) if relu else acc


def max_pool(y: torch.Tensor) -> torch.Tensor:
    return F.max_pool2d(y, 2)


def head_logit(y: torch.Tensor, head_w: torch.Tensor, head_b) -> torch.Tensor:
    """the fused head's logit on the ReLU output y: head_b[o] + sum_c head_w[o][c] y[c]"""
    z = torch.einsum("oc,nchw->nohw", head_w.double().reshape(head_w.shape[0], -1), y)
    return z if head_b is None else z + head_b.double()[None, :, None, None]


# ---- the arithmetic: a list of (op, x parts, w parts) halves whose results add (K1q: one; K1u: the low and the skip half) ---------------------
def f16_only(halves) -> torch.Tensor:
    return sum(op(x.hi, w.hi) for op, x, w in halves)


def cross_terms(halves):
    """(res_w * copy_x, copy_w * res_x)"""
    return sum(op(x.copy, w.res) for op, x, w in halves), sum(op(x.res, w.copy) for op, x, w in halves)


def three_term(halves) -> torch.Tensor:
    a, b = cross_terms(halves)
    return f16_only(halves) + a + b


def abs_sum(halves) -> torch.Tensor:
    """sum of |term| per output (the ops have non-negative coefficients)"""
    return sum(op(torch.cat([x.hi.abs(), x.copy.abs(), x.res.abs()], dim=1), torch.cat([w.hi.abs(), w.res.abs(), w.copy.abs()], dim=1)) for op, x, w in halves)


def products_on_grid(halves, q: float) -> bool:
    for _, x, w in halves:
        for a, b in ((x.hi, w.hi), (x.copy, w.res), (x.res, w.copy)):
            pa, pb = a.abs()[a != 0], b.abs()[b != 0]
            if pa.numel() and pb.numel():
                ub = pb.unique()
                for v in pa.unique():
                    t = v * ub / q
                    if not torch.equal(t, t.round()):
                        return False
    return True


def in_window(halves, q: float, extra: float = 0.0, bound: float = 2.0 ** 24) -> bool:
    """The exactness window of family A: every product is a multiple of the quantum q (checked on the operands' parts: then every term is)
    and sum |terms| + extra (|bias|) < bound * q for every output -- with bound = 2^24 any summation order and any rounding mode of the
    matrix units give the same fp32 value; with bound = 2^11 (variants b, c) that value is also exact in f16."""
    return products_on_grid(halves, q) and float(abs_sum(halves).max()) + extra < bound * q


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


# ---- the comparisons the GPU tests use (tests/test_q4_terms_host.py feeds them wrong results) ------------------------------------------------
def exact_equal(got: torch.Tensor, want: torch.Tensor) -> bool:
    """fp32 outputs: bit for bit (as values: -0 == +0)"""
    return got.shape == want.shape and bool(torch.equal(got.detach().cpu().double(), want.double()))


def q_mismatch(got: QT, want: torch.Tensor):
    """None if the planar Q tensor `got` holds the store encoding of the exact values `want` -- f16 planes, in-image scale bytes, all 32
    nibbles, as values -- else the name of the first field that differs and the number of differing entries"""
    e = q_encode(want.float())
    if (got.n, got.c, got.h, got.w) != (e.n, e.c, e.h, e.w):
        return "shape", 0
    for name, a, b in zip(("f16 planes", "copy nibbles", "residual nibbles", "scale bytes"), q_fields(got), q_fields(e)):
        if not torch.equal(a, b):
            return name, int((a != b).sum())
    return None


def q_equal(got: QT, want: torch.Tensor) -> bool:
    return q_mismatch(got, want) is None


def a_equal(got_planes: torch.Tensor, want: torch.Tensor) -> bool:
    g, e = a_fields(got_planes), a_fields(a_encode(want.float()))
    return g[0].shape == e[0].shape and bool(torch.equal(g[0], e[0])) and bool(torch.equal(g[1], e[1]))


def h_equal(got: QT, want: torch.Tensor) -> bool:
    return (got.n, got.c, got.h, got.w) == tuple(want.shape) and bool(torch.equal(h_decode(got), f16_round(want.float())))


def q_same_bytes(a: QT, b: QT) -> bool:
    """two planar Q tensors hold the same bytes wherever the format defines them"""
    hw = a.h * a.w
    s = 48 * hw + scale_index(a.h, a.w).reshape(-1)
    da, db = a.data.cpu(), b.data.cpu()
    return (a.n, a.c, a.h, a.w) == (b.n, b.c, b.h, b.w) and bool(torch.equal(da[:, :, :48 * hw], db[:, :, :48 * hw])) and bool(torch.equal(da[:, :, s], db[:, :, s]))


RATIO_BOUND = 0.25             # family B (as tests/f16f8_np.py): a kernel without cross terms sits at 1.0, one term missing at ~0.7, one halved at ~0.35
E1_MIN = 1e-4                  # ... and the operands must really carry residuals


def ring(h: int, w: int) -> torch.Tensor:
    """the image's border ring: rows 0 and h - 1, columns 0 and w - 1"""
    m = torch.zeros((h, w), dtype=torch.bool)
    m[[0, h - 1], :] = True
    m[:, [0, w - 1]] = True
    return m


def ratio(got: torch.Tensor, want: torch.Tensor, e1: float) -> float:
    return rel_l2(got, want) / e1


def ratio_ok(got: torch.Tensor, want: torch.Tensor, e1: float) -> bool:
    return e1 >= E1_MIN and ratio(got, want, e1) <= RATIO_BOUND


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def hashed(shape, seed: int, table) -> torch.Tensor:
    """table[hash(seed, index)]: a value per element that depends on every index through an integer hash (no period in 8, 16, 32, 64)"""
    idx = np.indices(shape).astype(np.uint64)
    ks = [0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x27D4EB2F165667C5, 0x85EBCA77C2B2AE63, 0xA0761D6478BD642F]
    with np.errstate(over="ignore"):
        h = np.full(shape, (seed + 1) * 0xD6E8FEB86659FD93 % 2 ** 64, dtype=np.uint64)
        for d in range(len(shape)):
            h = (h ^ (idx[d] + np.uint64(1)) * np.uint64(ks[d])) * np.uint64(0xFF51AFD7ED558CCD)
            h ^= h >> np.uint64(33)
        h = h * np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(29)
    t = np.asarray(table, dtype=np.float64)
    return torch.from_numpy(t[(h % np.uint64(len(t))).astype(np.int64)])


def rand_act(shape, seed: int) -> torch.Tensor:
    """family B: relu(randn) times per-channel powers of two 2^-3 .. 2^3"""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(shape, generator=g))
    e = torch.randint(-3, 4, (shape[1],), generator=g).float()
    return x * torch.exp2(e)[None, :, None, None]


def rand_weight(shape, seed: int, fan_in: int) -> torch.Tensor:
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * (2.0 / fan_in) ** 0.5
