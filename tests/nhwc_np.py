"""fp64 torch-CPU / numpy restatements of the NHWC pointwise, pool, head and first-layer kernels (csrc/pointwise.hip, the non-matrix half
of csrc/backward.hip), for tests/test_gpu_nhwc_edges.py.  Every function that feeds a tolerance returns the pair (ref, S): the operation in
fp64 and the same operation on absolute values, S = sum |x| |w| + |bias| per output element.

Two kinds of input:
  dyadic()  multiples of 2^-3 of magnitude <= amax: every product and every partial sum of a dot product is exact in fp32 in any order, so
            the kernel equals the reference BIT FOR BIT (exact_budget() asserts on the reference that the promise holds);
  rand()    normal values: |kernel - ref| <= dot_bound(K, S) = (K + 4) 2^-24 S for a K-term fp32 dot product in any order, with or without
            fma (each of the K - 1 additions and K products rounds once, (1 + 2^-24)^(K+4) - 1 <= (K + 4) 2^-24 to first order; the 4 spare
            roundings cover the bias, a sigmoid-derivative factor of two roundings and the final store)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import np_ops

U24 = 2.0 ** -24
BF16_HALF_ULP = 2.0 ** -8            # round to nearest on 8 significant bits: |bf16(v) - v| <= 2^-9 * 2^ceil(log2 |v|) <= 2^-8 |v|


def dyadic(shape, seed, amax=4.0, device="cpu"):
    k = int(amax * 8)
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-k, k + 1, tuple(shape), generator=g, device=device).float() / 8.0


def rand(shape, seed, scale=1.0, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(tuple(shape), generator=g, device=device) * scale


def exact_budget(ref: torch.Tensor, s_abs: torch.Tensor, quantum: float) -> None:
    """The promise of the exact inputs, asserted on the reference alone: the result is an fp32 number, and the absolute sum of the terms (all
    multiples of `quantum`) stays below 2^24 quanta, so no partial sum in any order needs more than 24 bits."""
    assert torch.equal(ref.float().double(), ref)
    assert float(s_abs.max()) / quantum < 2.0 ** 24, (float(s_abs.max()) / quantum)


def dot_bound(k: int, s_abs: torch.Tensor) -> torch.Tensor:
    return (k + 4) * U24 * s_abs


def bf16_bound(e: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """an fp32 value within e of ref, rounded to nearest bf16: |bf16(v) - ref| <= e + 2^-8 |v| <= e (1 + 2^-8) + 2^-8 |ref|"""
    return e * (1.0 + BF16_HALF_ULP) + BF16_HALF_ULP * ref.abs()


def ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """largest err / bound; a zero bound (every term zero) admits only a zero error"""
    err = (got.double().cpu() - ref.double().cpu()).abs()
    b = bound.double().cpu()
    r = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def _pad(x):
    return F.pad(x, (1, 1, 1, 1), mode="reflect")


# ---- first layer ----------------------------------------------------------------------------------------------------------------------------------
def conv_first(x, w, b, relu):
    """x (N,cin,H,W), w (cout,cin,3,3), b (cout) or None -> NHWC (ref, S); K = 9 cin + 1"""
    xp, w64 = _pad(x.double()), w.double()
    ref = F.conv2d(xp, w64, None if b is None else b.double())
    s = F.conv2d(xp.abs(), w64.abs(), None if b is None else b.double().abs())
    if relu:
        ref = ref.clamp_min(0.0)
    return ref.permute(0, 2, 3, 1).contiguous(), s.permute(0, 2, 3, 1).contiguous()


def conv_first_wgrad(g, x):
    """g (N,H,W,cout), x (N,cin,H,W) (any device) -> (dw, S_dw, db, S_db); K = N H W"""
    n, h, w, cout = g.shape
    cin = x.shape[1]
    cols = F.unfold(_pad(x.double()), 3)                       # (n, cin * 9, h w), row ci * 9 + u * 3 + v
    gm = g.double().reshape(n, h * w, cout)
    dw = torch.einsum("nkp,npo->ok", cols, gm).reshape(cout, cin, 3, 3)
    sw = torch.einsum("nkp,npo->ok", cols.abs(), gm.abs()).reshape(cout, cin, 3, 3)
    return dw, sw, gm.sum((0, 1)), gm.abs().sum((0, 1))


def conv_first_dgrad(g, w):
    """g (N,H,W,cout), w (cout,cin,3,3) -> (dx, S) NCHW: fp64 autograd of conv2d(pad(x, reflect), w).  All coefficients of the adjoint are
    products of entries of w, so the adjoint of (|g|, |w|) is S.  K <= 36 cout (up to four padded positions fold onto a pixel)."""
    n, h, wd, cout = g.shape
    cin = w.shape[1]

    def adj(gg, ww):
        x = torch.zeros((n, cin, h, wd), dtype=torch.float64, device=g.device, requires_grad=True)
        F.conv2d(_pad(x), ww).backward(gg.permute(0, 3, 1, 2))
        return x.grad
    return adj(g.double(), w.double()), adj(g.double().abs(), w.double().abs())


# ---- head -----------------------------------------------------------------------------------------------------------------------------------------
def head_fwd(x, w, b):
    """x (N,H,W,C), w (cout,C), b (cout) or None -> NCHW (logit, S); K = C + 1"""
    z = torch.einsum("nhwc,oc->nohw", x.double(), w.double())
    s = torch.einsum("nhwc,oc->nohw", x.double().abs(), w.double().abs())
    if b is not None:
        z, s = z + b.double()[None, :, None, None], s + b.double().abs()[None, :, None, None]
    return z, s


def head_bwd(x, w, out, dout, relu_mask):
    """-> dict of (ref, S) for gx (N,H,W,C; K = cout), dw (cout,C; K = N H W), db (cout; K = N H W); dz = dout out (1 - out)"""
    x64, w64 = x.double(), w.double()
    dz = dout.double() * out.double() * (1.0 - out.double())
    gx = torch.einsum("nohw,oc->nhwc", dz, w64)
    sgx = torch.einsum("nohw,oc->nhwc", dz.abs(), w64.abs())
    if relu_mask:
        gx, sgx = gx * (x > 0), sgx * (x > 0)
    dw = torch.einsum("nohw,nhwc->oc", dz, x64)
    sdw = torch.einsum("nohw,nhwc->oc", dz.abs(), x64.abs())
    return {"gx": (gx, sgx), "dw": (dw, sdw), "db": (dz.sum((0, 2, 3)), dz.abs().sum((0, 2, 3)))}


# ---- max-pool -------------------------------------------------------------------------------------------------------------------------------------
def pool_fwd(x_nhwc: np.ndarray):
    """np_ops.maxpool2x2 on the even crop of an NHWC array -> (values, argmax) NHWC"""
    n, h, w, c = x_nhwc.shape
    v, a = np_ops.maxpool2x2(np.ascontiguousarray(x_nhwc[:, :h // 2 * 2, :w // 2 * 2].transpose(0, 3, 1, 2)))
    return v.transpose(0, 2, 3, 1), a.transpose(0, 2, 3, 1)


def pool_windows(x_nhwc: np.ndarray) -> np.ndarray:
    """(N, H/2, W/2, C, 4): the windows in the order (0,0) (0,1) (1,0) (1,1)"""
    n, h, w, c = x_nhwc.shape
    e = x_nhwc[:, :h // 2 * 2, :w // 2 * 2]
    return np.stack([e[:, 0::2, 0::2], e[:, 0::2, 1::2], e[:, 1::2, 0::2], e[:, 1::2, 1::2]], axis=-1)


def pool_bwd_routed(dyp, idx, mask, h, w):
    """the pooled gradient at the recorded position of every window, where mask > 0; zero in a dropped last row / column (fp32, NHWC)"""
    n, hp, wp, c = dyp.shape
    routed = torch.zeros((n, h, w, c), dtype=torch.float32)
    keep = torch.ones_like(dyp, dtype=torch.bool) if mask is None else mask > 0
    for k, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        routed[:, a:2 * hp:2, b:2 * wp:2] = torch.where((idx == k) & keep, dyp, torch.zeros_like(dyp))
    return routed


# ---- UniformDropout -------------------------------------------------------------------------------------------------------------------------------
def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def dropout_mask(n, h, w, keep_prob, seed) -> np.ndarray:
    """the drawn keep-mask (N,1,H,W): a counter-based hash of (seed, index in the mask), compared in fp64 with the fp32 keep_prob"""
    with np.errstate(over="ignore"):
        mi = np.arange(n * h * w, dtype=np.uint64)
        gold = np.uint64(0x9E3779B97F4A7C15)
        r = _mix64(_mix64(mi * gold + np.uint64(seed)) + gold)
    u = (r >> np.uint64(32)).astype(np.float64) * (1.0 / 4294967296.0)
    return (u < np.float64(np.float32(keep_prob))).astype(np.float32).reshape(n, 1, h, w)


def dropout(x: torch.Tensor, mask: torch.Tensor, channel: int) -> torch.Tensor:
    """fp32, one IEEE operation after another in the kernel's row-major order (no contraction: every torch call rounds once).  x (N,C,H,W),
    mask (N,1,H,W), on any device."""
    p = x[:, channel:channel + 1]
    pp = _pad(p)
    h, w = x.shape[2:]
    taps = [(-0.25, 0, 0), (0.5, 0, 1), (-0.25, 0, 2), (0.5, 1, 0), (0.5, 1, 2), (-0.25, 2, 0), (0.5, 2, 1), (-0.25, 2, 2)]
    kb = None
    for coef, u, v in taps:
        term = pp[:, :, u:u + h, v:v + w] * coef
        kb = term if kb is None else kb + term
    y = x.clone()
    y[:, channel:channel + 1] = p * mask + kb * (1.0 - mask)
    return y


# ---- WS statistics --------------------------------------------------------------------------------------------------------------------------------
def ws_stats(u8: np.ndarray, y01: np.ndarray):
    """oracle/np_ops.ws_stats with its float32 operation sequence (x - float32(y * 255), the product in float32), accumulated in fp64:
    (beta_hat, l1) per image as fp64, before the one rounding to float32"""
    x = u8[:, 1:-1, 1:-1].astype(np.float32)
    xbar = (u8[:, 1:-1, 1:-1] ^ 1).astype(np.float32)
    d = x - y01[:, 1:-1, 1:-1].astype(np.float32) * np.float32(255.0)
    assert d.dtype == np.float32
    cnt = x.shape[1] * x.shape[2]
    return ((x - xbar) * d).astype(np.float64).sum((1, 2)) / cnt, np.abs(d).astype(np.float64).sum((1, 2)) / cnt


def ws_meter(x01: np.ndarray, y01: np.ndarray):
    """metrics.WSMeter.update's beta_hat in fp64 on the same float32 xi -> (beta, sum |term|) per image"""
    xi = x01[:, 1:-1, 1:-1].astype(np.float32) * np.float32(255.0)
    xh = y01[:, 1:-1, 1:-1].astype(np.float32) * np.float32(255.0)
    x_bar = np.round(xi).astype("int") ^ 1
    term = (xi - x_bar) * (xi - xh) / np.prod(xi.shape[1:])
    assert term.dtype == np.float64 and (xi - xh).dtype == np.float32
    return term.sum((1, 2)), np.abs(term).sum((1, 2))


def half_ties():
    """float32 x in [0, 1] with float32(x * 255) == k + 0.5 exactly -> (x of even k, x of odd k)"""
    even, odd = [], []
    for k in range(255):
        x = np.float32((k + 0.5) / 255.0)
        for _ in range(4):
            x = np.nextafter(x, np.float32(0))
        for _ in range(9):
            if x * np.float32(255.0) == np.float32(k + 0.5):
                (odd if k & 1 else even).append(x)
                break
            x = np.nextafter(x, np.float32(2))
    return np.array(even, np.float32), np.array(odd, np.float32)
