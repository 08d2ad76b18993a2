"""Operands and expected values of tests/test_gpu_f16f8_terms.py, built on the CPU alone (tests/test_f16f8_terms_host.py checks their
conditions without a device).  A case is a dict: the operands' bytes / fp32 weights, their parts, the exact operation, and the restated
results `three` (what products 'f16f8' must give), `f16` (products 'f16') and the two cross terms.

Family A variants (term isolation):
  a  residuals all zero                      -> three == f16
  b  u = f16 parts only, v carries residuals -> planar v: its f16 parts are zero, the result is the single term copy_u * res_v;
                                                weights v: a weight's residual needs its f16 part (a value below the f16 grid has none),
                                                so the result is f16 + copy_u * res_w and (result - f16) is the single term
  c  u = residuals only (f16 parts zero), v = f16 parts only -> the single term res_u * copy_v
  d  everything
"""
import functools

import torch

import f16f8_np as P

KERNELS = ("cw", "tw", "cd", "td", "cf", "tf")
# quantum of every product of a family A case (2^-14 for the weight gradients: 0.25 * 2^-12 and 2^-14 * 4)
QUANTUM = {"cw": 2.0 ** -14, "tw": 2.0 ** -14, "cd": 2.0 ** -20, "td": 2.0 ** -20, "cf": 2.0 ** -16, "tf": 2.0 ** -16}
W_TABLE = {"cd": [0, 0.125, 0, -0.125, 0, 0.125, 0], "td": [0, 0.5, 0, -0.5, 0, 0.5, 0],
           "cf": [0, 0.125, 0, -0.125, 0, 0.125, 0], "tf": [0, 0.5, 0, -0.5, 0, 0.5, 0]}
BIAS_A = [0.5, -1.25, 0, 2, -0.5]

# ---- family A shapes -------------------------------------------------------------------------------------------------------------------------
# conv weight gradient (n, h, w, c1, c2, cout): ring tile 2 x 32, V window 34 wide, walk down the image columns
CW_SHAPES = [(1, h, w, 64, 0, 64) for h in (2, 3, 4, 5) for w in (2, 3, 4, 5)] + [
    (1, 3, 33, 64, 0, 64), (1, 7, 32, 64, 0, 64), (2, 9, 34, 64, 0, 64),        # a column past a tile; odd rows, ragged last row pair; two tile columns
    (3, 2, 2, 64, 0, 64),                                                      # more images than tiles per image
    (1, 5, 7, 64, 128, 64), (1, 5, 7, 128, 64, 128),                           # unequal concat halves: the nb * 64 < cv1 source switch with nnb = 3
    (1, 288, 8, 256, 0, 256),                                                  # 144 tiles over 16 splits (256 CUs, 16 (mb, nb) workgroups per split): 9 tiles + the
]                                                                              # prologue = 10 steps per workgroup, the rings of 4 / 5 slots wrap
# transposed-conv weight gradient (n, h, w, cin, cout): tile rows 1 (f16f8) / 3 (f16), 32 columns
TW_SHAPES = [(1, h, w, 64, 64) for h in (1, 2, 4, 5) for w in (1, 31, 33)] + [(2, 3, 5, 128, 64), (2, 3, 5, 64, 128)]
# conv data gradient (n, h, w, cin, csplit, cout, masked); cout >= 32 is the entry's lower limit
CD_SHAPES = [(1, 2, 2, 64, 64, 64, False), (1, 3, 5, 64, 64, 64, True), (1, 5, 3, 64, 64, 64, False), (1, 17, 33, 64, 64, 64, True),
             (1, 5, 7, 128, 64, 32, True), (2, 4, 6, 128, 64, 64, True)]
# transposed-conv data gradient (n, h, w, cin, cout, masked): tile 4 x 32
TD_SHAPES = [(1, 1, 1, 64, 16, False), (1, 5, 33, 64, 32, True), (2, 2, 3, 128, 64, True)]
# conv forward (n, h, w, c1, c2, cout, relu, bias, pool)
CF_SHAPES = [(1, 2, 2, 64, 0, 64, True, False, True), (1, 17, 33, 64, 0, 64, False, True, False), (1, 4, 6, 64, 64, 128, True, True, True),
             (3, 80, 128, 64, 0, 192, True, True, False)]                       # 180 work items: beyond the small-grid variant that splits a tile's channels
# transposed-conv forward (n, h, w, cin, cout, bias): tile 4 x 32
TF_SHAPES = [(1, 1, 1, 32, 64, False), (1, 5, 33, 64, 64, True), (2, 2, 3, 128, 128, True)]

# ---- family B shapes: one tile-exact, one ragged, from the parametrisations of tests/test_gpu_planar_train.py / test_gpu_planar.py -------------
B_SHAPES = {
    "cw": [(2, 16, 32, 64, 0, 64), (1, 37, 70, 64, 0, 128)],
    "tw": [(2, 8, 32, 64, 64), (1, 13, 40, 128, 64)],
    "cd": [(2, 16, 32, 64, 64, 64, False), (1, 40, 72, 64, 64, 64, True)],
    "td": [(2, 8, 32, 64, 64, True), (1, 13, 40, 128, 64, True)],
    "cf": [(2, 16, 32, 64, 0, 64, True, True, False), (1, 18, 34, 64, 64, 128, True, True, True)],
    "tf": [(2, 8, 32, 64, 64, True), (1, 13, 40, 128, 64, True)],
}


def _operands_a(kernel, shape, variant, seed):
    """(u bytes, u parts, v bytes or fp32 weights, v parts) of a family A case"""
    ures = variant in ("c", "d")
    uhi = variant != "c"
    vres = variant in ("b", "d")
    if kernel == "cw":
        n, h, w, c1, c2, cout = shape
        ub = P.crafted((n, cout, h, w), seed, P.GRAD_A, zero_hi=not uhi, zero_res=not ures)
        vb = P.crafted((n, c1 + c2, h, w), seed + 1, P.ACT_A, zero_hi=variant == "b", zero_res=not vres)
        return ub, P.parts(ub, P.G_LO), vb, P.parts(vb, P.X_LO)
    if kernel == "tw":
        n, h, w, cin, cout = shape
        ub = P.crafted((n, cin, h, w), seed, P.ACT_A, zero_hi=not uhi, zero_res=not ures)
        vb = P.crafted((n, cout, 2 * h, 2 * w), seed + 1, P.GRAD_A, zero_hi=variant == "b", zero_res=not vres)
        return ub, P.parts(ub, P.X_LO), vb, P.parts(vb, P.G_LO)
    if kernel in ("cd", "td"):
        if kernel == "cd":
            n, h, w, cin, _, cout, _ = shape
            ushape, wshape = (n, cout, h, w), (cout, cin, 3, 3)
        else:
            n, h, w, cin, cout, _ = shape
            ushape, wshape = (n, cout, 2 * h, 2 * w), (cin, cout, 2, 2)
        ub = P.crafted(ushape, seed, P.GRAD_A, zero_hi=not uhi, zero_res=not ures)
        wt = P.crafted_weights(wshape, seed + 1, W_TABLE[kernel], zero_res=not vres)
        return ub, P.parts(ub, P.G_LO), wt, P.weight_parts(wt)
    if kernel == "cf":
        n, h, w, c1, c2, cout = shape[:6]
        ushape, wshape = (n, c1 + c2, h, w), (cout, c1 + c2, 3, 3)
    else:
        n, h, w, cin, cout = shape[:5]
        ushape, wshape = (n, cin, h, w), (cin, cout, 2, 2)
    ub = P.crafted(ushape, seed, P.ACT_A if kernel == "cf" else P.ACT_A3, zero_hi=not uhi, zero_res=not ures)
    wt = P.crafted_weights(wshape, seed + 1, W_TABLE[kernel], zero_res=not vres)
    return ub, P.parts(ub, P.X_LO), wt, P.weight_parts(wt)


def _operands_b(kernel, shape, seed):
    """realistic operands, sent through the planar encoding / kept as fp32 weights"""
    if kernel == "cw":
        n, h, w, c1, c2, cout = shape
        ub, vb = P.encode(P.rand_grad((n, cout, h, w), seed), P.G_LO), P.encode(P.rand_act((n, c1 + c2, h, w), seed + 1), P.X_LO)
        return ub, P.parts(ub, P.G_LO), vb, P.parts(vb, P.X_LO)
    if kernel == "tw":
        n, h, w, cin, cout = shape
        ub, vb = P.encode(P.rand_act((n, cin, h, w), seed), P.X_LO), P.encode(P.rand_grad((n, cout, 2 * h, 2 * w), seed + 1), P.G_LO)
        return ub, P.parts(ub, P.X_LO), vb, P.parts(vb, P.G_LO)
    if kernel == "cd":
        n, h, w, cin, _, cout, _ = shape
        ub, wt = P.encode(P.rand_grad((n, cout, h, w), seed), P.G_LO), P.rand_weight((cout, cin, 3, 3), seed + 1, 9 * cin)
        return ub, P.parts(ub, P.G_LO), wt, P.weight_parts(wt)
    if kernel == "td":
        n, h, w, cin, cout, _ = shape
        ub, wt = P.encode(P.rand_grad((n, cout, 2 * h, 2 * w), seed), P.G_LO), P.rand_weight((cin, cout, 2, 2), seed + 1, 2 * cin)
        return ub, P.parts(ub, P.G_LO), wt, P.weight_parts(wt)
    if kernel == "cf":
        n, h, w, c1, c2, cout = shape[:6]
        ub, wt = P.encode(P.rand_act((n, c1 + c2, h, w), seed), P.X_LO), P.rand_weight((cout, c1 + c2, 3, 3), seed + 1, 9 * (c1 + c2))
    else:
        n, h, w, cin, cout = shape[:5]
        ub, wt = P.encode(P.rand_act((n, cin, h, w), seed), P.X_LO), P.rand_weight((cin, cout, 2, 2), seed + 1, 2 * cin)
    return ub, P.parts(ub, P.X_LO), wt, P.weight_parts(wt)


def _op(kernel, pad_zero):
    return {"cw": P.conv_wgrad, "tw": P.convt_wgrad, "cd": P.conv_dgrad(pad_zero), "td": P.convt_dgrad, "cf": P.conv_fwd, "tf": P.convt_fwd}[kernel]


@functools.lru_cache(maxsize=None)
def case(kernel: str, shape: tuple, variant: str, pad_zero: bool = True) -> dict:
    """variant 'a' .. 'd': family A; 'B': family B.  Cached: the float64 restatement is the slow part."""
    seed = 7 + 131 * KERNELS.index(kernel) + 17 * sum((i + 1) * s for i, s in enumerate(shape) if not isinstance(s, bool))
    ub, u, vb, v = _operands_b(kernel, shape, seed) if variant == "B" else _operands_a(kernel, shape, variant, seed)
    op = _op(kernel, pad_zero)
    ca, cb = P.cross_terms(op, u, v)
    f16 = P.f16_only(op, u, v)
    c = {"kernel": kernel, "shape": shape, "variant": variant, "pad_zero": pad_zero, "op": op, "ub": ub, "u": u, "vb": vb, "v": v,
         "f16": f16, "cross": (ca, cb), "three": f16 + ca + cb, "q": QUANTUM[kernel], "extra": 0.0, "act": None, "bias": None, "mask": None}
    if kernel in ("cw", "tw"):                                              # bias gradient: the sum of the DECODED gradient / of its f16 parts
        gp = u if kernel == "cw" else v
        c["db"], c["db_f16"] = (gp.hi + gp.res).sum(dim=(0, 2, 3)), gp.hi.sum(dim=(0, 2, 3))
        c["db_abs"] = (gp.hi.abs() + gp.res.abs()).sum(dim=(0, 2, 3))
    masked = {"cd": lambda s: s[6], "td": lambda s: s[5]}.get(kernel, lambda s: False)(shape)
    if masked:                                                              # ReLU mask of the layer below: its STORED f16 part > 0
        act = P.rand_act(c["three"].shape, seed + 5) if variant == "B" else P.hashed(tuple(c["three"].shape), seed + 5, [0, 1.5, 0, 0.75, 2])
        c["act"] = P.encode(act.float(), P.X_LO)
        c["mask"] = P.parts(c["act"], P.X_LO).hi > 0
        for k in ("f16", "three"):
            c[k] = c[k] * c["mask"]
        c["cross"] = (ca * c["mask"], cb * c["mask"])
    if kernel == "cd" and not pad_zero:                                     # the border ring is stored, folded and stored again: restated as staged
        c["staged"], c["staged16"] = P.reflect_staged(u, v, "f16f8", c["mask"]), P.reflect_staged(u, v, "f16", c["mask"])
    if kernel in ("cf", "tf") and shape[7 if kernel == "cf" else 5]:
        cout = shape[5] if kernel == "cf" else shape[4]
        b = (P.hashed((cout,), seed + 9, BIAS_A) if variant != "B" else torch.randn(cout, generator=torch.Generator().manual_seed(seed + 9)).double() * 0.1).float()
        c["bias"] = b
        c["extra"] = float(b.abs().max())
        for k in ("f16", "three"):
            c[k] = c[k] + b.double()[None, :, None, None]
    if kernel == "cf" and shape[6]:                                         # ReLU (after the bias)
        for k in ("f16", "three"):
            c[k] = c[k].clamp_min(0.0)
    return c


def window_ok(c: dict) -> bool:
    """the exactness window of a family A case, from the restatement alone"""
    ok = P.in_window(c["op"], c["u"], c["v"], c["q"], c["extra"])
    if "db" in c:
        ok = ok and float(c["db_abs"].max()) < 2.0 ** 24 * 2.0 ** -14       # the gradient's residual quantum
    return ok


def e1(c: dict) -> float:
    """family B: how far the f16-only arithmetic is from the three-term arithmetic on these operands (both restatements in float64, before any
    store encoding)"""
    return P.rel_l2(c["f16"], c["three"])
