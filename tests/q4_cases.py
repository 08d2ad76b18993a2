"""Operands and expected values of tests/test_gpu_q4_terms.py, built on the CPU alone (tests/test_q4_terms_host.py checks their conditions
without a device).  A case is a dict: the operands' bytes / fp32 weights, the halves (operation, activation parts, weight parts) whose results
add, and the restated results `three` (what the kernel must give), `f16` (the first term alone) and the two cross terms.

Kinds:  'q'  conv3x3_q (K1q)          shape (n, h, w, c1, c2, cout)
        'h'  conv3x3_h (K1h)          the same, planar H operands: one product, variant 'a' only
        'u'  conv3x3_up_q (K1u)       shape (n, hl, wl, cl, cup, c2, cout): x_low at hl x wl, x_skip and y at 2 hl x 2 wl
        'uh' conv3x3_up_h             the same, planar H operands, variant 'a' only
        'f1' conv3x3_first_pl / conv3x3_q_fused_first   shape (n, h, w, cout)

Family A variants (the input bytes are free, so both cross terms isolate cleanly):
  a  residual nibbles and weight residuals zero          -> three == f16
  b  f16 planes zero, residual nibbles zero, copies set  -> the single term res_w * copy_x
  c  f16 planes zero, copy nibbles zero, residuals set   -> the single term copy_w * res_x
  d  everything
b and c run without bias and ReLU and keep sum |terms| < 2^11 q, so the output's f16 planes hold the value exactly.  'B' is family B:
realistic operands sent through the real encodings.
"""
import functools

import torch

import q4_np as P

Q = 2.0 ** -16                                         # quantum of every product of a family A case of kinds q, h, u, uh
Q_F1 = 2.0 ** -19                                      # ... of kind f1, whose activations are a computed first layer (multiples of 2^-16) times +-0.125

# ---- family A tables: 60-75 % zeros ----------------------------------------------------------------------------------------------------------
HI_X = [0, 0, 1, 0, 0, 2, 0, 0, 3, 0, 0]               # f16 parts
COPY_X = [0, 0, 2, 0, 0, 4, 0, -2, 0, 6, 0, 0, 0]      # copy nibbles (fp4 values): even, so that copy = nibble * 2^E is an integer for E = -1 too
RES_X = [0, 0, 1, 0, -1, 0, 0, 2, 0, 0, -2, 0, 3, 0]   # residual nibbles (fp4 values): res = nibble * 2^(E - 11)
E_X = [-1, 0, 0, -1, -1, 0, -1]                        # scale bytes - 127, hashed per (pixel, chunk) independently of the values
E_LOW = [0, 1, 1, 0, 0, 1, 0]                          # ... of K1u's low tensor, whose class weights carry halves (+-0.5 in wt)
W_HI = [0, 0, 0.125, 0, 0, -0.125, 0, 0, 0.1875, 0, 0, -0.1875, 0, 0]
W_K = [0, 1, 0, -1, 0, 2, 0, -2, 0]                    # weight residuals k * 2^-16, only where the f16 part is non-zero (a value below the f16
BIAS = [0.5, -1.25, 0, 2, -0.5]                        # grid is its own f16 part)

# ---- family A shapes -------------------------------------------------------------------------------------------------------------------------
# K1q (n, h, w, c1, c2, cout): one chunk per tile, every pad pixel reflects, half-block variant | odd sizes | one pixel past a 16 x 32 tile both
# ways, partial scale-plane blocks | concat with unequal halves, 5 steps (the 3-slot and the 2-slot ring wrap differently), two output
# blocks, pool | 320 work items: the non-split plain variant, workgroups walk two tiles
Q_SHAPES = [(1, 2, 2, 16, 0, 64), (1, 3, 5, 64, 0, 64), (1, 17, 33, 64, 0, 64), (1, 4, 6, 32, 48, 128)]
Q_LARGE = (5, 128, 128, 32, 0, 128)
Q_POOL = {(1, 4, 6, 32, 48, 128)}
Q_HEAD = (1, 17, 33, 64, 0, 64)
HEAD_CHANNELS = [(0, 17, 63), (5, 32, 46)]             # three one-hot head planes per launch
H_SHAPES = [(1, 2, 2, 16, 0, 64), (1, 17, 33, 64, 0, 64), (1, 4, 6, 32, 48, 128)]
# first layer (n, h, w, cout)
F1_SHAPES = [(1, 2, 2, 64), (1, 18, 34, 64), (2, 16, 64, 128)]
# K1u (n, hl, wl, cl, cup, c2, cout): 2 x 2 output, every low read clamps | exactly one tile | one pixel past the tile both ways, cup != cl / 2,
# two blocks | three low chunks + two skip chunks = five steps | more skip than low | 270 work items of three steps: the step region's
# parity flips from tile to tile inside a workgroup
U_SHAPES = [(1, 1, 1, 16, 16, 16, 64), (1, 8, 16, 32, 16, 16, 64), (1, 9, 17, 32, 32, 16, 128), (1, 2, 3, 48, 16, 32, 64), (2, 5, 7, 16, 16, 48, 64)]
U_LARGE = (3, 48, 80, 16, 16, 16, 192)
UH_SHAPES = U_SHAPES[:4]

# ---- family B shapes: one tile-exact, one ragged -------------------------------------------------------------------------------------------
B_SHAPES = {"q": [(2, 16, 32, 64, 0, 64), (1, 18, 34, 64, 64, 128)], "u": [(2, 8, 16, 64, 32, 32, 64), (1, 9, 20, 32, 16, 48, 128)]}
B_POOL = {(1, 18, 34, 64, 64, 128)}


def _seed(kind, shape):
    return 11 + 131 * ("q", "h", "u", "uh", "f1").index(kind) + 17 * sum((i + 1) * s for i, s in enumerate(shape))


def crafted_q(shape, seed, variant, e_table=E_X) -> P.QT:
    """family A planar Q operand (n, c, h, w): bytes from the tables, the scale byte hashed on its own"""
    n, c, h, w = shape
    z = torch.zeros(shape, dtype=torch.float64)
    hi = z if variant in ("b", "c") else P.hashed(shape, seed, HI_X)
    cv = z if variant == "c" else P.hashed(shape, seed + 1000, COPY_X)
    rv = z if variant in ("a", "b") else P.hashed(shape, seed + 2000, RES_X)
    e = P.hashed((n, c // 16, h, w), seed + 3000, e_table).long()
    if e.numel() > 1 and e.unique().numel() == 1:                           # a handful of scale bytes that all hashed alike: the first takes the other value
        e.view(-1)[0] = min(e_table) + max(e_table) - int(e.view(-1)[0])
    return P.make_q(hi, P.fp4_codes(cv), P.fp4_codes(rv), e)


def crafted_h(shape, seed) -> P.QT:
    return P.h_encode(P.hashed(shape, seed, HI_X))


def crafted_weights(shape, seed, variant, hi_table=W_HI) -> torch.Tensor:
    """fp32 weights  hi + k 2^-16  that the packers decompose into exactly these parts (the caller asserts it)"""
    hi = P.hashed(shape, seed, hi_table)
    k = torch.zeros(shape, dtype=torch.float64) if variant == "a" else P.hashed(shape, seed + 1000, W_K)
    return (hi + torch.where(hi != 0, k, torch.zeros_like(k)) * Q).float()


def crafted_up_weights(cl, cup, c2, cout, seed, variant):
    """K1u: (w3, wt, bt, b3) dyadic and sparse so that Wc is exact in fp32.  wt selects channels (+-1 or +-0.5 at c == ci, per sub-position);
    per (co, ci) the upsampled half of w3 is either a corner pattern -- taps (0,0), (0,2), (2,0), (2,2), each alone in its (class, dy, dx),
    values with residuals -- or a dense pattern of all nine taps from {0, +-0.125} without residuals, whose class weights are sums of up to
    four taps."""
    w3 = crafted_weights((cout, cup + c2, 3, 3), seed, variant)
    dense = P.hashed((cout, cup, 1, 1), seed + 50, [0, 0, 1, 0]) != 0
    corner = torch.zeros((3, 3), dtype=torch.bool)
    corner[0::2, 0::2] = True
    up = w3[:, :cup].double()
    dense_vals = P.hashed((cout, cup, 3, 3), seed + 51, [0, 0.125, 0, 0, -0.125, 0, 0])
    w3[:, :cup] = torch.where(dense, dense_vals, torch.where(corner, up, torch.zeros_like(up))).float()
    wt = torch.zeros((cl, cup, 2, 2), dtype=torch.float64)
    sel = P.hashed((min(cl, cup), 2, 2), seed + 52, [1, -1, 0.5, 1, -0.5, 1, 0])
    idx = torch.arange(min(cl, cup))
    wt[idx, idx] = sel
    with_bias = variant in ("a", "d")
    bt = P.hashed((cup,), seed + 53, [0, 0.5, -0.5, 1, 0]).float() if with_bias else None
    b3 = P.hashed((cout,), seed + 54, BIAS).float() if with_bias else None
    return w3, wt.float(), bt, b3


def halves_of(c: dict, neighbour_scale=False, wrong_pad=False, swap_px=False, swap_concat=False):
    """the (operation, activation parts, weight parts) halves of case c; the keyword arguments restate it WRONGLY in one way each (the
    mutants of tests/test_q4_terms_host.py)"""
    fmt_h = c["kind"] in ("h", "uh")
    xp = (lambda t: P.h_parts(t)) if fmt_h else (lambda t: P.q_parts(t, neighbour_scale))
    if c["kind"] in ("u", "uh"):
        wc = c["wc"]
        if swap_px:
            wc = P.combined_weights(c["w3"], c["wt"], c["shape"][4], swap_px=True).float()
        low = functools.partial(P.conv_up_low, pad_mode="reflect" if wrong_pad else "replicate")
        return [(low, xp(c["xl"]), P.class_weight_parts(wc, fmt_h)), (P.conv_reflect, xp(c["xs"]), c["wparts"])]
    xs = [xp(c["x1"])] + ([] if c["x2"] is None else [xp(c["x2"])])
    if swap_concat:
        xs.reverse()
    op = functools.partial(P.conv_reflect, pad_mode="replicate" if wrong_pad else "reflect")
    return [(op, xs[0] if len(xs) == 1 else P.cat_parts(*xs), c["wparts"])]


def finish(c: dict, v: torch.Tensor) -> torch.Tensor:
    """bias and ReLU of case c on the accumulated value"""
    if c["bias"] is not None:
        v = v + c["bias"].double()[None, :, None, None]
    return v.clamp_min(0.0) if c["relu"] else v


def results(c: dict, **mutant):
    """(f16 only, (cross a, cross b)) of case c before bias and ReLU"""
    hv = halves_of(c, **mutant)
    return P.f16_only(hv), P.cross_terms(hv)


def _first_layer_operands(n, h, w, c11, seed):
    """image values k / 16 and dyadic w1 = a + b 2^-12: xe11 is exact in fp32 (every partial sum a multiple of 2^-16 below 2^4) and carries
    residuals.  Channel 0 of every 16-channel chunk is the constant 1 (zero weights, bias 1): no block maximum falls below 1, so no scale
    byte puts a nibble below the quantum."""
    img = P.hashed((n, 1, h, w), seed, [k / 16.0 for k in range(17)]).float()
    w1 = (P.hashed((c11, 1, 3, 3), seed + 1, [0, 0.5, 0, -0.25, 0.25, 0, -0.5, 0]) + P.hashed((c11, 1, 3, 3), seed + 2, [0, 1, 0, -1, 3, 0, -3]) * 2.0 ** -12)
    b1 = P.hashed((c11,), seed + 3, [0, 0.5, -0.25, 0.25])
    w1[0::16], b1[0::16] = 0.0, 1.0
    return img, w1.float(), b1.float()


@functools.lru_cache(maxsize=None)
def case(kind: str, shape: tuple, variant: str) -> dict:
    """variant 'a' .. 'd': family A; 'B': family B.  Cached: the float64 restatement is the slow part."""
    seed = _seed(kind, shape)
    fam_b = variant == "B"
    plain = variant in ("b", "c")                                          # no bias, no ReLU
    c = {"kind": kind, "shape": shape, "variant": variant, "relu": not plain, "bias": None, "q": Q, "x2": None}
    if kind in ("q", "h"):
        n, h, w, c1, c2, cout = shape
        wshape = (cout, c1 + c2, 3, 3)
        if fam_b:
            x = P.rand_act((n, c1 + c2, h, w), seed)
            c["x1"], c["x2"] = P.q_encode(x[:, :c1]), (P.q_encode(x[:, c1:]) if c2 else None)
            c["w"] = P.rand_weight(wshape, seed + 1, 9 * (c1 + c2))
        elif kind == "h":
            c["x1"], c["x2"] = crafted_h((n, c1, h, w), seed), (crafted_h((n, c2, h, w), seed + 7) if c2 else None)
            c["w"] = crafted_weights(wshape, seed + 1, "a")
        else:
            c["x1"], c["x2"] = crafted_q((n, c1, h, w), seed, variant), (crafted_q((n, c2, h, w), seed + 7, variant) if c2 else None)
            c["w"] = crafted_weights(wshape, seed + 1, variant)
        c["wparts"] = P.weight_parts_h(c["w"]) if kind == "h" else P.weight_parts(c["w"])
        if not plain:
            c["bias"] = (torch.randn(cout, generator=torch.Generator().manual_seed(seed + 9)) * 0.1) if fam_b else P.hashed((cout,), seed + 9, BIAS).float()
    elif kind in ("u", "uh"):
        n, hl, wl, cl, cup, c2, cout = shape
        if fam_b:
            c["xl"], c["xs"] = P.q_encode(P.rand_act((n, cl, hl, wl), seed)), P.q_encode(P.rand_act((n, c2, 2 * hl, 2 * wl), seed + 1))
            g = torch.Generator().manual_seed(seed + 2)
            c["wt"], c["bt"] = torch.randn((cl, cup, 2, 2), generator=g) * (1.0 / cl) ** 0.5, torch.randn(cup, generator=g) * 0.1
            c["w3"], c["b3"] = torch.randn((cout, cup + c2, 3, 3), generator=g) * (2.0 / (9 * (cup + c2))) ** 0.5, torch.randn(cout, generator=g) * 0.1
        else:
            if kind == "uh":
                c["xl"], c["xs"] = crafted_h((n, cl, hl, wl), seed), crafted_h((n, c2, 2 * hl, 2 * wl), seed + 7)
            else:
                c["xl"], c["xs"] = crafted_q((n, cl, hl, wl), seed, variant, E_LOW), crafted_q((n, c2, 2 * hl, 2 * wl), seed + 7, variant)
            c["w3"], c["wt"], c["bt"], c["b3"] = crafted_up_weights(cl, cup, c2, cout, seed + 1, "a" if kind == "uh" else variant)
        wc64 = P.combined_weights(c["w3"], c["wt"], cup)
        c["wc"] = wc64.float()                                              # family A: exact (asserted); family B: the fp64 sums rounded once
        c["wc_exact"] = bool(torch.equal(c["wc"].double(), wc64))
        c["wparts"] = (P.weight_parts_h if kind == "uh" else P.weight_parts)(c["w3"][:, cup:].contiguous())
        b64 = P.combined_bias(c["w3"], c["bt"], c["b3"], cup)
        c["bias"] = b64.float()
        c["bias_exact"] = bool(torch.equal(c["bias"].double(), b64))
    else:                                                                   # f1: first layer -> planar Q -> conv (+ pool)
        n, h, w, cout = shape
        c["q"] = Q_F1
        c["img"], c["w1"], c["b1"] = _first_layer_operands(n, h, w, 64, seed)
        xe = P.first_layer(c["img"], c["w1"], c["b1"])
        c["xe11"] = xe
        c["xe11_exact"] = bool(torch.equal(xe, xe.float().double()))
        c["x1"] = P.q_encode(xe.float())
        c["w"] = crafted_weights((cout, 64, 3, 3), seed + 5, variant, [0, 0, 0, 0.125, 0, 0, 0, -0.125, 0, 0, 0, 0, 0])
        c["wparts"] = P.weight_parts(c["w"])
        c["bias"] = P.hashed((cout,), seed + 9, BIAS).float()
    f16, (ca, cb) = results(c)
    c["halves"] = halves_of(c)
    c["raw"] = (f16, ca, cb)
    c["cross"] = (ca, cb)
    c["f16"], c["three"] = finish(c, f16), finish(c, f16 + ca + cb)
    c["extra"] = 0.0 if c["bias"] is None else float(c["bias"].abs().max())
    return c


def first_pl_case(shape: tuple) -> dict:
    """conv3x3_first_pl alone: (n, h, w, cout) with cout first-layer channels; the exact fp32 values its three store encodings are made of"""
    n, h, w, cout = shape
    img, w1, b1 = _first_layer_operands(n, h, w, cout, _seed("f1", shape) + 1)
    y = P.first_layer(img, w1, b1)
    assert torch.equal(y, y.float().double())
    return {"img": img, "w1": w1, "b1": b1, "y": y}


def window_ok(c: dict) -> bool:
    """the exactness window of a family A case, from the restatement alone (variants b, c: also exact in the f16 planes of the output)"""
    return P.in_window(c["halves"], c["q"], c["extra"], 2.0 ** 11 if c["variant"] in ("b", "c") else 2.0 ** 24)


def e1(c: dict) -> float:
    """family B: how far the f16-only arithmetic is from the three-term arithmetic on these operands (float64, before any store encoding)"""
    return P.rel_l2(c["f16"], c["three"])


def a_cases():
    """every family A case: (kind, shape, variant)"""
    out = [("q", s, v) for s in Q_SHAPES for v in "abcd"] + [("q", Q_LARGE, "d")]
    out += [("h", s, "a") for s in H_SHAPES]
    out += [("u", s, v) for s in U_SHAPES for v in "abcd"] + [("u", U_LARGE, "d")]
    out += [("uh", s, "a") for s in UH_SHAPES]
    out += [("f1", s, "d") for s in F1_SHAPES]
    return out
