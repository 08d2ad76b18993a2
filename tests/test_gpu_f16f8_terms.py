"""The six matrix kernels of the planar training path with products 'f16f8', held to THEIR arithmetic -- f16 a * f16 b on the f16 pipe plus the
two residual cross terms on the block-scaled fp8 pipe (wsu_mfma_f8x2) -- as restated in tests/f16f8_np.py.  The oracle bands of
tests/test_gpu_planar_train.py cannot tell this arithmetic from its f16-only sibling; these tests can.

Family A (bit for bit): operands crafted as bytes from small dyadic sets, so that every product is a multiple of one quantum and the sum of
their magnitudes stays below 2^24 quanta -- any summation order and any rounding mode then give one fp32 value.  Each kernel runs with
(a) no residuals, (b) / (c) one cross term alone, (d) all three terms (tests/f16f8_cases.py).  Under reflect padding the data gradient
stores the zero-padding adjoint and the four strips' 1x3 convolutions, folds the strips onto the border ring (rows 1, h-2, columns 1, w-2)
in fp32 in a fixed order and stores the ring again; the restatement stages the store encoding the same way (f16f8_np.reflect_staged), so
the ring is held bit for bit too, in both families.

Family B (realistic operands): E1 = rel_l2(f16-only, three-term) on the CPU; the kernel must sit within 0.25 E1 of the three-term value (a
kernel without cross terms sits at 1.0, with one term missing at ~0.7, with one term off by a factor of two at ~0.35 .. 0.7).

Observed on an MI355X (profiles/r43), rel_l2(got, three-term restatement) / E1 with E1 = 2.7e-4 .. 3.0e-4, worst case per kernel:
    conv weight gradient 0.0006, transposed-conv weight gradient 0.0004 (fp32 outputs: accumulation order only);
    conv data gradient 0.0053 (either padding), transposed-conv data gradient 0.0041, conv forward 0.0065 (pooled 0.0064), transposed-conv
    forward 0.0035 (planar outputs: last-place flips of the store encoding where the fp32 sums differ in their last bit).
    products 'f16' against the f16-only restatement: 0.0006, 0.0003, 0.0411, 0.0147 (an f16 tensor: a flip is a whole f16 place).
The staged restatement of the reflect ring matters: against a single store encoding of the reflect adjoint the same correct kernels gave
0.010 .. 0.013 (f16f8) and 0.34 .. 0.51 (products 'f16', whose ring pixels are rounded to f16 twice), the latter above the bound.

The conv data gradient's entry refuses cout < 32, so its small-cout case is 32.  A weight's residual needs its f16 part (a value below the f16
grid is its own f16 part), so for the four kernels that take packed weights variant (b) is f16 term + one cross term, not the cross term alone.
"""
import pytest
import torch
import torch.nn.functional as F

import f16f8_cases as C
import f16f8_np as P
from gpu_util import DEV, planar_encode

pytestmark = pytest.mark.gpu


def _ops():
    from ws_unet_amd import ops
    return ops


def _dev(planes, lo=None, hi=None):
    return P.as_device_planar(planes if lo is None else planes[:, lo:hi], DEV)


def _planes(*ts):
    return torch.cat([t.detach().contiguous().view(torch.uint8).cpu() for t in ts if t is not None], dim=1)


def run(c: dict, products: str = "f16f8", want_bias: bool = True) -> dict:
    """the kernel of case c -> {'dw', 'db'} (fp32, CPU) or {'y'[, 'pool', 'flag']} (planar bytes, CPU)"""
    ops = _ops()
    k, s = c["kernel"], c["shape"]
    if k == "cw":
        c1 = s[3]
        dw, db = ops.conv3x3_pl_bwd_weight(_dev(c["ub"]), _dev(c["vb"], 0, c1 // 16), _dev(c["vb"], c1 // 16, None) if s[4] else None,
                                           want_bias=want_bias, products=products)
        return {"dw": dw.cpu(), "db": None if db is None else db.cpu()}
    if k == "tw":
        dw, db = ops.convt2x2_pl_bwd_weight(_dev(c["ub"]), _dev(c["vb"]), want_bias=want_bias, products=products)
        return {"dw": dw.cpu(), "db": None if db is None else db.cpu()}
    if k == "cd":
        cin, csplit = s[3], s[4]
        wd = c["vb"].to(DEV)
        wp = ops.pack_conv3x3(wd, ops.MODE_F16F8, dgrad=True)
        wr = None if c["pad_zero"] else ops.pack_conv3x3_ring(wd)
        m1 = None if c["act"] is None else _dev(c["act"], 0, csplit // 16)
        m2 = None if (c["act"] is None or csplit == cin) else _dev(c["act"], csplit // 16, None)
        dx1, dx2 = ops.conv3x3_pl_bwd_data(_dev(c["ub"]), wp, wr, cin, csplit, m1, m2, pad_zero=c["pad_zero"], products=products)
        return {"y": _planes(dx1, dx2)}
    if k == "td":
        wp = ops.pack_convt2x2_pl_dgrad(c["vb"].to(DEV))
        dx = ops.convt2x2_pl_bwd_data(_dev(c["ub"]), wp, s[3], None if c["act"] is None else _dev(c["act"]), products=products)
        return {"y": _planes(dx)}
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    bias = None if c["bias"] is None else c["bias"].to(DEV)
    if k == "cf":
        c1, c2, cout, relu, pool = s[3], s[4], s[5], s[6], s[8]
        wp = ops.pack_conv3x3(c["vb"].to(DEV), ops.MODE_F16F8)
        res = ops.conv3x3_pl(_dev(c["ub"], 0, c1 // 16), _dev(c["ub"], c1 // 16, None) if c2 else None, wp, bias, cout, relu=relu, pool=pool,
                             range_flag=flag)
        out = {"y": _planes(res[0] if pool else res), "flag": int(flag.item())}
        if pool:
            out["pool"] = _planes(res[1])
        return out
    wp = ops.pack_convt2x2(c["vb"].to(DEV), ops.MODE_F16F8)
    y = ops.convt2x2_pl(_dev(c["ub"]), wp, bias, s[4], range_flag=flag)
    return {"y": _planes(y), "flag": int(flag.item())}


def _out_lo(k):
    return P.G_LO if k in ("cd", "td") else P.X_LO


def check_family_a(c: dict, out: dict, products: str = "f16f8") -> None:
    """bit-for-bit against the restatement (the window is a condition on the inputs, asserted first)"""
    assert C.window_ok(c), "the operands leave the exactness window"
    k, v = c["kernel"], c["variant"]
    want = c["three"] if products == "f16f8" else c["f16"]
    ca, cb = c["cross"]
    if v == "a":
        assert torch.equal(c["three"], c["f16"])
    if v == "b":
        assert float(ca.abs().max()) > 0 and float(cb.abs().max()) == 0
        if k in ("cw", "tw"):
            assert float(c["f16"].abs().max()) == 0                       # the single term copy_u * res_v
    if v == "c":
        assert float(cb.abs().max()) > 0 and float(ca.abs().max()) == 0 and float(P.f16_only(c["op"], c["u"], c["v"]).abs().max()) == 0
    if v in ("b", "c") and c["bias"] is None and not (k == "cf" and c["shape"][6]):
        assert float(want.abs().max()) > 0 or products == "f16"
    if k in ("cw", "tw"):
        assert P.exact_equal(out["dw"], want), (k, c["shape"], v, float((out["dw"].double() - want).abs().max()))
        if out["db"] is not None:
            db = c["db"] if products == "f16f8" else c["db_f16"]
            assert P.exact_equal(out["db"], db), (k, c["shape"], v)
        return
    lo = _out_lo(k)
    if "staged" in c:                                                     # reflect padding: off the ring the plain store encoding, on it the staged one
        h, w = want.shape[2:]
        assert P.planar_equal(out["y"], want, lo, where=P.off_ring(h, w), residual=products == "f16f8"), (k, c["shape"], v, "off the ring")
        want = c["staged"] if products == "f16f8" else c["staged16"]
    assert P.planar_equal(out["y"], want, lo, residual=products == "f16f8"), (k, c["shape"], v, c["pad_zero"])
    if c["mask"] is not None:
        got = P.parts(out["y"], lo)
        assert float(got.hi[~c["mask"]].abs().max()) == 0 and (products == "f16" or float(got.res[~c["mask"]].abs().max()) == 0)
    if "pool" in out:
        assert P.planar_equal(out["pool"], F.max_pool2d(want, 2), lo)
    if "flag" in out:
        assert out["flag"] == 0


VARIANTS = ["a", "b", "c", "d"]


def test_store_encoding_restatement_matches_gpu_util():
    x = P.rand_grad((2, 32, 5, 7), 3) * 1.001
    for lo in (P.X_LO, P.G_LO):
        assert torch.equal(P.encode(x, lo), planar_encode(x, lo).view(torch.uint8).cpu())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", C.CW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_conv3x3_wgrad(shape, variant):
    c = C.case("cw", shape, variant)
    check_family_a(c, run(c))


def test_a_conv3x3_wgrad_without_bias():
    c = C.case("cw", (2, 9, 34, 64, 0, 64), "d")
    out = run(c, want_bias=False)
    assert out["db"] is None
    check_family_a(c, out)


@pytest.mark.parametrize("shape", [(2, 9, 34, 64, 0, 64), (1, 24, 8, 64, 0, 64)], ids=lambda s: "x".join(map(str, s)))
def test_a_conv3x3_wgrad_workspace_splits(shape):
    """run_wgrad_pl sizes its splits by the workspace: the full size, exactly one slab (one split: a single workgroup walks every tile -- 12
    tiles + a prologue per column for the second shape, the rings wrap) and two slabs + 4 bytes give identical, exact bits; one byte less
    than a slab is an argument error that writes nothing."""
    from ws_unet_amd import _lib
    lib = _lib.load()
    c = C.case("cw", shape, "d")
    assert C.window_ok(c)
    n, h, w, c1, _, cout = shape
    g, x = _dev(c["ub"]), _dev(c["vb"])
    slab, bslab = (cout // 64) * (c1 // 64) * 9 * 4096 * 4, cout * 4
    full = int(lib.wsu_wgrad_workspace_bytes(cout, c1, 9))
    ws = torch.zeros(full // 4 + 2, dtype=torch.float32, device=DEV)

    def call(nbytes, dw, db):
        return lib.wsu_conv3x3_pl_bwd_weight(g.data_ptr(), x.data_ptr(), None, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes,
                                             n, h, w, c1, 0, cout, 0, _ops()._stream())
    for nbytes in (full, slab + bslab, 2 * (slab + bslab) + 4):
        dw = torch.full((cout, c1, 3, 3), 7.5, dtype=torch.float32, device=DEV)
        db = torch.full((cout,), 7.5, dtype=torch.float32, device=DEV)
        assert call(nbytes, dw, db) == 0, nbytes
        torch.cuda.synchronize()
        assert P.exact_equal(dw.cpu(), c["three"]) and P.exact_equal(db.cpu(), c["db"]), nbytes
    dw = torch.full((cout, c1, 3, 3), 7.5, dtype=torch.float32, device=DEV)
    db = torch.full((cout,), 7.5, dtype=torch.float32, device=DEV)
    assert call(slab + bslab - 1, dw, db) == -1                            # WSU_ERR_ARG
    torch.cuda.synchronize()
    assert bool((dw == 7.5).all()) and bool((db == 7.5).all())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", C.TW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_convt2x2_wgrad(shape, variant):
    c = C.case("tw", shape, variant)
    check_family_a(c, run(c))


@pytest.mark.parametrize("shape", [(1, 4, 33, 64, 64), (1, 5, 31, 64, 64), (2, 3, 5, 128, 64)], ids=lambda s: "x".join(map(str, s)))
def test_a_convt2x2_wgrad_f16_products(shape):
    """variant (a) with products 'f16': the instantiation with 3 tile rows at heights that are no multiple of 3"""
    c = C.case("tw", shape, "a")
    check_family_a(c, run(c, products="f16"), products="f16")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("pad_zero", [True, False])
@pytest.mark.parametrize("shape", C.CD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_conv3x3_dgrad(shape, pad_zero, variant):
    c = C.case("cd", shape, variant, pad_zero)
    check_family_a(c, run(c))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", C.TD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_convt2x2_dgrad(shape, variant):
    c = C.case("td", shape, variant)
    check_family_a(c, run(c))


@pytest.mark.parametrize("shape,variant", [(s, v) for s in C.CF_SHAPES for v in VARIANTS if s[0] != 3 or v == "d"],      # (the large grid: all three terms only)
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_a_conv3x3_fwd(shape, variant):
    c = C.case("cf", shape, variant)
    check_family_a(c, run(c))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", C.TF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_convt2x2_fwd(shape, variant):
    c = C.case("tf", shape, variant)
    check_family_a(c, run(c))


# ---- family B ------------------------------------------------------------------------------------------------------------------------------
def _value(c, out, products="f16f8"):
    """(what the kernel gave, what the restatement gives after the store encoding) as float64"""
    k = c["kernel"]
    want = c["three"] if products == "f16f8" else c["f16"]
    if "staged" in c:                                                       # reflect padding: the staged store encoding of the border ring
        want = c["staged"] if products == "f16f8" else c["staged16"]
    if k in ("cw", "tw"):
        return out["dw"].double(), want
    lo = _out_lo(k)
    p = P.parts(out["y"], lo)
    if products == "f16":                                                   # no residual plane: one f16 rounding
        return p.hi, want.float().half().double()
    return p.hi + p.res, P.store(want, lo)


B_CASES = [(k, s, pz) for k in C.KERNELS for s in C.B_SHAPES[k] for pz in ((True, False) if k == "cd" else (True,))]


@pytest.mark.parametrize("kernel,shape,pad_zero", B_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_b_three_term_arithmetic(kernel, shape, pad_zero):
    c = C.case(kernel, shape, "B", pad_zero)
    e1 = C.e1(c)
    assert e1 >= P.E1_MIN, e1                                               # a condition on the operands: they carry residuals
    out = run(c)
    got, want = _value(c, out)
    r = P.ratio(got, want, e1)
    print(f"f16f8 terms: {kernel} {shape} pad_zero={pad_zero} E1={e1:.3e} ratio={r:.4f}")
    assert P.ratio_ok(got, want, e1), (r, e1)
    if c["mask"] is not None:
        assert float(got[~c["mask"]].abs().max()) == 0
    if "pool" in out:
        pl = P.parts(out["pool"], P.X_LO)
        rp = P.ratio(pl.hi + pl.res, P.store(F.max_pool2d(c["three"], 2), P.X_LO), e1)
        print(f"f16f8 terms: {kernel} {shape} pooled ratio={rp:.4f}")
        assert rp <= P.RATIO_BOUND, rp
    if "flag" in out:
        assert out["flag"] == 0
    if kernel in ("cw", "tw", "cd", "td"):                                  # products 'f16' on the same operands: the first term alone
        out16 = run(c, products="f16")
        got16, want16 = _value(c, out16, "f16")
        r16 = P.ratio(got16, want16, e1)
        print(f"f16f8 terms: {kernel} {shape} pad_zero={pad_zero} products f16 ratio={r16:.4f}")
        assert r16 <= P.RATIO_BOUND, (r16, e1)
        assert not torch.equal(got16, got)
