"""Self-checks of the f16f8 restatement (tests/f16f8_np.py) and of the cases of tests/test_gpu_f16f8_terms.py, without a device: the
conditions on the inputs hold, and the comparisons the GPU tests use reject a kernel without cross terms and one with a cross term's scale
off by a factor of two."""
import pytest
import torch

import f16f8_cases as C
import f16f8_np as P

A_SHAPES = {"cw": C.CW_SHAPES, "tw": C.TW_SHAPES, "cd": C.CD_SHAPES, "td": C.TD_SHAPES, "cf": C.CF_SHAPES, "tf": C.TF_SHAPES}
# one small and one multi-tile shape per kernel for the checks that need a full case
PICK = {k: [v[0], v[-2] if k in ("cw", "cf") else v[-1]] for k, v in A_SHAPES.items()}


def _pads(k):
    return (True, False) if k == "cd" else (True,)


def test_e4m3_and_copies():
    v = torch.tensor([0.0, 1.0, 0.3046875, 500.0, -500.0, 2.0 ** -9, 2.0 ** -10, 17.0, 19.0], dtype=torch.float64)
    assert P.e4m3(v).tolist() == [0.0, 1.0, 0.3125, 448.0, -448.0, 2.0 ** -9, 0.0, 16.0, 20.0]       # 4 significant bits, ties to even, saturating
    hi = torch.tensor([4.0, 8.0, 0.25, -0.25, 3000.0, -3000.0, 4.25, 200.0], dtype=torch.float64)
    assert P.copy_of(hi, P.X_LO).tolist() == [4.0, 8.0, 0.25, -0.25, 1792.0, -1792.0, 4.0, 192.0]    # e4m3(hi / 4) * 4, clamp at 1792
    assert P.copy_of(hi, P.G_LO).tolist() == [4.0, 8.0, 0.25, -0.25, 112.0, -112.0, 4.0, 112.0]      # e4m3(hi * 4) / 4, clamp at 112


def test_planes_round_trip():
    hi, res = P.hashed((2, 32, 3, 5), 1, P.ACT_A3), P.hashed((2, 32, 3, 5), 2, P.RES_A)
    p = P.parts(P.make_planes(hi, res), P.X_LO)
    assert torch.equal(p.hi, hi) and torch.equal(p.res, res / P.X_LO) and torch.equal(p.copy, hi)
    x = P.rand_act((1, 16, 4, 4), 5)
    d = P.store(x, P.X_LO)
    assert float((d - x.double()).abs().max()) <= 2.0 ** -16 * float(x.abs().max())                   # f16 + a 4-bit residual of at most 2^-12
    assert torch.equal(P.store(d.float(), P.X_LO), d)


def test_hash_is_not_periodic():
    t = P.hashed((1, 128, 8, 128), 3, list(range(7)))
    for period in (8, 16, 32, 64):
        assert not torch.equal(t[:, period:], t[:, :-period]) and not torch.equal(t[..., period:], t[..., :-period])
    assert 0.35 < float((P.hashed((1, 64, 9, 9), 4, P.ACT_A) == 0).double().mean()) < 0.75            # about half zero


@pytest.mark.parametrize("kernel", ["cd", "td", "cf", "tf"])
def test_crafted_weights_decompose_as_meant(kernel):
    shape = (64, 128, 3, 3) if kernel in ("cd", "cf") else (128, 64, 2, 2)
    w = P.crafted_weights(shape, 11, C.W_TABLE[kernel])
    hi = P.hashed(shape, 11, C.W_TABLE[kernel])
    k = torch.where(hi != 0, P.hashed(shape, 1011, P.RES_A), torch.zeros_like(hi))
    p = P.weight_parts(w)
    assert torch.equal(p.hi, hi) and torch.equal(p.res, k / 2.0 ** 18) and torch.equal(p.copy, hi)
    assert float(k.abs().max()) == 2 and float(hi.abs().max()) > 0
    # independent of torch's conversions: f16 keeps 11 significant bits, so hi + k 2^-18 (k <= 2, hi >= 2^-3) rounds to hi; e4m3 keeps 4
    assert torch.equal(w.double(), hi + k / 2.0 ** 18)
    r = P.rand_weight((64, 64, 3, 3), 3, 576)
    q = P.weight_parts(r)
    assert float((q.hi + q.res - r.double()).abs().max()) <= 2.0 ** -16 * float(r.abs().max())
    assert float((q.copy - r.double()).abs().max()) <= 2.0 ** -4 * float(r.abs().max())


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_family_a_windows_and_term_structure(kernel):
    for shape in A_SHAPES[kernel]:
        for pz in _pads(kernel):
            for v in "abcd":
                if kernel == "cf" and shape[0] == 3 and v != "d":
                    continue
                c = C.case(kernel, shape, v, pz)
                assert C.window_ok(c), (kernel, shape, v)
                raw3, raw16 = P.three_term(c["op"], c["u"], c["v"]), P.f16_only(c["op"], c["u"], c["v"])
                ca, cb = P.cross_terms(c["op"], c["u"], c["v"])
                assert torch.equal(raw3 - raw16, ca + cb)
                t = raw3 / c["q"]
                assert torch.equal(t, t.round()) and torch.equal(raw3.float().double(), raw3)           # multiples of the quantum, exact in fp32
                if v == "a":
                    assert float((ca.abs() + cb.abs()).max()) == 0 and float(raw16.abs().max()) > 0
                if v == "b":
                    assert float(ca.abs().max()) > 0 and float(cb.abs().max()) == 0
                if v == "c":
                    assert float(cb.abs().max()) > 0 and float(ca.abs().max()) == 0 and float(raw16.abs().max()) == 0
                if v == "d":
                    assert float(ca.abs().max()) > 0 and float(cb.abs().max()) > 0 and float(raw16.abs().max()) > 0


def test_window_rejects_long_reductions():
    c = dict(C.case("cw", (2, 9, 34, 64, 0, 64), "d"))
    assert C.window_ok(c)
    c["q"] = 2.0 ** -15
    assert C.window_ok(c)                                                   # a finer quantum: still inside (sum |terms| < 512)
    c["q"] = 2.0 ** -13
    assert not C.window_ok(c)                                               # not every product is a multiple
    big = C.case("cw", (1, 288, 8, 256, 0, 256), "d")
    assert float(P.abs_sum(big["op"], big["u"], big["v"]).max()) > 256      # the long column is a real reduction, and inside the window
    assert not P.in_window(big["op"], big["u"], big["v"], 2.0 ** -14 / 8)   # 2^24 quanta of an eighth would not hold it


def _halved(c, which):
    """the three-term value with one cross term's scale halved"""
    ca, cb = c["cross"]
    raw = P.f16_only(c["op"], c["u"], c["v"]) + (ca / 2 + cb if which == 0 else ca + cb / 2)
    return raw if c["mask"] is None else raw * c["mask"]


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_family_a_comparison_rejects_wrong_arithmetic(kernel):
    """what check_family_a applies: exact_equal (fp32 outputs) / planar_equal (planar outputs) on the bytes a wrong kernel would write"""
    for shape in PICK[kernel]:
        if kernel in ("cf", "tf"):
            shape = tuple(False if isinstance(s, bool) else s for s in shape)                           # (no bias / ReLU / pool: the halved term stays visible)
        for pz in _pads(kernel):
            c = C.case(kernel, shape, "d", pz)
            wrongs = [c["f16"], _halved(c, 0), _halved(c, 1)]
            if kernel in ("cw", "tw"):
                assert P.exact_equal(c["three"].float(), c["three"])
                assert not any(P.exact_equal(wv.float(), c["three"]) for wv in wrongs)
            else:
                lo = P.G_LO if kernel in ("cd", "td") else P.X_LO
                where = P.off_ring(*c["three"].shape[2:]) if (kernel == "cd" and not pz) else None
                if where is not None and not bool(where.any()):
                    continue                                                    # 2 x 2: every pixel is on the ring
                assert P.planar_equal(P.encode(c["three"], lo), c["three"], lo, where=where)
                assert not any(P.planar_equal(P.encode(wv, lo), c["three"], lo, where=where) for wv in wrongs)


B_CASES = [(k, s, pz) for k in C.KERNELS for s in C.B_SHAPES[k] for pz in _pads(k)]


@pytest.mark.parametrize("kernel,shape,pad_zero", B_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_family_b_operands_and_comparison(kernel, shape, pad_zero):
    c = C.case(kernel, shape, "B", pad_zero)
    e1 = C.e1(c)
    assert e1 >= P.E1_MIN, e1
    planar = kernel not in ("cw", "tw")
    lo = P.G_LO if kernel in ("cd", "td") else P.X_LO
    enc = (lambda t: P.store(t, lo)) if planar else (lambda t: t.float().double())
    want = enc(c["three"])
    assert P.ratio_ok(want, want, e1)
    noisy = enc(c["three"] * (1 + 2.0 ** -22 * torch.randn(c["three"].shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)))
    assert P.ratio_ok(noisy, want, e1), P.ratio(noisy, want, e1)            # fp32 accumulation noise passes
    if kernel in ("cf", "tf"):                                              # the epilogue (bias, ReLU) comes after the terms
        pre = C.case(kernel, tuple(False if isinstance(s, bool) else s for s in shape), "B", pad_zero)
        e1p = C.e1(pre)
        for wv in (pre["f16"], _halved(pre, 0), _halved(pre, 1)):
            assert not P.ratio_ok(enc(wv), enc(pre["three"]), e1p), P.ratio(enc(wv), enc(pre["three"]), e1p)
        return
    for wv in (c["f16"], _halved(c, 0), _halved(c, 1)):
        assert not P.ratio_ok(enc(wv), want, e1), P.ratio(enc(wv), want, e1)


@pytest.mark.parametrize("shape", [(1, 2, 2, 64, 64, 64, False), (1, 3, 5, 64, 64, 64, True), (1, 17, 33, 64, 64, 64, True)])
def test_reflect_pieces_sum_to_the_reflect_adjoint(shape):
    """the staging of the reflect data gradient: zero-padding adjoint + the folded strips == the reflect adjoint, exactly; and where every
    value survives the store encoding (variant a) the staged result is the plain one"""
    c = C.case("cd", shape, "d", False)
    g, w = c["u"].hi + c["u"].res, c["v"].hi
    z, *strips = P.reflect_pieces(g, w)
    h, wd = z.shape[2:]
    tot = z.clone()
    for s, si, ty, tx in P.fold_order(h, wd):
        tot[:, :, ty, tx] += strips[s - 1][:, :, si]
    assert torch.equal(tot, P.conv_dgrad(False)(g, w))
    a = C.case("cd", shape, "a", False)
    assert torch.equal(a["staged"], a["three"]) and torch.equal(a["staged16"], a["f16"])
    assert torch.equal(c["staged"][..., P.off_ring(h, wd)], c["three"][..., P.off_ring(h, wd)])
    if h > 2 and wd > 2:
        assert not torch.equal(c["staged"], c["three"])                    # on the ring the staging shows
