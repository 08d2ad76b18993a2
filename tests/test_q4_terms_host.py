"""CPU checks of the operands and comparisons of tests/test_gpu_q4_terms.py: every family A case lies in its exactness window, the crafted
weights decompose into the intended parts under the restated packers, the scale bytes of every crafted tensor take more than one value --
and the comparisons reject wrong restatements of the arithmetic (a dropped, doubled or halved cross term, scale bytes gathered from the
neighbouring pixel, the wrong padding, swapped parity classes, a truncated residual nibble, swapped concat halves), bit for bit in family A
and through the ratio in family B.  No device, no library."""
import pytest
import torch

import q4_cases as C
import q4_np as P

A_CASES = C.a_cases()
_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_fp4_rounding_and_block_scale():
    v = torch.tensor([0.0, 0.25, 0.26, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 5.01, 7.0, -0.75, -100.0], dtype=torch.float64)
    assert P.fp4_values(P.fp4_codes(v)).tolist() == [0.0, 0.0, 0.5, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0, 6.0, -1.0, -6.0]      # ties to the even code
    assert P.fp4_values(P.fp4_codes(v, truncate=True)).tolist() == [0.0, 0.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 4.0, 6.0, -0.5, -6.0]
    amax = torch.tensor([0.0, 2.0 ** -20, 1.0, 1.5, 1.5 + 2.0 ** -10, 1.999, 448.0, 6.0])
    e = P.block_exp(amax)
    assert e.tolist() == [-16, -16, -2, -2, -1, -1, 7, 0]
    q = amax[2:].double() / torch.exp2(e[2:].double())                     # the smallest power of two that does not saturate: the largest lands in [2, 4) or [4, 6]
    assert bool(((q >= 2) & (q <= 6)).all()) and bool((P.fp4_values(P.fp4_codes(q)) >= 2).all())
    assert bool((amax[2:].double() / torch.exp2(e[2:].double() - 1) > 6).all())      # one binade finer would saturate


def test_q_bytes_round_trip():
    """make_q / q_fields are inverse on crafted bytes, and a real encoding decodes to within the format's residual step"""
    t = C.crafted_q((2, 32, 17, 33), 5, "d")
    hi, cv, rv, e = P.q_fields(t)
    again = P.make_q(hi, P.fp4_codes(cv), P.fp4_codes(rv), e)
    assert torch.equal(again.data, t.data)
    x = P.rand_act((1, 32, 19, 45), 3)
    back = P.q_decode(P.q_encode(x))
    amax = P._chunked(x).abs().amax(dim=-1).repeat_interleave(16, dim=1)
    assert bool(((back - x.double()).abs() <= 2.0 ** -12 * amax.double()).all())
    assert torch.equal(P.h_decode(P.h_encode(x)), P.f16_round(x))
    assert float((P.a_decode(P.a_encode(x)) - x.double()).abs().max()) <= 2.0 ** -16 * float(x.abs().max())


@pytest.mark.parametrize("kind,shape,variant", A_CASES, ids=_id)
def test_family_a_case_conditions(kind, shape, variant):
    c = C.case(kind, shape, variant)
    assert C.window_ok(c)
    hv = c["halves"]
    assert P.products_on_grid(hv, c["q"])
    total = float(P.abs_sum(hv).max()) + c["extra"]
    assert total < 2.0 ** 24 * c["q"]
    f16, ca, cb = c["raw"]
    if variant in ("b", "c"):                                               # one term alone, and the output's f16 planes hold it exactly
        assert total < 2.0 ** 11 * c["q"] and (c["bias"] is None or float(c["bias"].abs().max()) == 0)
        assert not c["relu"]
        assert float(f16.abs().max()) == 0 and float((cb if variant == "b" else ca).abs().max()) == 0
        assert float((ca if variant == "b" else cb).abs().max()) > 0
        assert torch.equal(P.f16_round(c["three"].float()), c["three"])
    if variant == "a":
        assert float(ca.abs().max()) == 0 and float(cb.abs().max()) == 0
    if variant == "d":
        assert min(float(t.abs().max()) for t in (f16, ca, cb)) > 0
    if kind in ("u", "uh"):
        assert c["wc_exact"] and c["bias_exact"]
    if kind == "f1":
        assert c["xe11_exact"]
        hi = P.f16_round(c["xe11"].float())
        assert float((c["xe11"] - hi).abs().max()) > 0                     # the computed first layer carries residuals
    if kind not in ("h", "uh"):                                             # the scale byte is hashed on its own: at least two values per tensor
        es = [P.q_fields(c[key])[3] for key in ("x1", "x2", "xl", "xs") if c.get(key) is not None]
        assert all(e.unique().numel() >= 2 for e in es if e.numel() > 1)    # (K1u's 1 x 1 low tensor of one chunk has ONE scale byte)
        assert torch.cat([e.reshape(-1) for e in es]).unique().numel() >= 2


@pytest.mark.parametrize("variant", ["a", "d"])
def test_crafted_weights_decompose_into_the_intended_parts(variant):
    for shape in [(64, 16, 3, 3), (128, 80, 3, 3)]:
        w = C.crafted_weights(shape, 3, variant)
        p = P.weight_parts(w)
        k = (w.double() - p.hi) / C.Q
        assert set(p.hi.unique().tolist()) <= set(C.W_HI) and set(k.unique().tolist()) <= ({0.0} if variant == "a" else set(map(float, C.W_K)))
        assert torch.equal(p.hi + p.res, w.double()) and torch.equal(p.copy, p.hi)       # nothing of the weight is lost in its fp4 parts
        assert variant == "a" or float(p.res.abs().max()) > 0
    # K1u: corner patterns keep their residuals in the class weights, dense patterns are sums of up to four taps
    w3, wt, bt, b3 = C.crafted_up_weights(32, 16, 16, 64, 7, "d")
    wc = P.combined_weights(w3, wt, 16)
    assert torch.equal(wc.float().double(), wc) and float(wc[:, 16:].abs().max()) == 0
    p = P.class_weight_parts(wc.float())
    assert float(p.res.abs().max()) > 0 and float(wc.abs().max()) > 0.1875
    assert not torch.equal(wc[:, :, :, 0], wc[:, :, :, 1])                  # the column-parity classes differ


# ---- rejection of wrong restatements ---------------------------------------------------------------------------------------------------------
def _value(c, wa=1.0, wb=1.0, **mutant):
    f16, (ca, cb) = C.results(c, **mutant)
    return C.finish(c, f16 + wa * ca + wb * cb)


def _rejected_a(c, wrong) -> bool:
    """family A: a kernel computing `wrong` fails the bit-for-bit comparison against the restatement of case c"""
    return not P.q_equal(P.q_encode(wrong.float()), c["three"])


TERM_MUTANTS = [("drop res_w*copy_x", 0.0, 1.0, "b"), ("drop copy_w*res_x", 1.0, 0.0, "c"), ("double res_w*copy_x", 2.0, 1.0, "b"),
                ("double copy_w*res_x", 1.0, 2.0, "c"), ("halve res_w*copy_x", 0.5, 1.0, "b"), ("halve copy_w*res_x", 1.0, 0.5, "c")]
SMALL = {"q": (1, 3, 5, 64, 0, 64), "u": (1, 2, 3, 48, 16, 32, 64)}


@pytest.mark.parametrize("kind", ["q", "u"])
@pytest.mark.parametrize("name,wa,wb,iso", TERM_MUTANTS, ids=[m[0] for m in TERM_MUTANTS])
def test_family_a_rejects_wrong_cross_terms(kind, name, wa, wb, iso):
    for variant in (iso, "d"):
        c = C.case(kind, SMALL[kind], variant)
        wrong = _value(c, wa, wb)
        assert _rejected_a(c, wrong), (name, variant)
        if variant == "d":
            assert float((wrong != c["three"]).float().mean()) > 0.4          # (ReLU zeroes about half of the outputs)
    if kind == "q":                                                         # the fused first layer's conv and the head's logit
        c = C.case("f1", C.F1_SHAPES[1], "d")
        assert _rejected_a(c, _value(c, wa, wb))
        c = C.case("q", C.Q_HEAD, "d")
        assert not P.exact_equal(_value(c, wa, wb)[:, [17]].float(), c["three"][:, [17]]) and not P.a_equal(P.a_encode(_value(c, wa, wb).float()), c["three"])


@pytest.mark.parametrize("kind", ["q", "u"])
def test_family_a_rejects_scale_bytes_of_the_neighbour(kind):
    for variant in ("b", "c", "d"):
        c = C.case(kind, SMALL[kind], variant)
        assert _rejected_a(c, _value(c, neighbour_scale=True)), variant


def test_family_a_rejects_wrong_padding_swapped_classes_and_swapped_halves():
    c = C.case("q", (1, 3, 5, 64, 0, 64), "d")
    wrong = _value(c, wrong_pad=True)
    assert _rejected_a(c, wrong)
    m = P.ring(3, 5)
    assert torch.equal(wrong[..., ~m], c["three"][..., ~m])                 # only border outputs change: hence the ring ratio of family B
    c = C.case("u", (1, 9, 17, 32, 32, 16, 128), "d")
    wrong = _value(c, wrong_pad=True)
    assert _rejected_a(c, wrong)
    m = P.ring(18, 34)
    assert torch.equal(wrong[..., ~m], c["three"][..., ~m])
    for shape in C.U_SHAPES:
        c = C.case("u", shape, "d")
        assert _rejected_a(c, _value(c, swap_px=True)), shape
    c = C.case("q", (1, 4, 6, 32, 48, 128), "d")
    assert _rejected_a(c, _value(c, swap_concat=True))


@pytest.mark.parametrize("kind,shape", [("q", s) for s in C.Q_SHAPES] + [("u", s) for s in C.U_SHAPES] + [("f1", s) for s in C.F1_SHAPES], ids=_id)
def test_family_a_rejects_a_truncated_residual_nibble(kind, shape):
    c = C.case(kind, shape, "d")
    got = P.q_encode(c["three"].float(), truncate_residual=True)
    bad = P.q_mismatch(got, c["three"])
    assert bad is not None and bad[0] == "residual nibbles", bad


def _b_ratios(c, wrong):
    """family B as the GPU test takes it: through the Q encoding, over all pixels and over the border ring"""
    thru = lambda v: P.q_decode(P.q_encode(v.float()))
    t, f, g = thru(c["three"]), thru(c["f16"]), thru(wrong) if not isinstance(wrong, P.QT) else P.q_decode(wrong)
    out = []
    for sel in (slice(None), P.ring(*t.shape[2:])):
        e1 = P.rel_l2(f[..., sel], t[..., sel])
        out.append((e1, P.ratio(g[..., sel], t[..., sel], e1), P.ratio_ok(g[..., sel], t[..., sel], e1)))
    return out


@pytest.mark.parametrize("kind", ["q", "u"])
def test_family_b_separates_the_arithmetic_from_its_mutants(kind):
    """Every wrong restatement of the arithmetic fails the ratio on BOTH shapes of the kernel.  A truncated residual nibble of the output is an
    error of the store encoding, not of the arithmetic: through the Q encoding it sits AT the bound (0.248 .. 0.260 of E1 here) and fails the
    ratio on at least one shape per kernel; what holds the rounding of that nibble is family A, bit for bit on every case."""
    truncated = []
    for shape in C.B_SHAPES[kind]:
        c = C.case(kind, shape, "B")
        assert C.e1(c) >= P.E1_MIN
        noise = 1.0 + 1e-7 * torch.randn(c["three"].shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        good = _b_ratios(c, c["three"] * noise)                              # the correct result with accumulation noise passes, with room
        print(f"q4 host: {kind} {shape} E1={good[0][0]:.3e} noise ratio all={good[0][1]:.4f} ring={good[1][1]:.4f}")
        assert all(ok for _, _, ok in good) and max(r for _, r, _ in good) < 0.05
        mutants = {name: _value(c, wa, wb) for name, wa, wb, _ in TERM_MUTANTS}
        mutants["f16 only"] = c["f16"]
        mutants["neighbour scale"] = _value(c, neighbour_scale=True)
        mutants["wrong padding"] = _value(c, wrong_pad=True)
        if kind == "u":
            mutants["swapped column classes"] = _value(c, swap_px=True)
        if kind == "q" and shape[4]:
            mutants["swapped concat halves"] = _value(c, swap_concat=True)
        for name, wrong in mutants.items():
            rs = _b_ratios(c, wrong)
            print(f"q4 host: {kind} {shape} {name}: ratio all={rs[0][1]:.4f} ring={rs[1][1]:.4f}")
            assert not all(ok for _, _, ok in rs), (name, rs)
            if name != "wrong padding":
                assert not rs[0][2], (name, rs)                             # ... over all pixels already; the wrong padding needs the ring
        rs = _b_ratios(c, P.q_encode(c["three"].float(), truncate_residual=True))
        print(f"q4 host: {kind} {shape} truncated residual nibble: ratio all={rs[0][1]:.4f} ring={rs[1][1]:.4f}")
        assert min(r for _, r, _ in rs) > 0.24
        truncated.append(not all(ok for _, _, ok in rs))
    assert any(truncated)
