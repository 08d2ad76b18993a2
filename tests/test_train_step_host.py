"""CPU checks of the train-step references (tests/train_np.py) and of the case tables of tests/test_gpu_train_step.py: the references
reproduce the reference project's golden vectors, and the GPU tests' inputs can tell a wrong kernel from a right one."""
import math

import numpy as np
import pytest

from oracle import np_ops
import train_np
import test_gpu_train_step as cases
from test_oracle_golden import _loss_inputs

F32 = np.float32


# ---- the references themselves -----------------------------------------------------------------------------------------------------------

def test_loss_ref_reproduces_golden(golden):
    """All four losses of tests/golden/losses.npz at the tolerances test_oracle_golden.py uses for np_ops.l1ws_loss."""
    g = golden["losses"]
    covers, inputs, alphas = (t.numpy() for t in _loss_inputs())
    out = g["loss_outputs"]
    for i, (name, use_l1, use_ws) in enumerate([("l1", 1, 0), ("l2", 2, 0), ("ws", 0, 1), ("l1ws", 1, 1)]):
        loss, parts, beta_hat, coef, dout = train_np.loss_ref(out, covers, inputs, alphas, use_l1, use_ws)
        assert math.isclose(loss, float(g["loss_values"][i]), rel_tol=1e-5), name
        np.testing.assert_allclose(dout, g[f"loss_{name}_dout"], rtol=1e-4, atol=1e-9, err_msg=name)
    lv, grad = np_ops.l1ws_loss(out, covers, alphas, inputs)
    assert math.isclose(loss, lv, rel_tol=1e-6) and parts[0] + parts[1] == loss
    np.testing.assert_allclose(dout, grad, rtol=1e-12, atol=0)
    assert beta_hat.shape == coef.shape == (4,) and np.all((coef == 0) == (beta_hat == 0))


def test_adamw_ref_reproduces_np_ops():
    rng = np.random.default_rng(5)
    p, g, m = (rng.standard_normal(1000).astype(F32) for _ in range(3))
    v = (rng.standard_normal(1000) ** 2).astype(F32)
    for step, kw, gs in ((1, {}, 1.0), (7, dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6, wd=0.1), 0.25)):
        got = train_np.adamw_ref(p, g, m, v, step, grad_scale=gs, **kw)
        np_kw = {k: x for k, x in kw.items() if k != "betas"}
        if "betas" in kw:
            np_kw.update(b1=kw["betas"][0], b2=kw["betas"][1])
        want = np_ops.adamw_step(p, g.astype(np.float64) * gs, m, v, step, **np_kw)
        for a, b in zip(got, want):
            assert a.dtype == np.float64 and np.array_equal(a.astype(F32), b)


def test_pow2_scale_ref_known_values():
    assert train_np.pow2_scale_ref(1.0) == 4.0 and train_np.pow2_scale_ref(1.5) == 2.0 and train_np.pow2_scale_ref(2.0) == 2.0
    assert train_np.pow2_scale_ref(float(np.nextafter(F32(2.0), F32(3.0)))) == 1.0
    assert train_np.pow2_scale_ref(0.75) == 4.0 and train_np.pow2_scale_ref(0.5) == 8.0
    assert train_np.pow2_scale_ref(0.0) == train_np.pow2_scale_ref(float("nan")) == train_np.pow2_scale_ref(1e-30) == 2.0 ** 101
    assert train_np.pow2_scale_ref(float("inf")) == train_np.pow2_scale_ref(1e30) == 2.0 ** -98


# ---- input self-checks of the GPU tests ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cases.LOSS_SHAPES + [cases.LOSS_LARGE], ids=lambda s: "x".join(map(str, s)))
def test_loss_cases_stay_off_the_branches(shape):
    """|e_n| > 1e-3 and |beta_n| > 1e-3 in float64 for every image not built to sit on a branch: rounding can never pick the other
    branch of relu or of sign(e).  The images built for a branch sit on it exactly."""
    out, covers, inputs, alphas, rows, on_branch = cases.loss_inputs(shape)
    n = shape[0]
    _, b, _ = train_np.loss_terms(out, covers, inputs, 1)
    beta = b.reshape(n, -1).sum(axis=1)
    e = np.maximum(beta, 0.0) - alphas.astype(np.float64) / 2.0
    assert np.all(np.abs(beta) > 1e-3), beta
    assert np.all(np.abs(e[~on_branch]) > 1e-3), e
    assert np.all(e[on_branch] == 0.0) and np.all(beta[on_branch] < -1e-3)
    for i in range(n):
        assert np.array_equal(out[i, :, rows[i], :], covers[i, :, rows[i], :])
        mask = np.ones(out.shape[2], bool)
        mask[rows[i]] = False
        assert np.all(out[i][:, mask, :] != covers[i][:, mask, :])
    if n >= 3:                                                     # every sign of e, and an exact zero, within three images
        *_, coef, _ = train_np.loss_ref(out, covers, inputs, alphas, 1, 1)
        assert (coef > 0).any() and (coef < 0).any() and on_branch.any() and (beta < 0).any()


def _adamw_variant(p, g, m, v, step, lr, betas, eps, wd, grad_scale, bc1=None, bc2=None):
    """The update of p in float64, written out, with optional stand-ins for the two bias corrections."""
    b1, b2 = betas
    g = g.astype(np.float64) * grad_scale
    m = b1 * m.astype(np.float64) + (1.0 - b1) * g
    v = b2 * v.astype(np.float64) + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step if bc1 is None else bc1
    bc2 = 1.0 - b2 ** step if bc2 is None else bc2
    return p.astype(np.float64) * (1.0 - lr * wd) - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)


def _adamw_trajectory(case, length):
    """(step, p, g, m, v) before every update of the case, following the reference rounded to float32 after each step as the kernel's state is."""
    hp = cases.adamw_hp(case)
    p, m, v = cases.adamw_state(case, length)
    for step in cases.ADAMW_CASES[case]["steps"]:
        g = cases.adamw_grad(case, length, step)
        yield step, p, g, m, v
        p, m, v = (a.astype(F32) for a in train_np.adamw_ref(p, g, m, v, step, **hp))


DROPS = {"wd": dict(wd=0.0), "eps": dict(eps=0.0), "grad_scale": dict(grad_scale=1.0), "bc1": dict(bc1=1.0), "bc2": dict(bc2=1.0)}


@pytest.mark.parametrize("case", sorted(cases.ADAMW_CASES))
def test_adamw_cases_expose_a_dropped_term(case):
    """At every step of the case, for each term the case pins, dropping that single term moves the reference's p by more than 100x the
    asserted tolerance in at least nine elements of ten (the rest have a gradient or moment near zero): the tolerance cannot hide
    a missing term.  A term that the case's numbers cannot show is not in its pins; the table as a whole pins all five."""
    hp = cases.adamw_hp(case)
    for length in (1025, 70001):
        for step, p, g, m, v in _adamw_trajectory(case, length):
            ref = train_np.adamw_ref(p, g, m, v, step, **hp)
            np.testing.assert_allclose(_adamw_variant(p, g, m, v, step, **hp), ref[0], rtol=1e-14, atol=0)
            tol_p = cases.adamw_tolerance(p, g, m, v, step, hp, ref)[0]
            for term in cases.ADAMW_CASES[case]["pins"]:
                moved = np.abs(_adamw_variant(p, g, m, v, step, **{**hp, **DROPS[term]}) - ref[0])
                frac = float(np.mean(moved > 100.0 * tol_p))
                assert frac >= 0.9, f"case {case} step {step}: without {term} only {frac:.2%} of p moves by more than 100x the tolerance"


def test_adamw_cases_pin_every_term_and_bound_is_within_the_derived_one():
    assert set().union(*(c["pins"] for c in cases.ADAMW_CASES.values())) == set(DROPS)
    assert all(1 <= cases.ADAMW_K[k] <= cases.ADAMW_K_DERIVED[k] for k in cases.ADAMW_K_DERIVED)
    assert cases.ADAMW_CASES["e"]["grad_scale"] == 0.25 and cases.ADAMW_CASES["c"]["steps"] == (1000,)
    assert len(set(cases.ADAMW_GAPS)) > 2 and len(cases.ADAMW_GAPS) == len(cases.ADAMW_LENGTHS)


@pytest.mark.parametrize("case", sorted(cases.ADAMW_CASES))
def test_adamw_float32_restatement_is_within_the_bound(case):
    """The kernel's operation sequence in numpy float32 stays within the asserted bound of the float64 reference: the bound asks
    nothing that correct float32 arithmetic cannot give."""
    hp = cases.adamw_hp(case)
    for step, p, g, m, v in _adamw_trajectory(case, 70001):
        ref = train_np.adamw_ref(p, g, m, v, step, **hp)
        for got, want, tol in zip(cases.adamw_f32(p, g, m, v, step, hp), ref, cases.adamw_tolerance(p, g, m, v, step, hp, ref)):
            assert got.dtype == F32 and np.all(np.abs(got.astype(np.float64) - want) <= tol)


def test_pow2_table_products_lie_in_the_promised_interval():
    assert len(cases.POW2_MAXIMA) == 36 and len(set(cases.POW2_MAXIMA)) == 36
    for m in cases.POW2_MAXIMA:
        assert m != 0.0 and math.isfinite(m) and float(F32(m)) == m
        prod = abs(m) * train_np.pow2_scale_ref(abs(m))
        assert 2.0 < prod <= 4.0, (m, prod)
    # the table holds the maxima one float32 below, at and one above each power of two
    for j in cases.POW2_J:
        p = F32(2.0 ** j)
        assert {float(np.nextafter(p, F32(0))), float(p), float(np.nextafter(p, F32(np.inf)))} <= set(cases.POW2_MAXIMA)
