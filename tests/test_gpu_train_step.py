"""The train step's kernels (csrc/train.hip) one by one against the float64 references of tests/train_np.py, at their edges: the
loss and its gradient, multi-tensor AdamW, the non-finite guard, the power-of-two gradient scale and the scale kernel.  Every test
calls ops.* directly -- no model, no Trainer.  The case tables and input builders at the top are plain numpy, so
tests/test_train_step_host.py checks them without a GPU.  Measured figures: profiles/r17/train_step_kernels.md."""
import functools
import math

import numpy as np
import pytest
import torch

from gpu_util import DEV
from ws_unet_amd import formula, ops, _lib
import train_np
from train_np import ulp32

pytestmark = pytest.mark.gpu

F32 = np.float32


def hp32(x):
    """The C entries take float arguments: the operation under test runs at the float32-rounded hyper-parameter, and so does its reference."""
    return float(F32(x))


# ---- loss: cases and inputs -------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(1, 1, 1, 1), (2, 1, 7, 9), (3, 3, 7, 9), (4, 1, 32, 32), (2, 1, 25, 41), (67, 1, 8, 8)]
LOSS_LARGE = (1, 1, 4099, 4099)                 # 16 801 801 elements > 65536 * 256: loss_grad_kernel's grid-stride loop repeats
LOSS_MODES = [(1, 1), (1, 0), (0, 1), (2, 1)]   # (use_l1, use_ws)
LOSS_T = (0.2, -0.3, 0.05)                      # beta_hat_n ~ t_n, rotating with n
LOSS_ALPHA = (0.2, 0.0, 0.8)                    # rotating with n + n // 3: all nine (t, alpha) pairs within nine images


def loss_inputs(shape):
    """(out, covers, inputs, alphas, rows, on_branch) as float32 numpy.  inputs = hashed uint8 / 255; out255 = in255 - t_n * s + noise with
    s = in255 - flip(in255) = +-1, so beta_hat_n ~ t_n; covers = inputs with hashed LSB flips.  Row rows[n] of image n has out == covers
    bit for bit (and covers = the flipped input there, which keeps beta_hat away from 0 even in a one-row image).  on_branch[n]: image n
    is built to sit on a branch (t_n < 0 and alpha_n = 0: relu gives 0, e is exactly 0)."""
    n, c, h, w = shape
    total = n * c * h * w
    key = formula.fnv1a64(f"train_step/loss/{shape}")
    hsh = formula.hash_u64(key, total)
    u8 = (hsh >> np.uint64(56)).astype(np.uint8).reshape(shape)
    flip = (((hsh >> np.uint64(40)) & np.uint64(0xFF)) < np.uint64(77)).reshape(shape)
    cov_u8 = u8 ^ flip.astype(np.uint8)
    rows = np.arange(n) % h
    for i in range(n):
        cov_u8[i, :, rows[i], :] = u8[i, :, rows[i], :] ^ 1
    inputs = u8.astype(F32) / F32(255.0)
    covers = cov_u8.astype(F32) / F32(255.0)
    t = np.array([LOSS_T[i % 3] for i in range(n)])
    alphas = np.array([LOSS_ALPHA[(i + i // 3) % 3] for i in range(n)], dtype=F32)
    s = u8.astype(np.float64) - (u8 ^ 1).astype(np.float64)
    noise = 0.01 * formula.uniform_pm1(key + 1, total).reshape(shape)
    out255 = u8.astype(np.float64) - t[:, None, None, None] * s + noise
    out = (out255 / 255.0).astype(F32)
    for i in range(n):
        out[i, :, rows[i], :] = covers[i, :, rows[i], :]
    on_branch = (t < 0) & (alphas == 0)
    return out, covers, inputs, alphas, rows, on_branch


# ---- AdamW: cases and inputs ------------------------------------------------------------------------------------------------------------
ADAMW_LENGTHS = (1, 5, 1023, 1024, 1025, 4096, 70001)
ADAMW_GAPS = (3, 0, 17, 5, 0, 29, 1)            # sentinel floats between two tensors beyond the 64 + 64: pointers are no fixed stride apart
SENTINEL = -7.25
# steps: the 1-based update counts run in sequence.  warm: non-zero m and v before the first call.  pins: the single terms whose loss moves p by
# more than 100x the case's tolerance (tests/test_train_step_host.py checks that, and that the five terms are all pinned by some case):
#   (a) defaults: lr * wd = 1e-6 is 8..16 ulp of p, too close to the rounding of p itself; the bias corrections are far above it
#   (c) at step 1000 both bias corrections are 1 to within 5e-5; the case is there for pow(beta, step) and the warm state
#   eps is visible only where it dominates the denominator (d), grad_scale only where it differs from 1 on a warm state (e)
ADAMW_CASES = {
    "a": dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, grad_scale=1.0, steps=(1, 2, 3, 4, 5), warm=False, p_lo=0.0, p_hi=0.05, g_mag=1e-2,
              pins=("bc1", "bc2")),
    "b": dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6, wd=0.1, grad_scale=1.0, steps=(1, 2, 3, 4, 5), warm=False, p_lo=0.5, p_hi=1.5, g_mag=1e-2,
              pins=("wd", "bc1", "bc2")),
    "c": dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6, wd=0.1, grad_scale=1.0, steps=(1000,), warm=True, p_lo=0.5, p_hi=1.5, g_mag=1e-2,
              pins=("wd",)),
    "d": dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6, wd=0.1, grad_scale=1.0, steps=(1, 2, 3), warm=False, p_lo=0.5, p_hi=1.5, g_mag=1e-7,
              pins=("wd", "eps", "bc1")),
    "e": dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6, wd=0.1, grad_scale=0.25, steps=(3, 4), warm=True, p_lo=0.5, p_hi=1.5, g_mag=1e-2,
              pins=("wd", "grad_scale", "bc1", "bc2")),
}
# The bound, in float32 ulps, from the operation count of adamw_kernel (each float32 operation rounds by at most half an ulp of its result,
# which is at most 2^-24 of it; ulp32(x) > 2^-24 x).  With S = |b1 m0| + |(1 - b1) g'|, g' = g * grad_scale (exact for a power of two),
# 1 - b1 and 1 - b2 exact (Sterbenz):
#   m: b1 * m0, (1 - b1) * g', their sum                                               3 roundings   <= 1.5 ulp32(S)           KM = 2
#   v: b2 * v0, (1 - b2) * g' (carried through the next product: 1 ulp), * g', the sum  4 roundings   <= 2.5 ulp32(v)           KV = 3
#   p: 1 - lr * wd (2^-25 absolute), p * that, the final subtraction                   3 roundings   <= 1.5 ulp32(max|p|)      KP = 2
#   update (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps), relative to (lr / bc1) * S / denom, in units of 2^-24:
#      v 3, halved by sqrtf 1.5, sqrtf 1, float32 sqrt(bc2) 1, the division 1, + eps 1      -> denom 5.5
#      m 3, m / denom 1, float32 bc1 1, lr / bc1 1, the product 1                           -> 12.5                              KU = 13
# ADAMW_K holds what the tests assert: the smallest integers not below what an MI355X run measured, none above the derived ones.  Measured
# over the five cases (profiles/r17/train_step_kernels.md): p 1.71 in units of ulp32(max |p|) + ulp32(update), m 1.24 ulp32(S), v 1.82 ulp32(v).
ADAMW_K_DERIVED = dict(KP=2, KU=13, KM=2, KV=3)
ADAMW_K = dict(KP=2, KU=2, KM=2, KV=2)


def adamw_hp(case):
    c = ADAMW_CASES[case]
    return dict(lr=hp32(c["lr"]), betas=(hp32(c["betas"][0]), hp32(c["betas"][1])), eps=hp32(c["eps"]), wd=hp32(c["wd"]),
                grad_scale=hp32(c["grad_scale"]))


def adamw_state(case, length):
    """Start state (p, m, v) of one tensor, float32 numpy.  |p| in [p_lo, p_hi] with a hashed sign."""
    c = ADAMW_CASES[case]
    u = formula.formula_tensor(f"train_step/adamw/{case}/p/{length}", (length,), 1.0).astype(np.float64)
    p = (np.sign(u) * (c["p_lo"] + (c["p_hi"] - c["p_lo"]) * np.abs(u))).astype(F32)
    if c["warm"]:
        m = formula.formula_tensor(f"train_step/adamw/{case}/m/{length}", (length,), 0.5 * c["g_mag"])
        v = (formula.formula_tensor(f"train_step/adamw/{case}/v/{length}", (length,), c["g_mag"]).astype(np.float64) ** 2
             + (0.1 * c["g_mag"]) ** 2).astype(F32)
    else:
        m, v = np.zeros(length, F32), np.zeros(length, F32)
    return p, m, v


def adamw_grad(case, length, step):
    return formula.formula_tensor(f"train_step/adamw/{case}/g{step}/{length}", (length,), ADAMW_CASES[case]["g_mag"])


def adamw_units(p0, g, m0, v0, step, hp, ref=None):
    """The four float32 ulps the bound is stated in, per element, for one update from the float32 state (p0, m0, v0):
    ulp32(max |p|), ulp32 of the cancellation-free update (lr / bc1) * S / denom, ulp32(S), ulp32(v) -- see the derivation at ADAMW_K."""
    b1, b2 = hp["betas"]
    p_ref, _, v_ref = ref if ref is not None else train_np.adamw_ref(p0, g, m0, v0, step, **hp)
    g64 = g.astype(np.float64) * hp["grad_scale"]
    s_m = np.abs(b1 * m0.astype(np.float64)) + np.abs((1.0 - b1) * g64)
    denom = np.sqrt(v_ref) / math.sqrt(1.0 - b2 ** step) + hp["eps"]
    upd = hp["lr"] / (1.0 - b1 ** step) * s_m / denom
    return ulp32(np.maximum(np.abs(p0), np.abs(p_ref))), ulp32(upd), ulp32(s_m), ulp32(v_ref)


def adamw_tolerance(p0, g, m0, v0, step, hp, ref=None, k=None):
    """(tol_p, tol_m, tol_v) per element."""
    k = k or ADAMW_K
    u_p, u_upd, u_m, u_v = adamw_units(p0, g, m0, v0, step, hp, ref)
    return k["KP"] * u_p + k["KU"] * u_upd, k["KM"] * u_m, k["KV"] * u_v


def adamw_f32(p, g, m, v, step, hp):
    """adamw_kernel's float32 operation sequence in numpy (informative: the report says whether the device matched it bit for bit)."""
    f = F32
    lr, b1, b2, eps, wd, gs = f(hp["lr"]), f(hp["betas"][0]), f(hp["betas"][1]), f(hp["eps"]), f(hp["wd"]), f(hp["grad_scale"])
    bc1 = f(1.0 - float(b1) ** step)
    bc2s = f(math.sqrt(1.0 - float(b2) ** step))
    g = g * gs
    p = p * (f(1.0) - lr * wd)
    m = b1 * m + (f(1.0) - b1) * g
    v = b2 * v + (f(1.0) - b2) * g * g
    p = p - (lr / bc1) * (m / (np.sqrt(v) / bc2s + eps))
    return p, m, v


# ---- non-finite guard and power-of-two scale: cases -----------------------------------------------------------------------------------------
NONFINITE_LENGTHS = (1, 255, 256, 257, 1024 * 256 + 3)
POW2_J = (-20, -3, 0, 1, 7, 20)
POW2_D = (-2.0 ** -24, 0.0, 2.0 ** -23)
POW2_MAXIMA = [float(F32(sign * 2.0 ** j * (1.0 + d))) for j in POW2_J for d in POW2_D for sign in (1.0, -1.0)]
POW2_TAIL_LEN = 2048 * 256 + 7


# =============================================================================================================================================
# loss
# =============================================================================================================================================

def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _loss_case(shape):
    """Inputs (host and device) and the device results of every mode of one shape, computed once and shared by the tests below."""
    out, covers, inputs, alphas, rows, on_branch = loss_inputs(shape)
    dev = tuple(_dev(a) for a in (out, covers, inputs, alphas))
    modes = [(1, 1)] if shape == LOSS_LARGE else LOSS_MODES
    if shape == LOSS_LARGE:
        # ops allocates dout itself: leave it a block that holds NaN, so that an element the kernel skipped cannot look right by accident
        poison = torch.full(shape, float("nan"), device=DEV)
        del poison
    got = {}
    for mode in modes:
        loss, dout, parts, beta = ops.l1ws_loss_fwd_bwd(*dev, use_l1=mode[0], use_ws=bool(mode[1]))
        got[mode] = (loss.item(), dout, parts.cpu().numpy().astype(np.float64), beta.cpu().numpy().astype(np.float64))
    return dict(host=(out, covers, inputs, alphas), dev=dev, rows=rows, on_branch=on_branch, got=got)


def _loss_params():
    return [pytest.param(s, m, id=f"{'x'.join(map(str, s))}-l1_{m[0]}-ws_{m[1]}") for s in LOSS_SHAPES for m in LOSS_MODES] + \
           [pytest.param(LOSS_LARGE, (1, 1), id="1x1x4099x4099-l1_1-ws_1")]


@pytest.mark.parametrize("shape,mode", _loss_params())
def test_loss_values_and_gradient(shape, mode):
    """loss, parts, beta_hat and dout of wsu_l1ws_loss_fwd_bwd against train_np.loss_ref.

    Bound of a value: the kernel sums the same float32 summands as the reference in float64 and casts the result to float32 once, which
    is half a float32 ulp; a float64 sum of k terms in another order differs by at most k * 2^-53 * sum |terms|, where k is
    ceil(per_image / 1024) + 10 for the kernel's strided-then-tree order and at most that for numpy's pairwise sum, and n more terms join
    the per-image sums.  The assertion allows 1 ulp32(|ref|) -- the cast, and the reference lying just over a binade from the result --
    plus 2 (k + n) 2^-53 sum |terms|.  Measured on an MI355X: worst |got - ref| / bound = 0.50 (profiles/r17/train_step_kernels.md).
    Bound of dout: 4 float32 ulp of max(1 / total, 255 * wgt / n); a flipped sign is 2 / total away."""
    use_l1, use_ws = mode
    case = _loss_case(shape)
    out, covers, inputs, alphas = case["host"]
    n = shape[0]
    total = out.size
    per = total // n
    loss, parts, beta_hat, coef, dout = train_np.loss_ref(out, covers, inputs, alphas, use_l1, use_ws)
    g_loss, g_dout, g_parts, g_beta = case["got"][mode]
    a, b, _ = train_np.loss_terms(out, covers, inputs, use_l1)
    k = 2.0 * (math.ceil(per / 1024) + 10 + n) * 2.0 ** -53
    order_l1 = k * float(a.sum()) / total
    order_beta = k * np.abs(b).reshape(n, -1).sum(axis=1)
    order_ws = float(order_beta.mean())
    checks = [("loss", g_loss, loss, order_l1 * bool(use_l1) + order_ws * bool(use_ws)),
              ("parts[l1]", g_parts[0], parts[0], order_l1), ("parts[ws]", g_parts[1], parts[1], order_ws)]
    checks += [(f"beta_hat[{i}]", g_beta[i], beta_hat[i], order_beta[i]) for i in range(n)]
    worst = 0.0
    for what, got, ref, order in checks:
        bound = float(ulp32(ref)) + order if ref != 0.0 else 0.0
        err = abs(float(got) - float(ref))
        worst = max(worst, err / bound if bound else (0.0 if err == 0.0 else math.inf))
    g_dout_h = g_dout.cpu().numpy().astype(np.float64)
    scale = max(1.0 / total, 255.0 / per / n) if use_ws else 1.0 / total
    tol_d = 4.0 * float(ulp32(scale))
    err_d = float(np.abs(g_dout_h - dout).max())
    print(f"[loss {shape} l1={use_l1} ws={use_ws}] values: worst |got - ref| / bound = {worst:.3f};  dout: max err {err_d:.3e} = "
          f"{err_d / float(ulp32(scale)):.3f} ulp32({scale:.3e}) (bound 4)")
    for what, got, ref, order in checks:
        bound = float(ulp32(ref)) + order if ref != 0.0 else 0.0
        assert abs(float(got) - float(ref)) <= bound, f"{what}: got {got!r}, reference {ref!r}, bound {bound:.3e}"
    assert err_d <= tol_d, f"dout: max err {err_d:.3e} > {tol_d:.3e}"
    # branches: relu'(beta <= 0) = 0 and sign(0) = 0 give exact zeros, not small numbers
    assert np.all(g_beta[beta_hat == 0.0] == 0.0)
    if use_ws and not use_l1:
        assert np.all(g_dout_h[coef == 0.0] == 0.0), "an image with coef == 0 has a WS gradient"
    if use_l1 and not use_ws:
        for i, r in enumerate(case["rows"]):
            row = g_dout_h[i, :, r, :]
            assert np.all(row == 0.0) and not np.signbit(row).any(), "out == covers must give a gradient of exactly 0.0"


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_gradient_parts_are_separate(shape):
    """With both terms on: where out == covers the gradient is the WS part alone, in an image with coef == 0 it is the L1 part alone --
    bitwise what the runs with one term give."""
    case = _loss_case(shape)
    both, l1_only, ws_only = (case["got"][m][1] for m in ((1, 1), (1, 0), (0, 1)))
    *_, coef, _ = train_np.loss_ref(*case["host"], 1, 1)
    for i, r in enumerate(case["rows"]):
        assert torch.equal(both[i, :, r, :], ws_only[i, :, r, :])
        if coef[i] == 0.0:
            assert torch.equal(both[i], l1_only[i]) and not ws_only[i].any()
    assert any(coef == 0.0) or shape[0] == 1
    if case["on_branch"].any():
        assert np.all(coef[case["on_branch"]] == 0.0)


@pytest.mark.parametrize("shape", [(3, 3, 7, 9), (2, 1, 25, 41), LOSS_LARGE], ids=lambda s: "x".join(map(str, s)))
def test_loss_repeat_is_bitwise_equal(shape):
    case = _loss_case(shape)
    loss, dout, parts, beta = ops.l1ws_loss_fwd_bwd(*case["dev"], use_l1=1, use_ws=True)
    g_loss, g_dout, g_parts, g_beta = case["got"][(1, 1)]
    assert loss.item() == g_loss and torch.equal(dout, g_dout)
    assert np.array_equal(parts.cpu().numpy(), g_parts.astype(F32)) and np.array_equal(beta.cpu().numpy(), g_beta.astype(F32))


def test_loss_without_optional_outputs():
    """ops always passes loss_parts and beta_hat; the C entry takes them as optional.  Without them: the same loss and dout."""
    shape = (3, 3, 7, 9)
    case = _loss_case(shape)
    out, covers, inputs, alphas = case["dev"]
    lib = _lib.load()
    n, per = shape[0], out.numel() // shape[0]
    loss = torch.full((), float("nan"), device=DEV)
    dout = torch.full_like(out, float("nan"))
    ws = torch.empty((lib.wsu_l1ws_loss_workspace_bytes(n) + 7) // 8, dtype=torch.float64, device=DEV)
    rc = lib.wsu_l1ws_loss_fwd_bwd(out.data_ptr(), covers.data_ptr(), inputs.data_ptr(), alphas.data_ptr(), loss.data_ptr(), None,
                                   dout.data_ptr(), None, ws.data_ptr(), ws.numel() * 8, n, per, 1, 1, ops._stream())
    assert rc == 0
    g_loss, g_dout, _, _ = case["got"][(1, 1)]
    assert loss.item() == g_loss and torch.equal(dout, g_dout)


# =============================================================================================================================================
# AdamW
# =============================================================================================================================================

class _Buffers:
    """p, g, m, v of the seven tensors as slices of four larger device buffers: 64 sentinel floats on both sides of every tensor and unequal
    gaps, rotated per kind, so neither the tensors of one kind nor the four pointers of one tensor are a fixed stride apart."""

    def __init__(self, case, order):
        self.case, self.order = case, order
        self.bufs, self.inside, self.views = {}, {}, {}
        states = [adamw_state(case, n) for n in ADAMW_LENGTHS]
        idx = list(range(len(ADAMW_LENGTHS)))
        for ki, kind in enumerate("pgmv"):
            gaps = ADAMW_GAPS[ki:] + ADAMW_GAPS[:ki]
            if order == "flat":                                     # one tensor holding the concatenation
                starts, off = [64], 64 + sum(ADAMW_LENGTHS) + 64
            else:
                starts, off = [], 64
                for i in idx:
                    starts.append(off)
                    off += ADAMW_LENGTHS[i] + 64 + gaps[i]
            host = np.full(off, SENTINEL, F32)
            inside = np.zeros(off, bool)
            spans = [(starts[0], sum(ADAMW_LENGTHS))] if order == "flat" else [(starts[i], ADAMW_LENGTHS[i]) for i in idx]
            for s, n in spans:
                inside[s:s + n] = True
            if kind != "g":
                host[inside] = np.concatenate([st["pmv".index(kind)] for st in states])
            self.bufs[kind] = _dev(host)
            self.inside[kind] = inside
            self.views[kind] = [self.bufs[kind][s:s + n] for s, n in spans]
        views = [self.views[k] for k in "pgmv"]
        if order == "rev":
            views = [v[::-1] for v in views]
        self.table = ops.AdamWTable(*views)

    def set_grad(self, step, scale=1.0):
        g = np.concatenate([adamw_grad(self.case, n, step) for n in ADAMW_LENGTHS]) * F32(scale)
        host = np.full(self.inside["g"].size, SENTINEL, F32)
        host[self.inside["g"]] = g
        self.bufs["g"].copy_(torch.from_numpy(host))

    def read(self, kind):
        """The kind's tensors as one float32 array in ADAMW_LENGTHS order, after checking that no sentinel changed."""
        host = self.bufs[kind].cpu().numpy()
        assert np.all(host[~self.inside[kind]] == F32(SENTINEL)), f"a sentinel next to a {kind} tensor changed"
        return host[self.inside[kind]]


def _split(flat):
    return np.split(flat, np.cumsum(ADAMW_LENGTHS)[:-1])


@functools.lru_cache(maxsize=None)
def _adamw_run(case, order="fwd", premultiplied=False):
    """The case's sequence of updates on the device: a list, per step, of (before, g, after) with before / after = (p, m, v) flat float32."""
    c, hp = ADAMW_CASES[case], adamw_hp(case)
    buf = _Buffers(case, order)
    trace = []
    for step in c["steps"]:
        buf.set_grad(step, hp["grad_scale"] if premultiplied else 1.0)
        before = tuple(buf.read(k) for k in "pmv")
        buf.table.step(step, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["wd"],
                       grad_scale=1.0 if premultiplied else hp["grad_scale"])
        trace.append((before, buf.read("g"), tuple(buf.read(k) for k in "pmv")))
    return trace


@pytest.mark.parametrize("case", sorted(ADAMW_CASES))
def test_adamw_against_reference(case):
    """Every update of the case against train_np.adamw_ref fed the kernel's own float32 state of the step before: the errors are per
    step and do not accumulate.  One table over seven tensors; the bound is ADAMW_K; every sentinel stays (checked by each read)."""
    hp = adamw_hp(case)
    worst = dict(p=0.0, m=0.0, v=0.0, p_bound=0.0)
    exact = True
    for step, (before, g, after) in zip(ADAMW_CASES[case]["steps"], _adamw_run(case)):
        ref = train_np.adamw_ref(*((before[0], g) + before[1:]), step, **hp)
        u_p, u_upd, u_m, u_v = adamw_units(before[0], g, before[1], before[2], step, hp, ref)
        tols = adamw_tolerance(before[0], g, before[1], before[2], step, hp, ref)
        errs = [np.abs(got.astype(np.float64) - want) for got, want in zip(after, ref)]
        for name, err, unit in zip("pmv", errs, (u_p + u_upd, u_m, u_v)):
            worst[name] = max(worst[name], float((err / unit).max()))
        worst["p_bound"] = max(worst["p_bound"], float((errs[0] / tols[0]).max()))
        exact &= all(np.array_equal(got, r) for got, r in zip(after, adamw_f32(before[0], g, before[1], before[2], step, hp)))
    print(f"[adamw {case}] worst error: p {worst['p']:.3f} (ulp32(max |p|) + ulp32(update)) = {worst['p_bound']:.3f} of its bound, "
          f"m {worst['m']:.3f} ulp32(S), v {worst['v']:.3f} ulp32(v)  (asserted K = {ADAMW_K});  "
          f"bitwise equal to the float32 restatement: {exact}")
    for step, (before, g, after) in zip(ADAMW_CASES[case]["steps"], _adamw_run(case)):
        ref = train_np.adamw_ref(*((before[0], g) + before[1:]), step, **hp)
        tols = adamw_tolerance(before[0], g, before[1], before[2], step, hp, ref)
        for name, got, want, tol in zip("pmv", after, ref, tols):
            err = np.abs(got.astype(np.float64) - want)
            bad = np.flatnonzero(~(err <= tol))
            assert bad.size == 0, (f"case {case} step {step} {name}: {bad.size} elements off, first at flat index {bad[0]}: got {got[bad[0]]!r}, "
                                   f"reference {want[bad[0]]!r}, error {err[bad[0]]:.3e} > bound {tol[bad[0]]:.3e}")


@pytest.mark.parametrize("case", ["b", "e"])
@pytest.mark.parametrize("order", ["rev", "flat"])
def test_adamw_table_order_and_flat_tensor(case, order):
    """The table in reversed tensor order, and one flat tensor holding the concatenation, give bitwise the same per-tensor results."""
    for (_, _, want), (_, _, got) in zip(_adamw_run(case), _adamw_run(case, order)):
        for name, a, b in zip("pmv", want, got):
            assert np.array_equal(a, b), f"{name} differs between the table orders"


def test_adamw_grad_scale_equals_premultiplied_gradient():
    """Case (e), grad_scale = 0.25, equals bitwise a run on gradients multiplied by 0.25 beforehand (exact: a power of two)."""
    for (_, _, want), (_, g, got) in zip(_adamw_run("e"), _adamw_run("e", "fwd", True)):
        for name, a, b in zip("pmv", want, got):
            assert np.array_equal(a, b), name
    assert not np.array_equal(_adamw_run("e")[0][1], g)


def test_adamw_skip_flag():
    buf = _Buffers("b", "fwd")
    hp = adamw_hp("b")
    buf.set_grad(1)
    before = [buf.read(k) for k in "pmv"]
    kw = dict(lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["wd"])
    buf.table.step(1, skip_flag=torch.tensor([1, 0], dtype=torch.int32, device=DEV), **kw)
    for k, b in zip("pmv", before):
        assert np.array_equal(buf.read(k).view(np.uint32), b.view(np.uint32)), f"{k} changed under a set skip flag"
    buf.table.step(1, skip_flag=torch.tensor([0, 0], dtype=torch.int32, device=DEV), **kw)
    after = [buf.read(k) for k in "pmv"]
    for k, a, b in zip("pmv", after, before):
        assert np.all(a != b), f"{k}: some element did not change under a clear skip flag"
    for k, a, b in zip("pmv", after, _adamw_run("b")[0][2]):
        assert np.array_equal(a, b), k


def test_adamw_zero_gradient_on_fresh_state():
    """g = 0 everywhere with m = v = 0: m and v stay 0, p = p * (1 - lr * wd), and 0 / eps is no NaN."""
    hp = adamw_hp("b")
    buf = _Buffers("b", "fwd")
    buf.bufs["g"].copy_(torch.from_numpy(np.where(buf.inside["g"], F32(0.0), F32(SENTINEL))))
    p0 = buf.read("p")
    buf.table.step(1, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["wd"])
    p, m, v = (buf.read(k) for k in "pmv")
    assert not m.any() and not v.any()
    assert np.array_equal(p, p0 * (F32(1.0) - F32(hp["lr"]) * F32(hp["wd"])))
    want = p0.astype(np.float64) * (1.0 - hp["lr"] * hp["wd"])
    assert np.all(np.abs(p - want) <= ADAMW_K["KP"] * ulp32(p0))


# =============================================================================================================================================
# non-finite guard
# =============================================================================================================================================

def _flag():
    return torch.zeros(2, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("length", NONFINITE_LENGTHS)
def test_nonfinite_flag_every_poison_and_position(length):
    clean = formula.formula_tensor(f"train_step/nonfinite/{length}", (length,), 3.0)
    x = _dev(clean)
    flag = _flag()
    assert ops.nonfinite_flag(x, flag).tolist() == [0, 0]
    count = 0
    for poison in (float("inf"), float("-inf"), float("nan")):
        for pos in sorted({0, length // 2, length - 1}):
            x[pos] = poison
            count += 1
            assert ops.nonfinite_flag(x, flag).tolist() == [1, count], (poison, pos)
            x[pos] = float(clean[pos])
    assert ops.nonfinite_flag(x, flag).tolist() == [0, count]


@pytest.mark.parametrize("length", NONFINITE_LENGTHS)
def test_nonfinite_flag_passes_extreme_finite_values(length):
    """+-FLT_MAX, denormals and -0.0 are finite."""
    fmax = float(np.finfo(F32).max)
    vals = np.array([fmax, -fmax, 1e-45, -1e-45, 1.1754942e-38, -0.0, 0.0, 1.0], dtype=F32)
    x = np.resize(vals, length)
    x[-1] = -fmax if length > 1 else fmax
    flag = _flag()
    flag[0] = 1                                                   # the call has to reset it
    assert ops.nonfinite_flag(_dev(x), flag).tolist() == [0, 0]


def test_nonfinite_flag_counts_over_a_sequence():
    n = 1024 * 256 + 3
    clean = torch.ones(n, device=DEV)
    bad = clean.clone()
    bad[-1] = float("nan")
    flag = _flag()
    seen = [ops.nonfinite_flag(t, flag).tolist() for t in (clean, bad, bad, clean)]
    assert seen == [[0, 0], [1, 1], [1, 2], [0, 2]]


# =============================================================================================================================================
# power-of-two gradient scale, scale_by
# =============================================================================================================================================

def _check_pow2(x, m):
    s2 = ops.pow2_grad_scale(x).cpu().numpy()
    scale, inv = float(s2[0]), float(s2[1])
    want = train_np.pow2_scale_ref(abs(m))
    prod = abs(m) * scale                                          # exact in float64: a float32 times a power of two
    assert scale == want and scale * inv == 1.0 and 2.0 < prod <= 4.0, \
        f"max {m!r} = {abs(m).hex()}: scale {scale!r} (reference {want!r}), scale * inv = {scale * inv!r}, max * scale = {prod!r}"


@pytest.mark.parametrize("m", POW2_MAXIMA, ids=lambda m: float(m).hex())
def test_pow2_scale_at_binade_edges(m):
    """The maximum one float32 below, at and one above a power of two: scale == the exact reference, max * scale in (2, 4]."""
    x = formula.formula_tensor("train_step/pow2/head", (33 * 65,), 0.4 * abs(m))
    x[0] = m
    _check_pow2(_dev(x), m)


def test_pow2_scale_maximum_in_the_tail():
    """Every maximum of the table as the last element of a tensor longer than the 2048 * 256 threads of absmax_kernel; the rest is
    smaller noise."""
    unit = _dev(formula.formula_tensor("train_step/pow2/tail", (POW2_TAIL_LEN,), 0.4))
    for m in POW2_MAXIMA:
        x = unit * abs(m)
        x[-1] = m
        assert x[:-1].abs().max().item() < abs(m)
        _check_pow2(x, m)


@pytest.mark.parametrize("fill,clamped", [(0.0, 1e-30), (float("nan"), 1e-30), (float("inf"), 1e30), (float("-inf"), 1e30)])
def test_pow2_scale_clamps(fill, clamped):
    """All-zero, NaN-holding and inf-holding inputs give the finite powers of two of the kernel's clamps."""
    x = formula.formula_tensor("train_step/pow2/clamp", (33 * 65,), 1.0)
    if fill == 0.0:
        x[:] = 0.0
        x[1] = -0.0
    else:
        x[len(x) // 2] = fill
    s2 = ops.pow2_grad_scale(_dev(x)).cpu().numpy()
    want = train_np.pow2_scale_ref(clamped)
    assert float(s2[0]) == want and float(s2[0]) * float(s2[1]) == 1.0 and np.isfinite(s2).all()
    assert math.frexp(want)[0] == 0.5


def test_scale_by_aliasing_length_and_factors():
    n = 16384 * 256 + 5                                            # above the grid of scale_kernel: its loop repeats
    g = torch.Generator(device=DEV).manual_seed(17)
    x = torch.randn(n, device=DEV, generator=g)
    for f in (0.125, 0.3):
        factor = torch.tensor([f], device=DEV)
        want = x * factor[0]
        assert torch.equal(ops.scale_by(x, factor), want)
        y = x.clone()
        assert ops.scale_by(y, factor, out=y) is y and torch.equal(y, want)
    small = x[:5].clone()
    assert torch.equal(ops.scale_by(small, torch.tensor([0.3], device=DEV), out=small), x[:5] * 0.3)
