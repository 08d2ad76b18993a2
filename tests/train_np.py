"""float64 numpy references of the train step's kernels (csrc/train.hip): loss and its gradient, AdamW, the power-of-two
gradient scale.  TEST INFRASTRUCTURE ONLY, no GPU.  Built on oracle/np_ops.py where that fits."""
import math

import numpy as np

from oracle import np_ops

F32 = np.float32


def ulp32(x):
    """Spacing of float32 at |x| (array or scalar), as float64."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def loss_terms(out, covers, inputs, use_l1):
    """Per-element summands of the two reductions of loss_reduce_kernel, in the float32 operation sequence the kernel documents, as
    float64 arrays: (|cov - out| or (cov - out)^2, wgt * s * (in255 - out255)), plus s = in255 - flip(in255)."""
    out, covers, inputs = (np.asarray(a, dtype=F32) for a in (out, covers, inputs))
    per = out.size // out.shape[0]
    d = covers - out                                              # float32
    a = d * d if use_l1 == 2 else np.abs(d)                       # float32 (the square rounds once)
    wgt = F32(1.0) / F32(per)
    in255 = inputs * F32(255.0)
    out255 = out * F32(255.0)
    s = in255 - np_ops.lsb_flip_from_unit(inputs)                 # float32, +-1 up to the rounding of in255
    b = (wgt * s) * (in255 - out255)                              # float32: wgt * s is exact for s = +-1, one rounding in the product
    return a.astype(np.float64), b.astype(np.float64), s.astype(np.float64)


def loss_ref(out, covers, inputs, alphas, use_l1, use_ws):
    """wsu_l1ws_loss_fwd_bwd in float64: (loss, parts[l1, ws], beta_hat[n], coef[n], dout).  use_l1: 0 none, 1 L1, 2 L2 (mean d^2,
    gradient -2 d / total).  The summands are the kernel's float32 ones (loss_terms), summed in float64; everything after the sums
    is float64, so what is left between this and the kernel is the order of a float64 sum and the kernel's final float32 casts.
    parts holds both terms whatever the switches say, like the kernel's loss_parts."""
    out = np.asarray(out, dtype=F32)
    n = out.shape[0]
    total = out.size
    per = total // n
    a, b, s = loss_terms(out, covers, inputs, use_l1)
    axes = tuple(range(1, out.ndim))
    l1 = float(a.sum(dtype=np.float64)) / total
    beta = b.sum(axis=axes, dtype=np.float64)
    pos = beta > 0.0
    beta_hat = np.where(pos, beta, 0.0)
    e = beta_hat - np.asarray(alphas, dtype=F32).astype(np.float64) / 2.0
    ws = float(np.mean(np.abs(e)))
    coef = np.sign(e) * pos / n
    dout = np.zeros(out.shape, dtype=np.float64)
    if use_l1 == 1:
        dout += np_ops.l1ws_loss(out, np.asarray(covers, dtype=F32), alphas, inputs, use_l1=True, use_ws=False)[1]
    elif use_l1 == 2:
        dout += -2.0 * (np.asarray(covers, dtype=F32) - out).astype(np.float64) / total
    if use_ws:
        dout += coef.reshape((n,) + (1,) * (out.ndim - 1)) * (-255.0 / per) * s
    loss = (l1 if use_l1 else 0.0) + (ws if use_ws else 0.0)
    return loss, np.array([l1, ws]), beta_hat, coef, dout


def adamw_ref(p, g, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, grad_scale=1.0):
    """wsu_adamw_multi_tensor on one tensor: np_ops.adamw_step on g * grad_scale, float64 math on float32 state, float64 p, m, v."""
    g = np.asarray(g, dtype=F32).astype(np.float64) * grad_scale
    return np_ops.adamw_step(np.asarray(p, dtype=F32), g, np.asarray(m, dtype=F32), np.asarray(v, dtype=F32), step,
                             lr=lr, b1=betas[0], b2=betas[1], eps=eps, wd=wd, out_dtype=np.float64)


def pow2_scale_ref(max_abs):
    """Exact scale of wsu_pow2_grad_scale: for m in (2^(k-1), 2^k] the scale is 2^(2-k), so m * scale lies in (2, 4].
    m < 1e-30 or NaN counts as 1e-30 and m > 1e30 as 1e30 (the clamps of pow2_scale_kernel)."""
    m = float(max_abs)
    if not m >= 1e-30:
        m = 1e-30
    if m > 1e30:
        m = 1e30
    f, e = math.frexp(m)                                          # m = f * 2^e, f in [0.5, 1)
    k = e - 1 if f == 0.5 else e
    return math.ldexp(1.0, 2 - k)
