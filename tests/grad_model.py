"""numpy restatement of the gradient pass and of the clipped optimiser step (include/unet_hip.h:
unet_grad_accumulate_f32, unet_train_adam_step_rec; csrc/grad_kernels.cpp, csrc/train_kernels.h).

  accumulate(a, b)      dst = a + b, one fp32 addition per element; b None: a copy
  record(x)             [sum of x^2 over the finite elements, squares and sum in double; number of non-finite elements]
  record_bound(n)       the relative distance the kernel's record[0] may have from the exactly rounded sum
  coefficient(...)      grad_scale * min(1, max_norm / (|grad_scale| sqrt(record[0]) + 1e-6)), double, rounded once
  adam_step(...)        adam_kernel's update in fp32, one rounding per operation as written there

The kernel's sum is a sum of exact, non-negative doubles in SOME fixed order (per-thread partials, block trees, a final
tree); each of its at most n additions rounds once, relative 2^-53, and no term cancels, so any order is within
n * 2^-53, relative, of the exact sum.  `record` forms that exact sum with math.fsum and rounds it once."""
import math

import numpy as np


def accumulate(a, b=None):
    a = np.asarray(a, dtype=np.float32)
    if b is None:
        return a.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return (a + np.asarray(b, dtype=np.float32)).astype(np.float32)


def record(x):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    finite = np.isfinite(x)
    sq = x[finite].astype(np.float64) ** 2          # a 24-bit significand squared: exact in double
    return np.array([math.fsum(sq.tolist()), float(x.size - int(finite.sum()))], dtype=np.float64)


def record_fp32_sum(x):
    """what the record must NOT be: squares and running sum in fp32 (loses small terms, overflows at 1e30^2)"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    x = x[np.isfinite(x)]
    s = np.float32(0.0)
    with np.errstate(over="ignore"):
        for v in x:
            s = np.float32(s + np.float32(v * v))
    return float(s)


def record_bound(numel):
    return numel * 2.0 ** -53


def within_bound(got, x):
    """got: a record[0] for the buffer x"""
    want = record(x)[0]
    return abs(float(got) - want) <= record_bound(np.asarray(x).size) * want


def coefficient(grad_scale, max_norm, sumsq):
    """-> (coef as float32, scaled pre-clip norm as float64); max_norm None or inf: no clipping, coef == grad_scale"""
    gs = float(np.float32(grad_scale))
    mx = math.inf if max_norm is None else float(np.float32(max_norm))
    norm = abs(gs) * math.sqrt(float(sumsq))
    return np.float32(gs * min(1.0, mx / (norm + 1e-6))), norm


def adam_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, decoupled, coef):
    """One update of adam_kernel / adam_rec_kernel on fp32 arrays with the gradient multiplier `coef`; every operation
    rounds to fp32 (the device may fuse a multiply into the addition that follows: results agree within an fp32
    rounding or two per element, which is how tests use this).  Returns (p, m, v)."""
    f = np.float32
    p, g, m, v = (np.asarray(t, dtype=np.float32).copy() for t in (p, g, m, v))
    lr, beta1, beta2, eps, wd, coef = f(lr), f(beta1), f(beta2), f(eps), f(weight_decay), f(coef)
    bc1 = f(1.0 - float(beta1) ** step)
    bc2sqrt = f(math.sqrt(1.0 - float(beta2) ** step))
    gv = g * coef
    if wd != 0:
        if decoupled:
            p = p * f(f(1.0) - lr * wd)
        else:
            gv = gv + wd * p
    m = beta1 * m + f(f(1.0) - beta1) * gv
    v = beta2 * v + f(f(1.0) - beta2) * gv * gv
    denom = np.sqrt(v) / bc2sqrt + eps
    p = p - f(lr / bc1) * (m / denom)
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)
