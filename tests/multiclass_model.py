"""Float64 numpy restatement of the multi-class kernels (csrc/multiclass_kernels.h): the K-way 1x1 head, softmax and
argmax, the class loss with its logit gradient, the head's backward and the confusion matrix.  Not a test module: the
CPU tests hold it to torch, the GPU tests hold the kernels to it.

Layouts as in the library: activations x (P, C) with P = n * hw pixels; logits, probabilities and logit gradients
(n, K, hw); labels (n, hw) uint8."""
import numpy as np


def head(x, w, b, n):
    """x (P, C), w (K, C), b (K) -> logits (n, K, hw) in float64, and per logit sum_c |w x| + |b| (the magnitude the
    dot-product bound scales with)"""
    x, w, b = (np.asarray(a, dtype=np.float64) for a in (x, w, b))
    P, C = x.shape
    K = w.shape[0]
    z = x @ w.T + b                      # (P, K)
    mag = np.abs(x) @ np.abs(w).T + np.abs(b)
    to_planes = lambda a: a.reshape(n, P // n, K).transpose(0, 2, 1).copy()
    return to_planes(z), to_planes(mag)


def softmax(z):
    """(n, K, hw) -> exp(z_k - max z) / sum"""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def argmax(z):
    """labels (n, hw) uint8: the lowest index among the largest logits (scan from class 0 with `>`)"""
    return np.argmax(np.asarray(z), axis=1).astype(np.uint8)


def top_two_gap(z):
    """(n, hw): difference between the two largest logits of a pixel"""
    s = np.sort(np.asarray(z, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]


def valid_pixels(labels, K, ignore_index=-1):
    labels = np.asarray(labels)
    return (labels < K) & (labels != ignore_index)


def class_loss(z, labels, ce_weight=1.0, dice_weight=0.0, smooth=1.0, class_weight=None, ignore_index=-1, grad=True):
    """z (n, K, hw), labels (n, hw) uint8 -> {total, ce, dice, invalid} and dtotal/dz (n, K, hw).
    CE = sum_valid cw[t] (logsumexp(z) - z_t) / sum_valid cw[t] (0, with a zero gradient, when that sum is 0);
    Dice = 1 - mean_k (2 sum_valid p_k [t = k] + smooth) / (sum_valid p_k + sum_valid [t = k] + smooth)."""
    z = np.asarray(z, dtype=np.float64)
    labels = np.asarray(labels)
    n, K, hw = z.shape
    cw = np.ones(K) if class_weight is None else np.asarray(class_weight, dtype=np.float64)[:K]
    valid = valid_pixels(labels, K, ignore_index)                       # (n, hw)
    invalid = int(((labels >= K) & (labels != ignore_index)).sum())
    t = np.where(valid, labels, 0).astype(np.int64)
    onehot = (np.arange(K)[None, :, None] == t[:, None, :]) & valid[:, None, :]   # (n, K, hw)
    m = z.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]  # (n, hw)
    p = softmax(z)
    wt = np.where(valid, cw[t], 0.0)                                     # (n, hw)
    zt = np.take_along_axis(z, t[:, None, :], axis=1)[:, 0]
    den = wt.sum()
    ce = float((wt * (lse - zt)).sum() / den) if den > 0 else 0.0
    pv = p * valid[:, None, :]
    I = (pv * onehot).sum(axis=(0, 2))
    S = pv.sum(axis=(0, 2))
    T = onehot.sum(axis=(0, 2)).astype(np.float64)
    U = S + T + smooth
    dice = float(1.0 - ((2.0 * I + smooth) / U).mean())
    out = {"total": ce_weight * ce + dice_weight * dice, "ce": ce, "dice": dice, "invalid": invalid}
    if not grad:
        return out, None
    g_ce = (wt[:, None, :] * (p - onehot) / den) if den > 0 else np.zeros_like(z)
    # dDice/dp_k of a valid pixel: -(1/K) (2 [t = k] U_k - (2 I_k + smooth)) / U_k^2, then the softmax Jacobian
    A = (-2.0 / (K * U))[None, :, None]
    B = ((2.0 * I + smooth) / (K * U * U))[None, :, None]
    g = (A * onehot + B) * valid[:, None, :]
    g_dice = p * (g - (p * g).sum(axis=1, keepdims=True))
    return out, ce_weight * g_ce + dice_weight * g_dice


def head_backward(dl, a, w):
    """dl (n, K, hw), a (P, C), w (K, C) -> dA (P, C), dW (K, C), db (K)"""
    dl, a, w = (np.asarray(v, dtype=np.float64) for v in (dl, a, w))
    n, K, hw = dl.shape
    d = dl.transpose(0, 2, 1).reshape(n * hw, K)   # (P, K)
    return d @ w, d.T @ a, d.sum(axis=0)


def confusion(pred, truth, K, ignore_index=-1):
    """counts[t, p] over the pixels whose truth is < K and not ignore_index and whose prediction is < K (int64)"""
    pred, truth = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(truth).reshape(-1).astype(np.int64)
    keep = (truth < K) & (truth != ignore_index) & (pred < K)
    return np.bincount(truth[keep] * K + pred[keep], minlength=K * K).reshape(K, K).astype(np.int64)


def synthetic_labels(n, h, w, K, seed=0, ignore_index=None, ignore_fraction=0.0):
    """Blocky label planes (n, h, w) uint8 with every class present where the plane has room for it"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, K, size=(n, (h + 3) // 4, (w + 3) // 4))
    lab = np.repeat(np.repeat(coarse, 4, axis=1), 4, axis=2)[:, :h, :w].astype(np.uint8)
    flat = lab.reshape(-1)
    for k in range(min(K, flat.size)):
        flat[(k * 7919) % flat.size] = k
    if ignore_index is not None and ignore_fraction > 0:
        lab[rng.random(lab.shape) < ignore_fraction] = ignore_index
    return lab
