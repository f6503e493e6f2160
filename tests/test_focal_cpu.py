"""Host side of the general loss (mode 2: bce_weight * BCE(pos_weight) + focal_weight * Focal(alpha, gamma) +
dice_weight * Dice(smooth)): the formulas of include/unet_hip.h / DESIGN.md pinned to the reference's own loss classes,
the parameter domain of unet_train_set_loss_cfg, the focal slot of SegMetrics, the exported symbols.  No kernel runs
here."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from unet_lane_detection_amd import _lib, metrics
from unet_lane_detection_amd.metrics import SegMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def formulas(x, t, params, dtype):
    """The loss and its logit gradient exactly as DESIGN.md ("General loss") and csrc/loss_kernels.cpp state them,
    evaluated in `dtype`; the reductions in float64.  -> (total, bce, dice, focal), dL/dx."""
    wb, wf, wd, pw, alpha, gamma, smooth = (float(v) for v in params)
    f = dtype
    x, t = x.astype(f), t.astype(f)
    one = f(1)
    n = x.size
    e = np.exp(-np.abs(x))
    p = np.where(x >= 0, one / (one + e), e / (one + e))
    omp = np.where(x >= 0, e / (one + e), one / (one + e))
    l1p = np.log1p(e)
    ce = np.maximum(x, 0) - x * t + l1p
    q = p * (one - t) + omp * t                          # 1 - p_t, formed without the subtraction
    at = f(alpha) * t + (one - f(alpha)) * (one - t)
    if gamma == 0.0:                                     # no power: alpha-weighted BCE
        qg, qgm1 = np.ones_like(q), np.zeros_like(q)
    else:
        qgm1 = np.ones_like(q) if gamma == 1.0 else q ** f(gamma - 1.0)
        qg = qgm1 * q
    pmt = p * (one - t) - omp * t                        # p - t
    focal = float(np.sum((at * qg * ce).astype(np.float64)) / n)
    dfocal = at * (f(gamma) * qgm1 * (p * omp) * (one - f(2) * t) * ce + qg * pmt)
    # BCE(pos_weight) and Dice as csrc/train_kernels.h (bce_dice_*_kernel) has them
    logs, log1ms = np.minimum(x, 0) - l1p, -np.maximum(x, 0) - l1p
    bce = float(np.sum((-(f(pw) * t * logs + (one - t) * log1ms)).astype(np.float64)) / n)
    dbce = p * (one - t + f(pw) * t) - f(pw) * t
    inter, psum, tsum = (float(np.sum(v.astype(np.float64))) for v in (p * t, p, t))
    den = psum + tsum + smooth
    dice = 1.0 - (2.0 * inter + smooth) / den
    ddice = (p * omp) * (f(2) * t * f(1.0 / den) - f((2.0 * inter + smooth) / (den * den)))
    total = wb * bce + wf * focal + wd * dice
    grad = f(wb / n) * dbce + f(wf / n) * dfocal - f(wd) * ddice
    return np.array([total, bce, dice, focal]), grad.astype(np.float64)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "focal.npz"))


CASES = ("focal_a25_g2", "focal_a50_g1", "focal_a75_g35", "focal_a25_g0", "focal_dice", "combo", "dice", "soft")


def test_fixture_holds_the_cases_the_feature_is_specified_on(fixture):
    assert tuple(str(c) for c in fixture["cases"]) == CASES
    want = {"focal_a25_g2": (0, 1, 0, 0.25, 2), "focal_a50_g1": (0, 1, 0, 0.5, 1), "focal_a75_g35": (0, 1, 0, 0.75, 3.5),
            "focal_a25_g0": (0, 1, 0, 0.25, 0), "focal_dice": (0, 0.5, 0.5, 0.25, 2), "combo": (0.3, 0.3, 0.4, 0.25, 2),
            "dice": (0, 0, 1, 0.25, 2), "soft": (0, 0.5, 0.5, 0.25, 2)}
    for c in CASES:
        wb, wf, wd, pw, alpha, gamma, smooth = fixture[f"{c}/params"]
        assert (wb, wf, wd, alpha, gamma) == want[c] and smooth == 1e-6, c
        x, t = fixture[f"{c}/x"], fixture[f"{c}/t"]
        assert x.dtype == np.float32 and t.dtype == np.float32 and x.size == 3 * 2048 + 20
        tail_x, tail_t = x[-20:], t[-20:]
        assert sorted(set(np.abs(tail_x).tolist())) == [30.0, 60.0, 87.0, 100.0, 120.0]
        for v in (30.0, 60.0, 87.0, 100.0, 120.0):
            for sgn in (1.0, -1.0):     # each fixed logit with both targets
                assert sorted(tail_t[tail_x == sgn * v].tolist()) == ([0.0, 1.0] if c != "soft" else
                                                                      [float(np.float32(0.05)), float(np.float32(0.95))])
        assert set(np.unique(t).tolist()) == ({0.0, 1.0} if c != "soft" else {float(np.float32(0.05)), float(np.float32(0.95))})
        assert 0.05 < float((t > 0.5).mean()) < 0.12            # Bernoulli(0.085)
    assert fixture["combo/params"][3] == 3.0


@pytest.mark.parametrize("case", CASES)
def test_float64_formulas_reproduce_the_reference_classes(fixture, case):
    """The stable formulation is the same function as the reference's FocalLoss / BCEWithLogitsLoss / DiceLoss: in
    float64 it reproduces their loss terms to 1e-12 of max(1, |L|) and their gradient, element by element, to 1e-12 of
    the largest gradient element.  (Relative to the largest element, not to each one: where p_t is within 1e-6 of 1 the
    REFERENCE's 1 - p_t has lost ten digits even in float64, and those elements' gradients are ~1e-12 of the largest.)"""
    terms, grad = formulas(fixture[f"{case}/x"], fixture[f"{case}/t"], fixture[f"{case}/params"], np.float64)
    want_t, want_g = fixture[f"{case}/terms64"], fixture[f"{case}/gx64"]
    assert np.isfinite(grad).all()
    for got, want in zip(terms, want_t):
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (case, terms, want_t)
    worst = np.abs(grad - want_g).max() / np.abs(want_g).max()
    print(f"{case}: float64 formulas vs reference classes: {worst:.2e} of the largest gradient element")
    assert worst <= 1e-12, (case, worst)


@pytest.mark.parametrize("case", CASES)
def test_float32_formulas_stay_inside_the_device_bound(fixture, case):
    """The same expressions in fp32 numpy (the arithmetic the kernels do, minus the device's expf / log1pf / powf
    rounding) against the bound the GPU test applies: per element max(2 * E32, 2^-20 * max|dx64|), E32 the worst deviation
    of the reference's own fp32 run from its float64 run.  No NaN / Inf at the saturated logits."""
    terms, grad = formulas(fixture[f"{case}/x"], fixture[f"{case}/t"], fixture[f"{case}/params"], np.float32)
    g64 = fixture[f"{case}/gx64"]
    e32 = np.abs(fixture[f"{case}/gx32"].astype(np.float64) - g64).max()
    bound = max(2 * e32, 2.0 ** -20 * np.abs(g64).max())
    assert np.isfinite(grad).all() and np.isfinite(terms).all()
    worst = np.abs(grad - g64).max()
    print(f"{case}: fp32 formulas {worst / np.abs(g64).max():.2e}, reference fp32 {e32 / np.abs(g64).max():.2e} of max|dx|")
    assert worst <= bound, (case, worst, bound)
    for got, want in zip(terms, fixture[f"{case}/terms64"]):
        assert abs(got - want) <= 2e-5 * max(1.0, abs(want))


def _cfg(mode=2, wb=0.0, wf=0.5, wd=0.5, pw=3.0, alpha=0.25, gamma=2.0, smooth=1e-6):
    return _lib.LossConfig(mode, wb, wf, wd, pw, alpha, gamma, smooth)


@pytest.fixture(scope="module")
def bare_handle():
    """A handle that never touches a device: unet_create only enumerates the parameters."""
    lib = _lib.load()
    cfg = _lib.UnetConfig()
    cfg.in_channels, cfg.out_channels, cfg.depth = 3, 1, 2
    cfg.features[0], cfg.features[1] = 4, 8
    h = C.c_void_p()
    assert lib.unet_create(C.byref(cfg), C.byref(h)) == 0
    yield lib, h
    assert lib.unet_destroy(h) == 0


INVALID = [dict(wb=-0.1), dict(wf=-1.0), dict(wd=-1e-9), dict(wb=0.0, wf=0.0, wd=0.0), dict(pw=0.0), dict(pw=-3.0),
           dict(alpha=-0.01), dict(alpha=1.01), dict(smooth=0.0), dict(smooth=-1e-6), dict(gamma=0.5), dict(gamma=0.999),
           dict(gamma=1e-3), dict(gamma=-1.0), dict(gamma=float("nan")), dict(wf=float("inf")), dict(alpha=float("nan")),
           dict(pw=float("nan")), dict(mode=3), dict(mode=-1)]


@pytest.mark.parametrize("bad", INVALID, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_set_loss_cfg_rejects_parameters_outside_the_domain(bare_handle, bad):
    lib, h = bare_handle
    c = _cfg(**bad)
    assert lib.unet_train_set_loss_cfg(h, C.byref(c)) == 1          # UNET_ERR_INVALID_ARG


def test_set_loss_cfg_accepts_the_domain_and_then_asks_for_an_attached_state(bare_handle):
    """Parameters are judged first: a valid mode-2 configuration gets past the check and is then refused for the
    missing unet_train_attach (UNET_ERR_STATE = 3), so the rejections above are about the parameters."""
    lib, h = bare_handle
    for ok in (dict(), dict(gamma=0.0), dict(gamma=1.0), dict(gamma=3.5), dict(alpha=0.0), dict(alpha=1.0),
               dict(wb=1.0, wf=0.0, wd=0.0), dict(wb=0.0, wf=0.0, wd=1.0), dict(wb=0.3, wf=0.3, wd=0.4)):
        c = _cfg(**ok)
        assert lib.unet_train_set_loss_cfg(h, C.byref(c)) == 3, ok
    assert lib.unet_train_set_loss_cfg(h, None) == 1
    assert lib.unet_train_set_loss_cfg(None, C.byref(_cfg())) == 1
    # modes 0 and 1 are unet_train_set_loss itself, which answers INVALID_ARG without an attached state
    for mode in (0, 1):
        assert lib.unet_train_set_loss_cfg(h, C.byref(_cfg(mode=mode))) == lib.unet_train_set_loss(h, mode, 0.5, 0.5, 3.0, 1e-6) == 1


def test_operator_and_accumulate_reject_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    bad = _cfg(gamma=0.5)
    assert lib.unet_op_loss_grad(0, p, p, 4, C.byref(bad), p, p, None) == 1
    assert lib.unet_op_loss_grad(0, p, p, 0, C.byref(_cfg()), p, p, None) == 1
    assert lib.unet_op_loss_grad(0, p, p, 4, C.byref(_cfg(mode=1)), p, p, None) == 1      # the operator is mode 2 only
    assert lib.unet_op_loss_grad(0, None, p, 4, C.byref(_cfg()), p, p, None) == 1
    assert lib.unet_seg_metrics_accumulate_cfg(0, p, p, 0, 4, 0.0, C.byref(bad), p, None) == 1
    assert lib.unet_seg_metrics_accumulate_cfg(0, p, p, 0, 4, 0.0, None, p, None) == 1
    assert lib.unet_seg_metrics_accumulate_cfg(0, p, p, 0, 0, 0.0, C.byref(_cfg()), p, None) == 1
    assert lib.unet_mask_positive_counts(0, None, 1, 4, 127, p, None) == 1
    assert lib.unet_mask_positive_counts(0, p, 0, 4, 127, p, None) == 1
    assert lib.unet_mask_positive_counts(0, p, 1, 0, 127, p, None) == 1


def test_header_documents_the_gamma_domain_and_cites_the_reference():
    with open(os.path.join(ROOT, "include", "unet_hip.h")) as f:
        hdr = f.read()
    for name in ("unet_train_set_loss_cfg", "unet_seg_metrics_accumulate_cfg", "unet_op_loss_grad", "unet_mask_positive_counts"):
        assert f"int {name}(" in hdr
    assert "typedef struct unet_loss_config" in hdr
    assert "0 < gamma < 1 is rejected" in hdr and "README.md:1914-1939" in hdr and "README.md:2514-2530" in hdr
    lib = _lib.load()
    assert len(lib.unet_seg_metrics_accumulate_cfg.argtypes) == 9 and len(lib.unet_op_loss_grad.argtypes) == 8
    assert C.sizeof(_lib.LossConfig) == 32


def test_segmetrics_focal_slot():
    assert metrics.FOCAL == 10 and metrics.NUM_ACCUMULATORS == 16
    a = np.zeros(16)
    a[:10] = [30, 10, 20, 940, 1.5, 0.9, 2.1, 1.2, 3, 1000]
    a[metrics.FOCAL] = 0.6
    m = SegMetrics(a)
    assert abs(m.focal - 0.2) < 1e-15 and m.loss == 0.5 and m.bce == 0.3
    d = m.as_dict()
    assert d["focal"] == m.focal and d["loss"] == 0.5 and d["tp"] == 30
    # a pass under 'bce' / 'bce_dice' never writes the slot: the focal term reads 0, and nan with no batch
    a[metrics.FOCAL] = 0.0
    assert SegMetrics(a).focal == 0.0 and SegMetrics(a).as_dict()["focal"] == 0.0
    assert math.isnan(SegMetrics(np.zeros(16)).focal)


def test_loss_spec_carries_the_configuration():
    import unet_lane_detection_amd as pkg
    s = pkg.LossSpec("focal_dice", 0.0, 0.5, 0.5, 3.0, 0.25, 2.0, 1e-6)
    c = s.to_c()
    assert (c.mode, c.bce_weight, c.focal_weight, c.dice_weight, c.pos_weight, c.alpha, c.gamma) == (2, 0.0, 0.5, 0.5, 3.0, 0.25, 2.0)
    assert abs(c.smooth - 1e-6) < 1e-12 and "focal_dice" in repr(s)
