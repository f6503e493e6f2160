"""Multi-class segmentation without a GPU: the float64 model of the kernels (tests/multiclass_model.py) against torch,
and the host logic of the C ABI - creation with K classes, the parameter spec, the refusals between single-class and
K-class entry points, the class loss's domain.  No kernel runs here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multiclass_model as M
from unet_lane_detection_amd import _lib, augment as A, metrics, state as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = 1, 3


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


# ---- the model against torch, float64 ---------------------------------------------------------------------------------
def torch_class_loss(z, labels, ce_weight, dice_weight, smooth, class_weight, ignore_index):
    """The issue's statement of the loss in torch: F.cross_entropy for the CE term, the Dice formula written out"""
    n, K, hw = z.shape
    t = labels.long()
    ign = ignore_index if ignore_index >= 0 else -100
    ce = F.cross_entropy(z, t, weight=class_weight, ignore_index=ign)
    valid = (t != ignore_index) if ignore_index >= 0 else torch.ones_like(t, dtype=torch.bool)
    p = torch.softmax(z, dim=1) * valid[:, None, :]
    onehot = (torch.arange(K)[None, :, None] == t[:, None, :]) & valid[:, None, :]
    inter = (p * onehot).sum(dim=(0, 2))
    dice = 1.0 - ((2.0 * inter + smooth) / (p.sum(dim=(0, 2)) + onehot.sum(dim=(0, 2)) + smooth)).mean()
    return ce_weight * ce + dice_weight * dice, ce, dice


@pytest.mark.parametrize("K,n,hw,cw,ignore", [(2, 1, 35, None, -1), (3, 2, 96, [0.5, 2.0, 1.0], 255), (8, 2, 64, None, 255),
                                              (4, 3, 40, [1.0, 0.0, 3.0, 0.25], 255)])
@pytest.mark.parametrize("weights", [(1.0, 0.0), (0.5, 0.5), (0.0, 1.0)])
def test_class_loss_model_agrees_with_torch(K, n, hw, cw, ignore, weights):
    rng = np.random.default_rng(K * 100 + hw)
    z = rng.normal(0, 3, size=(n, K, hw))
    labels = rng.integers(0, K, size=(n, hw)).astype(np.uint8)
    if ignore >= 0:
        labels[rng.random(labels.shape) < 0.2] = ignore
    ce_w, dice_w = weights
    out, g = M.class_loss(z, labels, ce_w, dice_w, 1.0, cw, ignore)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    cwt = None if cw is None else torch.tensor(cw, dtype=torch.float64)
    total, ce, dice = torch_class_loss(zt, torch.from_numpy(labels), ce_w, dice_w, 1.0, cwt, ignore)
    total.backward()
    assert abs(out["ce"] - ce.item()) <= 1e-12 * abs(ce.item())
    assert abs(out["dice"] - dice.item()) <= 1e-12 * abs(dice.item())
    assert abs(out["total"] - total.item()) <= 1e-12 * abs(total.item())
    assert _rel(g, zt.grad.numpy()) <= 1e-12
    assert out["invalid"] == 0


def test_class_loss_model_edge_cases():
    """An out-of-range label counts as ignored and is reported; with nothing valid the CE term and its gradient are 0
    (torch gives NaN there) while the Dice term is that of empty sums"""
    rng = np.random.default_rng(3)
    z = rng.normal(size=(1, 3, 12))
    labels = rng.integers(0, 3, size=(1, 12)).astype(np.uint8)
    labels[0, 5] = 7
    out, g = M.class_loss(z, labels, 1.0, 0.0, 1.0, None, 255)
    assert out["invalid"] == 1 and np.all(g[0, :, 5] == 0)
    keep = np.arange(12) != 5
    ref = F.cross_entropy(torch.tensor(z[:, :, keep]), torch.from_numpy(labels[:, keep]).long())
    assert abs(out["ce"] - ref.item()) <= 1e-12
    out, g = M.class_loss(z, np.full((1, 12), 255, np.uint8), 0.5, 0.5, 1.0, None, 255)
    assert out["ce"] == 0.0 and out["dice"] == 0.0 and np.all(g == 0) and out["invalid"] == 0


def test_head_model_agrees_with_torch():
    rng = np.random.default_rng(0)
    n, hw, C, K = 2, 15, 8, 3
    x, w, b = rng.normal(size=(n * hw, C)), rng.normal(size=(K, C)), rng.normal(size=K)
    z, mag = M.head(x, w, b, n)
    xt = torch.tensor(x.reshape(n, hw, 1, C).transpose(0, 3, 1, 2).copy())       # (n, C, hw, 1)
    ref = F.conv2d(xt, torch.tensor(w.reshape(K, C, 1, 1)), torch.tensor(b))[..., 0]
    assert _rel(z, ref.numpy()) <= 1e-12 and np.all(mag >= np.abs(z) - 1e-12)
    assert _rel(M.softmax(z), torch.softmax(ref, dim=1).numpy()) <= 1e-12
    assert np.array_equal(M.argmax(z), ref.argmax(dim=1).numpy().astype(np.uint8))
    tie = np.zeros((1, 3, 2))
    tie[0, :, 1] = [1.0, 2.0, 2.0]
    assert M.argmax(tie).tolist() == [[0, 1]]                                     # ties go to the lowest index
    # backward: autograd of sum(dl * logits)
    dl = rng.normal(size=z.shape)
    xa = torch.tensor(x, requires_grad=True)
    wa, ba = torch.tensor(w, requires_grad=True), torch.tensor(b, requires_grad=True)
    zz = (xa @ wa.T + ba).reshape(n, hw, K).permute(0, 2, 1)
    (zz * torch.tensor(dl)).sum().backward()
    dA, dW, db = M.head_backward(dl, x, w)
    assert _rel(dA, xa.grad.numpy()) <= 1e-12 and _rel(dW, wa.grad.numpy()) <= 1e-12 and _rel(db, ba.grad.numpy()) <= 1e-12


def test_confusion_model_agrees_with_a_direct_count():
    rng = np.random.default_rng(1)
    K = 5
    pred = rng.integers(0, K, 1000).astype(np.uint8)
    truth = rng.integers(0, K + 2, 1000).astype(np.uint8)
    truth[::17] = 255
    for ignore in (-1, 255, 2):
        want = np.zeros((K, K), dtype=np.int64)
        for p, t in zip(pred, truth):
            if t < K and t != ignore:
                want[t, p] += 1
        assert np.array_equal(M.confusion(pred, truth, K, ignore), want)
    m = metrics.ClassMetrics(M.confusion(pred, truth, K, 255))
    c = m.counts
    assert abs(m.pixel_acc - np.trace(c) / c.sum()) < 1e-15
    iou0 = c[0, 0] / (c[0].sum() + c[:, 0].sum() - c[0, 0])
    assert abs(m.iou[0] - iou0) < 1e-15 and abs(m.miou - m.iou.mean()) < 1e-15
    assert abs(m.dice - np.mean([2 * c[k, k] / (c[k].sum() + c[:, k].sum()) for k in range(K)])) < 1e-15
    assert metrics.ClassMetrics(np.zeros((3, 3))).dice == 1.0                       # nothing there, nothing claimed


def test_augment_model_label_mode_agrees_with_warp_mask():
    rng = np.random.default_rng(2)
    images = rng.integers(0, 256, size=(3, 17, 23, 3), dtype=np.uint8)
    labels = rng.integers(0, 4, size=(3, 17, 23)).astype(np.uint8)
    labels[0, :2] = 255
    params = A.Augmenter(seed=5).sample_params(6, 3)
    out, lab = A.apply_model(images, labels, params, labels=True)
    assert lab.dtype == np.uint8 and lab.shape == (6, 17, 23)
    for i, p in enumerate(params):
        assert np.array_equal(lab[i], A.warp_mask(labels[p["src"]], p["m"]))
    out2, tgt = A.apply_model(images, labels, params)                              # the float mode is what it was
    assert np.array_equal(out, out2) and tgt.shape == (6, 1, 17, 23) and tgt.dtype == np.float32
    assert np.array_equal(tgt[:, 0], (lab > 127).astype(np.float32))


# ---- the C ABI's host logic --------------------------------------------------------------------------------------------
def _create(lib, K, feats=(8, 16)):
    cfg = _lib.UnetConfig()
    cfg.in_channels, cfg.out_channels, cfg.depth = 3, K, len(feats)
    for i, f in enumerate(feats):
        cfg.features[i] = f
    h = C.c_void_p()
    return lib.unet_create(C.byref(cfg), C.byref(h)), h


def test_create_accepts_two_to_eight_classes(lib):
    for K in (1, 2, 3, 8):
        rc, h = _create(lib, K)
        assert rc == 0, K
        assert lib.unet_destroy(h) == 0
    for K in (0, 9, -1):
        assert _create(lib, K)[0] == INVALID, K
    assert _create(lib, 8, feats=(1024,))[0] == INVALID          # 8 x 1024 weights do not fit the head's LDS copy


@pytest.mark.parametrize("K", [2, 3, 8])
def test_param_spec_of_a_k_class_handle(lib, K):
    feats = (8, 16)
    rc, h = _create(lib, K, feats)
    assert rc == 0
    got = {lib.unet_param_name(h, i).decode(): lib.unet_param_numel(h, i) for i in range(lib.unet_num_params(h))}
    want = {k: int(np.prod(shape)) if shape else 1 for k, shape, kind in S.state_dict_spec(feats, 3, K) if kind != "bn_count"}
    assert got == want and got["output.weight"] == K * feats[0] and got["output.bias"] == K
    assert lib.unet_train_param_numel(h) == sum(v for k, v in got.items() if "running_" not in k)
    assert lib.unet_destroy(h) == 0


def _refused(lib, h, rc):
    msg = lib.unet_last_error(h)
    return rc == INVALID and bool(msg) and len(msg) > 10


def test_single_class_entry_points_refuse_a_k_class_handle(lib):
    rc, h = _create(lib, 3)
    assert rc == 0
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for name in ("unet_forward_u8", "unet_forward_f32", "unet_forward_u8_bf16", "unet_forward_u8_x3", "unet_forward_f32_x3"):
        assert _refused(lib, h, getattr(lib, name)(h, p, 1, 8, 8, p, None, None, 0.0, None)), name
        assert name.encode() in lib.unet_last_error(h)
    for name in ("unet_train_forward_backward_u8", "unet_train_forward_backward_f32"):
        assert _refused(lib, h, getattr(lib, name)(h, p, p, 1, 8, 8, p, None, None)), name
    assert _refused(lib, h, lib.unet_train_set_loss(h, 1, 0.5, 0.5, 3.0, 1e-6))
    cfg = _lib.LossConfig(2, 0.0, 1.0, 0.0, 1.0, 0.25, 2.0, 1e-6)
    assert _refused(lib, h, lib.unet_train_set_loss_cfg(h, C.byref(cfg)))
    assert _refused(lib, h, lib.unet_forward_u8_ranges(h, p, 1, 8, 8, p, None))
    # the tiers without a K-class forward say so
    assert _refused(lib, h, lib.unet_forward_classes_u8(h, p, 1, 8, 8, 2, p, None, None, 0, None, None))
    assert b"fp32 tier" in lib.unet_last_error(h)
    assert lib.unet_forward_classes_u8(h, p, 1, 8, 8, 1, p, None, None, 0, None, None) == STATE     # f16x3: not finalized yet
    assert _refused(lib, h, lib.unet_forward_classes_u8(h, p, 1, 8, 8, 0, p, None, None, 3, p, None))     # mask_class == K
    assert lib.unet_destroy(h) == 0


def test_k_class_entry_points_refuse_a_single_class_handle(lib):
    rc, h = _create(lib, 1)
    assert rc == 0
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for name in ("unet_forward_classes_u8", "unet_forward_classes_f32"):
        assert _refused(lib, h, getattr(lib, name)(h, p, 1, 8, 8, 0, p, None, None, 0, None, None)), name
    for name in ("unet_train_forward_backward_labels_u8", "unet_train_forward_backward_labels_f32"):
        assert _refused(lib, h, getattr(lib, name)(h, p, p, 1, 8, 8, p, None, None)), name
    cfg = metrics.ClassLossSpec().to_c(3)
    assert _refused(lib, h, lib.unet_train_set_class_loss(h, C.byref(cfg)))
    assert lib.unet_destroy(h) == 0


def test_class_loss_domain(lib):
    """checked before the handle's state: a valid configuration on a handle without training state is UNET_ERR_STATE,
    anything outside the domain UNET_ERR_INVALID_ARG"""
    rc, h = _create(lib, 3)
    assert rc == 0
    nan, inf = float("nan"), float("inf")

    def status(**kw):
        args = dict(kind="ce_dice", ce_weight=0.5, dice_weight=0.5, smooth=1.0, class_weights=(1.0, 2.0, 0.0), ignore_index=255)
        args.update(kw)
        cfg = metrics.ClassLossSpec(**args).to_c(3)
        return lib.unet_train_set_class_loss(h, C.byref(cfg))
    assert status() == STATE
    assert status(ce_weight=1.0, dice_weight=0.0) == STATE and status(ce_weight=0.0) == STATE and status(ignore_index=None) == STATE
    assert status(ignore_index=0) == STATE
    for bad in (dict(ce_weight=0.0, dice_weight=0.0), dict(ce_weight=-1.0), dict(dice_weight=-0.5), dict(smooth=0.0),
                dict(smooth=-1.0), dict(ce_weight=nan), dict(dice_weight=inf), dict(smooth=nan), dict(smooth=inf),
                dict(class_weights=(1.0, -1.0, 1.0)), dict(class_weights=(1.0, nan, 1.0)), dict(class_weights=(inf, 1.0, 1.0)),
                dict(ignore_index=256), dict(ignore_index=-2)):
        assert status(**bad) == INVALID, bad
        assert lib.unet_last_error(h)
    assert lib.unet_destroy(h) == 0


def test_operator_entry_points_check_arguments_first(lib):
    f = (C.c_float * 256)()
    base = (C.addressof(f) + 63) & ~63
    q, u = C.c_void_p(base), C.c_void_p(base + 256)
    cfg = metrics.ClassLossSpec().to_c(3)

    def headk(c=8, k=3, x=q, mask=None, mask_class=0):
        return lib.unet_op_headk(0, x, 1, 2, 2, c, k, q, q, q, None, None, mask_class, mask, None)
    assert headk(c=6) == INVALID and headk(k=1) == INVALID and headk(k=9) == INVALID and headk(c=1024, k=8) == INVALID
    assert headk(x=C.c_void_p(base + 4)) == INVALID and headk(mask=u, mask_class=3) == INVALID and headk(x=None) == INVALID
    assert lib.unet_op_last_error().startswith(b"invalid argument: unet_op_headk")
    planes = lambda c=8, lo=64, x=q: lib.unet_op_headk_x3_planes(0, x, lo, 1, 2, 2, c, 3, q, q, q, None, None, 0, None, None)
    assert planes(c=4) == INVALID and planes(c=12) == INVALID and planes(lo=36) == INVALID and planes(lo=16) == INVALID
    assert planes(x=C.c_void_p(base + 8)) == INVALID
    assert lib.unet_op_headk_backward(0, q, q, q, 1, 2, 2, 6, 3, None, q, q, None) == INVALID
    assert lib.unet_op_headk_backward(0, q, q, q, 1, 2, 2, 8, 3, None, None, q, None) == INVALID
    assert lib.unet_class_loss_grad(0, q, u, 1, 1, 4, C.byref(cfg), q, None, q, None) == INVALID        # one class
    assert lib.unet_class_loss_grad(0, q, u, 1, 3, 4, C.byref(cfg), q, None, None, None) == INVALID     # no work buffer
    bad = metrics.ClassLossSpec(smooth=0.0).to_c(3)
    assert lib.unet_class_loss_grad(0, q, u, 1, 3, 4, C.byref(bad), q, None, q, None) == INVALID
    assert lib.unet_class_labels_f32(0, q, 1, 3, 4, None, 0, None, None) == INVALID
    assert lib.unet_confusion_accumulate(0, u, u, 0, 3, -1, q, q, None) == INVALID
    assert lib.unet_confusion_accumulate(0, u, u, 4, 9, -1, q, q, None) == INVALID
    assert lib.unet_confusion_accumulate(0, u, u, 4, 3, 300, q, q, None) == INVALID
    assert lib.unet_augment_u8_labels(0, u, None, 1, 8, 8, q, 1, u, u, None) == INVALID
    # a call that passes every check fails at the device selection (an ordinal the runtime refuses: no device is touched)
    assert lib.unet_confusion_accumulate(1 << 20, u, u, 4, 3, -1, q, q, None) == _lib.UNET_ERR_HIP
    assert b"hipSetDevice" in lib.unet_op_last_error()
    assert lib.unet_confusion_work_bytes() > 0 and lib.unet_class_loss_work_bytes() > 0


def test_every_new_symbol_has_its_signature(lib):
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    new = {"unet_forward_classes_u8", "unet_forward_classes_f32", "unet_train_set_class_loss",
           "unet_train_forward_backward_labels_u8", "unet_train_forward_backward_labels_f32", "unet_confusion_work_bytes",
           "unet_confusion_accumulate", "unet_op_headk", "unet_op_headk_backward", "unet_class_loss_grad",
           "unet_class_loss_work_bytes", "unet_class_labels_f32", "unet_augment_u8_labels", "unet_op_headk_x3_planes"}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    for name in new:
        assert hasattr(lib, name), name
    assert C.sizeof(_lib.ClassLossConfig) == 4 * (3 + _lib.UNET_MAX_CLASSES + 1)
    assert re.search(r"#define UNET_MAX_CLASSES 8\b", hdr) and _lib.UNET_MAX_CLASSES == 8
