"""Multi-class segmentation on the GPU: the kernels of csrc/multiclass_kernels.h against the float64 model
(tests/multiclass_model.py), the K-class forward, training step, eval pass and validation against the CPU oracle, and
the single-class path left as it was.

Label comparisons: a pixel is compared where the reference's two largest logits differ by more than twice the logit
bound in force; at most 0.5 % of the pixels may be left out."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multiclass_model as M
import x3_model as X3
from oracle import unet_oracle as O
from unet_lane_detection_amd import _lib, augment as A, metrics, state as S

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-4          # tests/test_forward_gpu.py: the fp32 tier's logit bound
U = 2.0 ** -24            # fp32 unit roundoff
MAX_LEFT_OUT = 0.005


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=False)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(1e-12, np.abs(b).max())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _labels_agree(got, ref_logits, bound, what):
    """got (n, hw) labels against the argmax of the reference logits (n, K, hw), off ties"""
    sure = M.top_two_gap(ref_logits) > 2.0 * bound
    left_out = 1.0 - sure.mean()
    print(f"{what}: {100 * left_out:.3f} % of the pixels within the tie margin")
    assert left_out <= MAX_LEFT_OUT, (what, left_out)
    assert np.array_equal(np.asarray(got)[sure], M.argmax(ref_logits)[sure]), what
    return sure


# ---- the head operator ---------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(1, 5, 7), (2, 16, 24), (1, 1, (1 << 16) + 3)]


def _run_headk(lib, x, n, h, w, c, k, wt, b, want):
    """want: subset of {"logits", "probs", "labels", "mask"}; untouched outputs are not allocated"""
    out = {}
    if "logits" in want:
        out["logits"] = torch.full((n, k, h * w), float("nan"), device="cuda")
    if "probs" in want:
        out["probs"] = torch.full((n, k, h * w), float("nan"), device="cuda")
    if "labels" in want:
        out["labels"] = torch.full((n, h * w), 77, dtype=torch.uint8, device="cuda")
    if "mask" in want:
        out["mask"] = torch.full((n, h * w), 77, dtype=torch.uint8, device="cuda")
    p = _lib.ptr
    rc = lib.unet_op_headk(0, p(x), n, h, w, c, k, wt.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                           p(out.get("logits")), p(out.get("probs")), p(out.get("labels")), k - 1, p(out.get("mask")), None)
    _lib.check(rc, "unet_op_headk")
    return {name: t.cpu().numpy() for name, t in out.items()}


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", [4, 8, 64])
def test_headk_against_the_model(lib, shape, c):
    n, h, w = shape
    rng = np.random.default_rng(c * 1000 + h * w)
    x = rng.normal(0, 1, size=(n * h * w, c)).astype(np.float32)
    xd = _dev(x)
    worst = 0.0
    for k in (2, 3, 8):
        wt = (rng.normal(0, 1, size=(k, c)) * (2.0 / c) ** 0.5).astype(np.float32)
        b = rng.normal(0, 0.3, size=k).astype(np.float32)
        z, mag = M.head(x, wt, b, n)
        zb = (c + 2) * U * mag                       # the standard dot-product bound, per logit
        pix_bound = zb.max(axis=1)                   # (n, hw)
        pref = M.softmax(z)
        both = _run_headk(lib, xd, n, h, w, c, k, wt, b, {"logits", "probs", "labels", "mask"})
        for want in ({"logits"}, {"probs"}, {"labels"}, {"mask"}):
            alone = _run_headk(lib, xd, n, h, w, c, k, wt, b, want)
            (name,) = want
            assert np.array_equal(alone[name], both[name]), (k, name)      # an output does not depend on the others
        err = np.abs(both["logits"] - z)
        assert np.all(err <= zb), (k, float((err / zb).max()))
        worst = max(worst, float((err / zb).max()))
        # softmax: |dp_k| <= p_k (1 - p_k) |dz_k| + p_k sum_{j != k} p_j |dz_j| <= max_j |dz_j| / 2
        assert np.all(np.abs(both["probs"] - pref) <= 4 * U + 0.5 * pix_bound[:, None, :]), k
        sure = _labels_agree(both["labels"], z, pix_bound, f"head C={c} K={k}")
        assert np.array_equal(both["mask"], np.where(both["labels"] == k - 1, 255, 0)), k
        assert set(np.unique(both["labels"][sure])) <= set(range(k))
    print(f"head C={c} {shape}: largest logit error / bound = {worst:.3f}")


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", [8, 64])
def test_headk_planes_against_the_model(lib, shape, c):
    """The same head on the f16x3 tier's operand planes (a lane's step is eight channels, so C = 4 has no planes form).
    The planes are exact operands (x3_model.split_f16 / merged); the kernel forms hi + lo in fp32 - one more rounding
    of each input - and then the fp32 dot product: (C + 3) 2^-24 (|b| + sum |w x|)."""
    n, h, w = shape
    P = n * h * w
    gen = torch.Generator().manual_seed(c + h * w)
    hi, lo = X3.split_f16(torch.randn(P, c, generator=gen) * 3.0)
    x = X3.merged(hi, lo).numpy()
    planes = torch.cat([hi.reshape(-1), lo.reshape(-1)]).cuda()          # the lo plane P * c halfs behind the hi plane
    rng = np.random.default_rng(c)
    for k in (2, 3, 8):
        wt = (rng.normal(0, 1, size=(k, c)) * (2.0 / c) ** 0.5).astype(np.float32)
        b = rng.normal(0, 0.3, size=k).astype(np.float32)
        z, mag = M.head(x, wt, b, n)
        zb = (c + 3) * U * mag
        pix_bound = zb.max(axis=1)
        out = {"logits": torch.full((n, k, h * w), float("nan"), device="cuda"),
               "probs": torch.full((n, k, h * w), float("nan"), device="cuda"),
               "labels": torch.full((n, h * w), 77, dtype=torch.uint8, device="cuda"),
               "mask": torch.full((n, h * w), 77, dtype=torch.uint8, device="cuda")}
        p = _lib.ptr
        rc = lib.unet_op_headk_x3_planes(0, p(planes), P * c, n, h, w, c, k, wt.ctypes.data_as(C.c_void_p),
                                         b.ctypes.data_as(C.c_void_p), p(out["logits"]), p(out["probs"]), p(out["labels"]), 0,
                                         p(out["mask"]), None)
        _lib.check(rc, "unet_op_headk_x3_planes")
        got = {name: t.cpu().numpy() for name, t in out.items()}
        err = np.abs(got["logits"] - z)
        print(f"planes head C={c} K={k} {shape}: largest logit error / bound = {(err / zb).max():.3f}")
        assert np.all(err <= zb), k
        assert np.all(np.abs(got["probs"] - M.softmax(z)) <= 4 * U + 0.5 * pix_bound[:, None, :]), k
        _labels_agree(got["labels"], z, pix_bound, f"planes head C={c} K={k}")
        assert np.array_equal(got["mask"], np.where(got["labels"] == 0, 255, 0)), k
        lg = torch.full((n, k, h * w), float("nan"), device="cuda")      # the logits alone
        rc = lib.unet_op_headk_x3_planes(0, p(planes), P * c, n, h, w, c, k, wt.ctypes.data_as(C.c_void_p),
                                         b.ctypes.data_as(C.c_void_p), p(lg), None, None, 0, None, None)
        assert rc == 0 and np.array_equal(lg.cpu().numpy(), got["logits"])


def test_headk_ties_and_nan(lib):
    """equal logits go to the lowest class; a NaN logit never wins"""
    c, k = 4, 3
    x = np.zeros((4, c), dtype=np.float32)
    x[:, 0] = 1.0
    wt = np.zeros((k, c), dtype=np.float32)
    wt[:, 0] = [1.0, 1.0, 0.5]
    out = _run_headk(lib, _dev(x), 1, 2, 2, c, k, wt, np.zeros(k, np.float32), {"labels"})
    assert out["labels"].tolist() == [[0, 0, 0, 0]]
    wt[0, 0] = np.nan
    out = _run_headk(lib, _dev(x), 1, 2, 2, c, k, wt, np.zeros(k, np.float32), {"labels"})
    assert out["labels"].tolist() == [[1, 1, 1, 1]]


@pytest.mark.parametrize("shape,c,k", [((1, 5, 7), 4, 2), ((2, 16, 24), 64, 3), ((1, 1, (1 << 16) + 3), 8, 8),
                                       ((2, 16, 24), 12, 5)])
def test_headk_backward_against_the_model(lib, shape, c, k):
    n, h, w = shape
    rng = np.random.default_rng(c + k)
    P = n * h * w
    a = rng.normal(size=(P, c)).astype(np.float32)
    dl = (rng.normal(size=(n, k, h * w)) / P).astype(np.float32)
    wt = rng.normal(size=(k, c)).astype(np.float32)
    dA, dW, db = M.head_backward(dl, a, wt)
    got = []
    dld, ad = _dev(dl), _dev(a)
    for _ in range(2):
        gA = torch.full((P, c), float("nan"), device="cuda")
        gW, gb = torch.full((k, c), float("nan"), device="cuda"), torch.full((k,), float("nan"), device="cuda")
        p = _lib.ptr
        rc = lib.unet_op_headk_backward(0, p(dld), p(ad), wt.ctypes.data_as(C.c_void_p), n, h, w, c, k, p(gA), p(gW),
                                        p(gb), None)
        _lib.check(rc, "unet_op_headk_backward")
        got.append((gA.cpu().numpy(), gW.cpu().numpy(), gb.cpu().numpy()))
    # sums of P products of fp32 values: the dot-product bound with the magnitudes' sums
    d64, a64 = dl.astype(np.float64).transpose(0, 2, 1).reshape(P, k), a.astype(np.float64)
    assert np.all(np.abs(got[0][0] - dA) <= (k + 2) * U * (np.abs(d64) @ np.abs(wt.astype(np.float64))) + 1e-45)
    assert np.all(np.abs(got[0][1] - dW) <= (P + 2) * U * (np.abs(d64).T @ np.abs(a64)))
    assert np.all(np.abs(got[0][2] - db) <= (P + 2) * U * np.abs(d64).sum(axis=0))
    for x, y in zip(got[0], got[1]):
        assert np.array_equal(x, y)                                           # the same bits on every run


# ---- the class loss --------------------------------------------------------------------------------------------------
def _run_class_loss(lib, z, labels, k, spec, grad=True):
    n, _, hw = z.shape
    zd, ld = _dev(z), _dev(labels)
    terms = torch.full((4,), float("nan"), device="cuda")
    dl = torch.full(z.shape, float("nan"), device="cuda") if grad else None
    work = torch.empty(int(lib.unet_class_loss_work_bytes()) // 8, dtype=torch.float64, device="cuda")
    cfg = spec.to_c(k)
    _lib.call("unet_class_loss_grad", torch.device("cuda", 0), zd, ld, n, k, hw, C.byref(cfg), terms, dl, work)
    torch.cuda.synchronize()
    return terms.cpu().numpy(), (dl.cpu().numpy() if grad else None)


LOSS_CASES = {
    "ce": dict(ce_weight=1.0, dice_weight=0.0, smooth=1.0),
    "ce_dice": dict(ce_weight=0.5, dice_weight=0.5, smooth=1.0),
    "dice_weighted_ignore": dict(ce_weight=0.0, dice_weight=1.0, smooth=1e-3, ignore_index=255),
    "weighted_ignore": dict(ce_weight=0.7, dice_weight=0.3, smooth=1.0, class_weights="ramp", ignore_index=255),
    "one_frame_ignored": dict(ce_weight=0.5, dice_weight=0.5, smooth=1.0, ignore_index=255, blank_frame=True),
    "out_of_range": dict(ce_weight=0.5, dice_weight=0.5, smooth=1.0, stray=True),
    "ignore_a_class": dict(ce_weight=1.0, dice_weight=1.0, smooth=1.0, ignore_index=0),
}


@pytest.mark.parametrize("case", sorted(LOSS_CASES))
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 7), (2, 32, 48)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", [2, 3, 8])
def test_class_loss_against_the_model(lib, k, shape, case):
    n, h, w = shape
    kw = dict(LOSS_CASES[case])
    rng = np.random.default_rng(k * 7 + h)
    z = (rng.normal(0, 2.5, size=(n, k, h * w))).astype(np.float32)
    if h * w > 1:
        # a saturated pixel: no NaN, no Inf.  (Not where it is the only pixel: its gradient p_t - 1 ~ -e^-40 lies below
        # what one fp32 rounding of p_t can resolve, and max |dl| then measures nothing.)
        z[0, 0, 0] = 40.0
    ignore = kw.get("ignore_index")
    labels = M.synthetic_labels(n, h, w, k, seed=k, ignore_index=ignore if ignore == 255 else None,
                                ignore_fraction=0.15).reshape(n, h * w)
    if kw.pop("blank_frame", False):
        labels[n - 1] = 255
    stray = kw.pop("stray", False)
    if stray:
        labels[0, (h * w) // 2] = k + 1
    if kw.get("class_weights") == "ramp":
        kw["class_weights"] = [0.25 + 0.5 * i for i in range(k)]
        kw["class_weights"][k - 1] = 0.0
    spec = metrics.ClassLossSpec("ce_dice", **kw)
    want, g = M.class_loss(z, labels, spec.ce_weight, spec.dice_weight, spec.smooth, spec.class_weights, spec.ignore_index)
    terms, dl = _run_class_loss(lib, z, labels, k, spec)
    print(f"{case} K={k} {shape}: total {terms[0]:.6f} ce {terms[1]:.6f} dice {terms[2]:.6f}; "
          f"|d total| {abs(terms[0] - want['total']):.2e}")
    assert np.all(np.isfinite(terms)) and np.all(np.isfinite(dl))
    assert abs(terms[0] - want["total"]) < 2e-5 and abs(terms[1] - want["ce"]) < 2e-5 and abs(terms[2] - want["dice"]) < 2e-5
    assert terms[3] == want["invalid"] == (1 if stray else 0)
    gmax = np.abs(g).max()
    err = np.abs(dl - g).max()
    print(f"    max |d dlogits| / max |dlogits| = {err / max(gmax, 1e-300):.2e} (bound 2^-20 = {2.0 ** -20:.2e})")
    assert err <= 2.0 ** -20 * gmax          # measured over these cases: up to 6.9e-7 = 0.73 of the bound, which stays
    invalid = ~M.valid_pixels(labels, k, spec.ignore_index)
    assert np.all(dl.transpose(0, 2, 1)[invalid] == 0)
    terms2, dl2 = _run_class_loss(lib, z, labels, k, spec)
    assert np.array_equal(terms, terms2) and np.array_equal(dl, dl2)        # two runs, the same bits
    only, none = _run_class_loss(lib, z, labels, k, spec, grad=False)       # the loss alone (validation)
    assert none is None and np.array_equal(only, terms)


# ---- the confusion matrix -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numel", [1, 255, 257, 3072, (1 << 20) + 3])
def test_confusion_is_bit_exact(numel):
    rng = np.random.default_rng(numel)
    for k, ignore in ((3, None), (8, 255), (5, 2)):
        pred = rng.integers(0, k, numel).astype(np.uint8)
        truth = rng.integers(0, k + 1, numel).astype(np.uint8)        # k itself: out of range, never counted
        truth[rng.random(numel) < 0.1] = 255
        cm = metrics.ConfusionMatrix(k, 0, ignore)
        cm.accumulate(_dev(pred), _dev(truth))
        want = M.confusion(pred, truth, k, -1 if ignore is None else ignore)
        assert np.array_equal(cm.counts(), want), (k, ignore)
        cm.accumulate(_dev(truth % k), _dev(truth))                   # a second batch is added
        want = want + M.confusion(truth % k, truth, k, -1 if ignore is None else ignore)
        assert np.array_equal(cm.counts(), want), (k, ignore)
        assert abs(cm.miou() - metrics.ClassMetrics(want).miou) == 0 and cm.iou().shape == (k,)
        assert cm.pixel_accuracy() == np.trace(want) / max(1, want.sum()) or want.sum() == 0


# ---- the augmentation's label mode -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 17, 23), (2, 32, 48)])
def test_augment_label_mode_is_bit_exact(shape):
    ns, h, w = shape
    rng = np.random.default_rng(h)
    images = rng.integers(0, 256, size=(ns, h, w, 3), dtype=np.uint8)
    labels = rng.integers(0, 5, size=(ns, h, w)).astype(np.uint8)
    labels[0, :3] = 255
    aug = A.Augmenter(seed=11)
    params = aug.sample_params(2 * ns, ns)
    want_img, want_lab = A.apply_model(images, labels, params, labels=True)
    got_img, got_lab = aug.apply(_dev(images), _dev(labels), params, labels=True)
    assert got_lab.dtype == torch.uint8 and tuple(got_lab.shape) == (2 * ns, h, w)
    assert np.array_equal(got_lab.cpu().numpy(), want_lab) and np.array_equal(got_img.cpu().numpy(), want_img)
    # the float-target entry on the same table: the bits of the model, as before
    _, want_tgt = A.apply_model(images, labels, params)
    img2, tgt = aug.apply(_dev(images), _dev(labels), params)
    assert np.array_equal(tgt.cpu().numpy(), want_tgt) and torch.equal(img2, got_img)


# ---- the network: forward ---------------------------------------------------------------------------------------------
def _oracle_logits(sdn, frames):
    with torch.no_grad():
        return O.forward(O.to_torch_state(sdn), O.normalize_u8_nhwc(frames)).numpy()


@pytest.mark.parametrize("feats,shape,k", [([64, 128], (2, 32, 48), 3), ([64, 128], (2, 32, 48), 2),
                                           ([64, 128, 256], (1, 16, 32), 8), ([8, 16], (2, 32, 48), 4)])
def test_forward_classes_fp32_vs_oracle(feats, shape, k):
    from unet_lane_detection_amd.model import UNetHIP
    n, h, w = shape
    sdn = S.seeded_state_dict(feats, seed=6, out_channels=k)
    frames = S.synthetic_frames(n, h, w, seed=2)
    ref = _oracle_logits(sdn, frames)
    m = UNetHIP(sdn, device=0)
    assert m.out_channels == k
    cls = k - 1
    logits, probs, labels, mask = m.run_u8(_dev(frames), return_probs=True, return_labels=True, mask_class=cls)
    torch.cuda.synchronize()
    assert m.device_error() == 0
    got = logits.cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"{feats} K={k}: max |dlogit| = {err:.2e}")
    assert got.shape == (n, k, h, w) and err < LOGIT_TOL
    lab = labels.cpu().numpy()
    _labels_agree(lab.reshape(n, -1), ref.reshape(n, k, -1), LOGIT_TOL, f"forward {feats} K={k}")
    assert np.array_equal(mask.cpu().numpy(), np.where(lab == cls, 255, 0))
    assert np.abs(probs.cpu().numpy() - M.softmax(ref.reshape(n, k, -1)).reshape(ref.shape)).max() < 4 * U + 0.5 * LOGIT_TOL
    # the float entry computes the same network; logits alone are a tensor, not a tuple
    lg2 = m.forward(O.normalize_u8_nhwc(frames).cuda())
    assert isinstance(lg2, torch.Tensor) and (lg2 - logits).abs().max().item() < 1e-4
    with pytest.raises(ValueError):
        m.run_u8(_dev(frames), return_mask=True)
    with pytest.raises(ValueError):
        m.run_u8(_dev(frames), precision="bf16")
    m.release()


@pytest.mark.parametrize("feats,shape,k", [([64, 128], (2, 32, 48), 3), ([64, 128], (2, 32, 48), 2),
                                           ([64, 128, 256], (1, 16, 32), 8)])
def test_forward_classes_f16x3_vs_oracle(feats, shape, k):
    """the f16x3 tier: the last convolution stores its operand planes and the K-way head reads them; the tier's logit bound
    is the fp32 tier's (tests/test_x3_gpu.py)"""
    from unet_lane_detection_amd.model import UNetHIP
    n, h, w = shape
    sdn = S.seeded_state_dict(feats, seed=6, out_channels=k)
    frames = S.synthetic_frames(n, h, w, seed=2)
    ref = _oracle_logits(sdn, frames)
    m = UNetHIP(sdn, device=0)
    logits, probs, labels, mask = m.run_u8(_dev(frames), return_probs=True, return_labels=True, mask_class=0, precision="f16x3")
    torch.cuda.synchronize()
    assert m.device_error() == 0
    err = np.abs(logits.cpu().numpy() - ref).max()
    print(f"f16x3 {feats} K={k}: max |dlogit| = {err:.2e}")
    assert err < LOGIT_TOL
    lab = labels.cpu().numpy()
    _labels_agree(lab.reshape(n, -1), ref.reshape(n, k, -1), LOGIT_TOL, f"f16x3 forward {feats} K={k}")
    assert np.array_equal(mask.cpu().numpy(), np.where(lab == 0, 255, 0))
    assert np.abs(probs.cpu().numpy() - M.softmax(ref.reshape(n, k, -1)).reshape(ref.shape)).max() < 4 * U + 0.5 * LOGIT_TOL
    lg2 = m.forward(O.normalize_u8_nhwc(frames).cuda(), precision="f16x3")
    assert (lg2 - logits).abs().max().item() < 1e-4
    names = set()
    m.profile(True)
    m.run_u8(_dev(frames), precision="f16x3")
    names = {r[0] for r in m.profile_records()}
    m.profile(False)
    assert "headk_f16x3" in names and not any(nm.startswith("head1x1") for nm in names), names
    m.release()


# ---- the network: training step ---------------------------------------------------------------------------------------
def _relu_margin(sd, x):
    """as tests/test_train_gpu.py: the smallest |BatchNorm output| feeding a ReLU in a train-mode forward"""
    taps = {}
    with torch.no_grad():
        O.forward(sd, x, training=True, new_stats={}, taps=taps)
    m = float("inf")
    for key, z in taps.items():
        if not key.startswith("z/"):
            continue
        prefix, conv_i = key[2:].rsplit(".", 1)
        bn = f"{prefix}.{int(conv_i) + 1}"
        mu = z.mean(dim=(0, 2, 3), keepdim=True)
        var = z.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        y = (z - mu) * torch.rsqrt(var + O.BN_EPS) * sd[bn + ".weight"][None, :, None, None] \
            + sd[bn + ".bias"][None, :, None, None]
        m = min(m, float(y.abs().min()))
    return m


def _tie_free_frames(sd_t, n, hh, ww, margin=2e-6, good=5e-6, max_seeds=32):
    """as tests/test_train_gpu.py: a synthetic batch whose train-mode forward keeps every BatchNorm output away from the
    ReLU kink; finding none is a hard failure"""
    best = (-1.0, None, 0)
    for seed in range(2, 2 + max_seeds):
        frames = S.synthetic_frames(n, hh, ww, seed=seed)
        m = _relu_margin(sd_t, O.normalize_u8_nhwc(frames))
        if m > best[0]:
            best = (m, frames, seed - 2)
        if m > good:
            break
    if best[0] <= margin:
        pytest.fail(f"no tie-free input among {max_seeds} seeds (largest margin {best[0]:.2e} <= {margin:.0e})")
    print(f"tie-free input: margin {best[0]:.2e}")
    return best[1], best[2]


def _torch_class_loss(logits, labels, ce_weight, dice_weight, smooth, class_weight=None, ignore_index=-1):
    """F.cross_entropy(weight=, ignore_index=) + the Dice formula of include/unet_hip.h, on (N,K,H,W) logits"""
    t = labels.long()
    k = logits.shape[1]
    cw = None if class_weight is None else torch.tensor(class_weight, dtype=logits.dtype)
    ce = F.cross_entropy(logits, t, weight=cw, ignore_index=ignore_index if ignore_index >= 0 else -100)
    valid = (t != ignore_index)[:, None]
    p = torch.softmax(logits, dim=1) * valid
    onehot = (torch.arange(k)[None, :, None, None] == t[:, None]) & valid
    inter = (p * onehot).sum(dim=(0, 2, 3))
    dice = 1.0 - ((2.0 * inter + smooth) / (p.sum(dim=(0, 2, 3)) + onehot.sum(dim=(0, 2, 3)) + smooth)).mean()
    return ce_weight * ce + dice_weight * dice, ce, dice


TRAIN_CONFIGS = [([8, 16], (2, 32, 48), 4),        # the exact-fp32 path
                 ([64, 128], (2, 32, 48), 3),      # planes mode
                 ([64, 128], (2, 28, 28), 2)]      # per-consumer splits


@pytest.mark.parametrize("loss", ["ce", "ce_dice"])
@pytest.mark.parametrize("feats,shape,k", TRAIN_CONFIGS)
def test_training_step_vs_oracle(feats, shape, k, loss):
    from unet_lane_detection_amd.trainer import UNetTrainer
    n, hh, ww = shape
    sdn = S.seeded_state_dict(feats, seed=6, out_channels=k)
    sd_t = O.to_torch_state(sdn)
    frames, _ = _tie_free_frames(sd_t, n, hh, ww)
    labels = M.synthetic_labels(n, hh, ww, k, seed=2, ignore_index=255, ignore_fraction=0.1 if loss == "ce_dice" else 0.0)
    lt = torch.from_numpy(labels)
    if loss == "ce":
        args = dict(ce_weight=1.0, dice_weight=0.0, smooth=1.0, class_weight=None, ignore_index=-1)
    else:
        args = dict(ce_weight=0.5, dice_weight=0.5, smooth=1.0, class_weight=[1.0 + 0.5 * i for i in range(k)], ignore_index=255)
    fn = lambda lg, t: _torch_class_loss(lg, t, **args)[0]
    ref_loss, grads, new_stats, logits = O.loss_and_grads(sd_t, O.normalize_u8_nhwc(frames), lt, loss_fn=fn)
    total, ce, dice = _torch_class_loss(logits, lt, **args)
    runs = []
    for _ in range(2):
        tr = UNetTrainer(sdn, device=0)
        assert tr.out_channels == k and tr.loss_term_names == ("total", "ce", "dice", "invalid")
        if loss == "ce":
            tr.set_loss("ce", smooth=1.0)
        else:
            tr.set_loss("ce_dice", ce_weight=0.5, dice_weight=0.5, smooth=1.0, class_weights=args["class_weight"], ignore_index=255)
        lg = tr.forward_backward(torch.from_numpy(frames), lt, return_logits=True)
        torch.cuda.synchronize()
        assert tr.device_error() == 0
        runs.append((tr, lg.cpu(), tr.grads.clone(), tr.loss_terms.cpu().numpy()))
    tr, lg, _, terms = runs[0]
    assert tuple(lg.shape) == (n, k, hh, ww) and (lg - logits).abs().max().item() < 1e-4
    print(f"{feats} K={k} {loss}: total {terms[0]:.6f} (oracle {total.item():.6f})")
    assert abs(terms[0] - total.item()) < 2e-5 and abs(terms[1] - ce.item()) < 2e-5 and abs(terms[2] - dice.item()) < 2e-5
    assert terms[3] == 0 and abs(tr.loss_dict()["ce"] - terms[1]) == 0
    got = {name: v.detach().cpu().numpy() for name, v in tr.grad_dict().items()}
    assert got["output.weight"].shape == (k, feats[0], 1, 1) and got["output.bias"].shape == (k,)
    worst = max((_rel(got[name], g.numpy()), name) for name, g in grads.items())
    print(f"    worst gradient: {worst}")
    assert worst[0] < 1e-3, worst
    sd = tr.state_dict()
    for name, v in new_stats.items():
        if not name.endswith("num_batches_tracked"):
            assert _rel(sd[name].numpy(), v.numpy()) < 1e-5, name
    assert torch.equal(runs[0][2], runs[1][2]) and np.array_equal(runs[0][3], runs[1][3])      # bit-identical gradients
    for r in runs:
        r[0].release()


def test_training_reduces_the_class_loss_and_rejects_float_targets():
    from unet_lane_detection_amd.trainer import UNetTrainer
    k, feats = 3, [16, 32, 64]
    tr = UNetTrainer(S.seeded_state_dict(feats, seed=8, out_channels=k), device=0, lr=1e-3)
    tr.set_loss("ce_dice", smooth=1.0)
    frames = torch.from_numpy(S.synthetic_frames(4, 32, 32, seed=4))
    labels = torch.from_numpy(M.synthetic_labels(4, 32, 32, k, seed=4))
    losses = [float(tr.step(frames, labels).item()) for _ in range(10)]
    assert losses[-1] < losses[0] * 0.9, losses
    with pytest.raises(ValueError):
        tr.forward_backward(frames, labels.float())
    with pytest.raises(ValueError):
        tr.set_loss("bce_dice")
    tr.release()


def test_eval_and_validate_at_three_classes():
    from unet_lane_detection_amd.trainer import UNetTrainer
    k, feats, (n, h, w) = 3, [64, 128], (2, 32, 48)
    sdn = S.seeded_state_dict(feats, seed=6, out_channels=k)
    frames = S.synthetic_frames(2 * n, h, w, seed=2)
    labels = M.synthetic_labels(2 * n, h, w, k, seed=3, ignore_index=255, ignore_fraction=0.05)
    ref = _oracle_logits(sdn, frames)
    tr = UNetTrainer(sdn, device=0)
    tr.set_loss("ce_dice", smooth=1.0, ignore_index=255)
    before = (tr.params.clone(), tr.bn.clone())
    got = tr.eval_logits(torch.from_numpy(frames)).cpu().numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-4
    batches = [(torch.from_numpy(frames[i:i + n]), torch.from_numpy(labels[i:i + n])) for i in (0, n)]
    val, kept = tr.validate(batches, return_logits=True)
    pred = np.concatenate([tr.predict_labels(lg).cpu().numpy() for lg in kept])
    dev_logits = np.concatenate([lg.cpu().numpy() for lg in kept])
    assert np.array_equal(pred, M.argmax(dev_logits.reshape(2 * n, k, -1)).reshape(pred.shape))   # the device's own argmax
    want = M.confusion(pred, labels, k, 255)
    assert np.array_equal(val.counts, want)
    _labels_agree(pred.reshape(2 * n, -1), ref.reshape(2 * n, k, -1), 1e-4, "validate")
    m = metrics.ClassMetrics(want)
    assert val.miou == m.miou and val.pixel_acc == m.pixel_acc and val.dice == m.dice and len(val.iou) == k
    per_batch = [M.class_loss(dev_logits[i:i + n].reshape(n, k, -1), labels[i:i + n].reshape(n, -1), 0.5, 0.5, 1.0, None, 255,
                              grad=False)[0] for i in (0, n)]
    assert abs(val.loss - np.mean([b["total"] for b in per_batch])) < 2e-5
    assert abs(val.ce - np.mean([b["ce"] for b in per_batch])) < 2e-5 and val.batches == 2
    assert torch.equal(tr.params, before[0]) and torch.equal(tr.bn, before[1])                   # nothing moved
    tr.release()


def test_checkpoint_round_trip_at_three_classes(tmp_path):
    from unet_lane_detection_amd.model import UNetHIP
    from unet_lane_detection_amd.trainer import UNetTrainer
    k, feats = 3, [16, 32]
    sdn = S.seeded_state_dict(feats, seed=3, out_channels=k)
    frames = torch.from_numpy(S.synthetic_frames(2, 32, 32, seed=1))
    labels = torch.from_numpy(M.synthetic_labels(2, 32, 32, k, seed=1))
    a = UNetTrainer(sdn, device=0, lr=1e-3)
    for _ in range(2):
        a.step(frames, labels)
    path = os.path.join(tmp_path, "ck.pth")
    a.save_checkpoint(path, epoch=1, best_dice=0.25)
    for _ in range(2):
        a.step(frames, labels)
    b = UNetTrainer(sdn, device=0, lr=5e-2)
    b.load_checkpoint(path)
    want_logits = b.eval_logits(frames)
    want_labels = b.predict_labels(want_logits).cpu().numpy()
    for _ in range(2):
        b.step(frames, labels)
    assert torch.equal(a.params, b.params) and torch.equal(a.bn, b.bn)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    m = UNetHIP.from_checkpoint(path, device=0)
    assert m.out_channels == k
    logits, got = m.run_u8(frames.cuda(), return_labels=True)
    ref = want_logits.cpu().numpy().reshape(2, k, -1)
    assert (logits - want_logits).abs().max().item() < LOGIT_TOL
    _labels_agree(got.cpu().numpy().reshape(2, -1), ref, LOGIT_TOL, "from_checkpoint")
    assert np.array_equal(want_labels.reshape(2, -1), M.argmax(ref))
    for t in (a, b, m):
        t.release()


# ---- K = 1 is untouched ------------------------------------------------------------------------------------------------
NEW_RECORDS = ("headk", "class_loss_grad", "headk_bwd")
PARENT_TRAIN_WORKSPACE = {(8, 16): 43249664, (64, 128): 75800576}     # unet_train_workspace_bytes(2, 32, 48) of the parent commit


@pytest.mark.parametrize("feats", [(8, 16), (64, 128)])
def test_single_class_trainer_is_untouched(feats):
    from unet_lane_detection_amd.trainer import UNetTrainer
    tr = UNetTrainer(S.seeded_state_dict(list(feats), seed=6), device=0)
    assert tr.out_channels == 1 and tr.loss_term_names == ("total", "bce", "dice", "focal")
    assert int(tr._lib.unet_train_workspace_bytes(tr._h, 2, 32, 48)) == PARENT_TRAIN_WORKSPACE[feats]
    tr.profile(True)
    tr.step(torch.from_numpy(S.synthetic_frames(2, 32, 48, seed=2)), torch.from_numpy(S.synthetic_targets(2, 32, 48, seed=2)))
    names = {r[0] for r in tr.profile_records()}
    tr.profile(False)
    assert names and not any(n.startswith(NEW_RECORDS) for n in names), names
    assert "head_bwd" in names and "adam" in " ".join(names), names
    with pytest.raises(ValueError):
        tr.set_loss("ce")
    tr.release()
