"""The general loss on the device (mode 2: bce_weight * BCE(pos_weight) + focal_weight * Focal(alpha, gamma) +
dice_weight * Dice(smooth)): the operator against the reference's own loss classes run in float64
(tests/golden/focal.npz, make_golden_focal.py), arbitrary sizes, its reductions to the two older modes, the training
step and two AdamW steps through the network, and the validation pass."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_oracle as O
from unet_lane_detection_amd import metrics, state as S

pytestmark = pytest.mark.gpu

CASES = ("focal_a25_g2", "focal_a50_g1", "focal_a75_g35", "focal_a25_g0", "focal_dice", "combo", "dice", "soft")
SMOOTH = 1e-6


def _lib():
    from unet_lane_detection_amd import _lib as L
    return L, L.load(build_if_missing=False)


def compose(x, t, wb, wf, wd, pw, alpha, gamma, smooth=SMOOTH):
    """The composition wb * BCEWithLogits(pos_weight) + wf * FocalLoss(alpha, gamma) + wd * DiceLoss(smooth) of the
    reference's classes (README.md:1855-1893, :1914-1939, :1781-1807) in torch, in the dtype of x, with autograd:
    -> (total, bce, dice, focal)."""
    bce = (-(pw * t * F.logsigmoid(x) + (1 - t) * F.logsigmoid(-x))).mean()
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    q = torch.sigmoid(x) * (1 - t) + torch.sigmoid(-x) * t          # 1 - p_t
    at = alpha * t + (1 - alpha) * (1 - t)
    focal = (at * (q ** gamma if gamma else 1.0) * ce).mean()
    s, tf = torch.sigmoid(x).reshape(-1), t.reshape(-1)
    dice = 1 - (2.0 * (s * tf).sum() + smooth) / (s.sum() + tf.sum() + smooth)
    return wb * bce + wf * focal + wd * dice, bce, dice, focal


def op_loss_grad(x, t, wb, wf, wd, pw, alpha, gamma, smooth=SMOOTH):
    """unet_op_loss_grad on device tensors -> (4 loss terms, dlogits), both on the device."""
    L, lib = _lib()
    terms = torch.full((4,), float("nan"), device="cuda")
    dx = torch.full_like(x, float("nan"))
    cfg = L.LossConfig(2, wb, wf, wd, pw, alpha, gamma, smooth)
    rc = lib.unet_op_loss_grad(0, C.c_void_p(x.data_ptr()), C.c_void_p(t.data_ptr()), x.numel(), C.byref(cfg),
                               C.c_void_p(terms.data_ptr()), C.c_void_p(dx.data_ptr()),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return terms, dx


@pytest.mark.parametrize("case", CASES)
def test_operator_vs_reference_classes(golden_dir, case):
    """Against the float64 run of the reference classes.  Loss terms within 2e-5 * max(1, |L|) (the project's bound on
    loss values, tests/test_train_gpu.py); the gradient per element within max(2 * E32, 2^-20 * max|dx64|), E32 = the
    worst deviation of the reference's own fp32 run from its float64 run for the case (factor 2: the device's expf /
    log1pf / powf rounding; the floor is 16 ulp at the largest element).
    tools/loss_timing.py records the worst ratio per case in profiles/r06/focal_loss.md."""
    g = np.load(os.path.join(golden_dir, "focal.npz"))
    wb, wf, wd, pw, alpha, gamma, smooth = (float(v) for v in g[f"{case}/params"])
    x, t = torch.from_numpy(g[f"{case}/x"]).cuda(), torch.from_numpy(g[f"{case}/t"]).cuda()
    terms, dx = op_loss_grad(x, t, wb, wf, wd, pw, alpha, gamma, smooth)
    terms, dx = terms.cpu().numpy().astype(np.float64), dx.cpu().numpy().astype(np.float64)
    g64, t64 = g[f"{case}/gx64"], g[f"{case}/terms64"]
    e32 = np.abs(g[f"{case}/gx32"].astype(np.float64) - g64).max()
    bound = max(2 * e32, 2.0 ** -20 * np.abs(g64).max())
    worst = np.abs(dx - g64).max()
    print(f"focal operator {case}: terms {terms} (float64 {t64}), worst |dx - dx64| {worst:.3e} = {worst / bound:.3f} of the "
          f"bound {bound:.3e} ({worst / np.abs(g64).max():.2e} of max|dx|; reference fp32 {e32 / np.abs(g64).max():.2e})")
    assert np.isfinite(terms).all() and np.isfinite(dx).all()
    for got, want in zip(terms, t64):
        assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (case, terms, t64)
    assert worst <= bound, (case, worst, bound)


@pytest.mark.parametrize("params", [(0.0, 0.5, 0.5, 3.0, 0.25, 2.0), (0.3, 0.3, 0.4, 3.0, 0.6, 3.5)],
                         ids=["focal_dice", "combo_g3.5"])
@pytest.mark.parametrize("numel", [1, 255, 257, 4099, 2 * 32 * 32, 64 * 224 * 224])
def test_operator_sizes_finite_and_deterministic(numel, params):
    """Sizes that are multiples of nothing (element-wise tail, buffers offset by one float: no 128-bit access) and the
    benchmark's batch, against a float64 torch evaluation of the same composition on the host: loss terms within
    2e-5 * max(1, |L|), every gradient element within 2^-20 * max|dx64| (16 ulp at the largest element: each element is
    a sum of three products of fewer than ten fp32 roundings each).  Two runs give the same bits."""
    gen = torch.Generator().manual_seed(numel)
    x = torch.randn(numel, generator=gen) * 2.5
    t = (torch.rand(numel, generator=gen) < 0.085).float()
    x64 = x.double().requires_grad_(True)
    want = compose(x64, t.double(), *params)
    want[0].backward()
    g64 = x64.grad.numpy()
    for offset in (0, 1):
        # offset 1: a view that starts 4 bytes into the allocation
        xd = torch.empty(numel + offset, device="cuda")[offset:].copy_(x)
        td = torch.empty(numel + offset, device="cuda")[offset:].copy_(t)
        terms, dx = op_loss_grad(xd, td, *params)
        terms2, dx2 = op_loss_grad(xd, td, *params)
        assert torch.equal(terms, terms2) and torch.equal(dx, dx2)
        terms, dx = terms.cpu().numpy().astype(np.float64), dx.cpu().numpy().astype(np.float64)
        assert np.isfinite(terms).all() and np.isfinite(dx).all()
        for got, w in zip(terms, want):
            assert abs(got - float(w)) <= 2e-5 * max(1.0, abs(float(w))), (numel, offset, terms, [float(v) for v in want])
        worst = np.abs(dx - g64).max() / np.abs(g64).max()
        print(f"numel {numel} offset {offset}: worst |dx - dx64| {worst:.2e} of max|dx|")
        assert worst <= 2.0 ** -20, (numel, offset, worst)


def _trainer(feats=(16, 32), seed=9, **kw):
    from unet_lane_detection_amd.trainer import UNetTrainer
    return UNetTrainer(S.seeded_state_dict(list(feats), seed=seed), device=0, **kw)


def _step_outputs(configure, frames, tgt):
    tr = _trainer()
    configure(tr)
    tr.forward_backward(frames, tgt)
    torch.cuda.synchronize()
    assert tr.device_error() == 0
    out = tr.loss_terms.clone(), tr.grads.clone()
    tr.release()
    return out


@pytest.mark.parametrize("old,new", [
    (("bce",), dict(kind="combo", bce_weight=1.0, pos_weight=1.0, focal_weight=0.0, dice_weight=0.0)),
    (("bce_dice", 0.5, 0.5, 3.0), dict(kind="combo", bce_weight=0.5, pos_weight=3.0, focal_weight=0.0, dice_weight=0.5)),
    (("bce",), dict(kind="focal", alpha=0.5, gamma=0.0, focal_weight=2.0))], ids=["bce", "bce_dice", "focal_gamma0"])
def test_general_loss_reduces_to_the_existing_modes(old, new):
    """The general loss with the weights of an existing mode against that mode's own kernels, through the training step
    (config [16, 32]: exact-fp32 convolutions, so the backward pass is one linear map of dlogits): loss within 2e-5,
    gradients within 2^-20 of the largest gradient element."""
    frames = torch.from_numpy(S.synthetic_frames(2, 32, 32, seed=3))
    tgt = torch.from_numpy(S.synthetic_targets(2, 32, 32, seed=5))
    lt_old, g_old = _step_outputs(lambda tr: tr.set_loss(*old), frames, tgt)
    lt_new, g_new = _step_outputs(lambda tr: tr.set_loss(**new), frames, tgt)
    assert abs(float(lt_new[0]) - float(lt_old[0])) < 2e-5
    if old[0] == "bce_dice":
        assert abs(float(lt_new[1]) - float(lt_old[1])) < 2e-5 and abs(float(lt_new[2]) - float(lt_old[2])) < 2e-5
    worst = float((g_new - g_old).abs().max() / g_old.abs().max())
    print(f"{new['kind']} vs {old[0]}: loss {float(lt_new[0]):.7f} / {float(lt_old[0]):.7f}, gradients differ by {worst:.2e} "
          "of the largest element")
    assert worst <= 2.0 ** -20, worst


@pytest.mark.parametrize("mode", [0, 1])
def test_old_modes_through_the_new_entry_point_are_bit_identical(mode):
    L, lib = _lib()
    frames = torch.from_numpy(S.synthetic_frames(2, 32, 32, seed=3))
    tgt = torch.from_numpy(S.synthetic_targets(2, 32, 32, seed=5))

    def via_old(tr):
        assert lib.unet_train_set_loss(tr._h, mode, 0.5, 0.5, 3.0, 1e-6) == 0

    def via_new(tr):
        # focal fields that mode 0 / 1 must ignore
        cfg = L.LossConfig(mode, 0.5, 7.0, 0.5, 3.0, 0.9, 0.5, 1e-6)
        assert lib.unet_train_set_loss_cfg(tr._h, C.byref(cfg)) == 0

    lt_old, g_old = _step_outputs(via_old, frames, tgt)
    lt_new, g_new = _step_outputs(via_new, frames, tgt)
    assert torch.equal(lt_old, lt_new) and torch.equal(g_old, g_new) and float(g_old.abs().max()) > 0


def test_set_loss_kinds_and_domain_on_a_live_trainer():
    L, lib = _lib()
    tr = _trainer()
    with pytest.raises(L.UnetError):
        tr.set_loss("focal", gamma=0.5)
    with pytest.raises(ValueError):
        tr.set_loss("combo", bce_weight=0.3, dice_weight=0.4)        # all three weights explicitly
    with pytest.raises(ValueError):
        tr.set_loss("tversky")
    tr.set_loss("focal_dice")
    s = tr._loss_cfg
    assert (s.bce_weight, s.focal_weight, s.dice_weight, s.alpha, s.gamma) == (0.0, 0.5, 0.5, 0.25, 2.0)
    tr.set_loss("bce_dice", 0.5, 0.5, 3.0)
    assert tr._loss_cfg == ("bce_dice", 0.5, 0.5, 3.0, 1e-6)       # the 5-tuple the older kinds leave
    tr.release()


# ---- the helpers of tests/test_train_gpu.py's gradient-parity tests, restated (test modules do not import each other) ----
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(1e-12, np.abs(b).max())


def _check_grads(tr, ref_grads, loss_ref, gtol):
    assert abs(float(tr.loss.item()) - loss_ref) < 2e-5 * max(1.0, abs(loss_ref))
    got = {k: v.detach().cpu().numpy() for k, v in tr.grad_dict().items()}
    worst = max((_rel(got[k], ref_grads[k]), k) for k in ref_grads)
    assert worst[0] < gtol, worst
    return worst


def _relu_margin(sd, x):
    """Smallest |BatchNorm output| feeding a ReLU in a train-mode forward: gradient parity is only defined away from
    the kink (see tests/test_train_gpu.py)."""
    taps = {}
    with torch.no_grad():
        O.forward(sd, x, training=True, new_stats={}, taps=taps)
    m = float("inf")
    for k, z in taps.items():
        if not k.startswith("z/"):
            continue
        prefix, conv_i = k[2:].rsplit(".", 1)
        bn = f"{prefix}.{int(conv_i) + 1}"
        mu = z.mean(dim=(0, 2, 3), keepdim=True)
        var = z.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        y = (z - mu) * torch.rsqrt(var + O.BN_EPS) * sd[bn + ".weight"][None, :, None, None] \
            + sd[bn + ".bias"][None, :, None, None]
        m = min(m, float(y.abs().min()))
    return m


def _tie_free_frames(sd_t, n, hh, ww, margin=2e-6, good=5e-6, max_seeds=32):
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
    return best[1], best[2]


def test_focal_dice_loss_and_grads_vs_oracle():
    """test_bce_dice_loss_and_grads_vs_oracle (tests/test_train_gpu.py) with the loss the reference prescribes for masks
    under 5 % lane: 0.5 * FocalLoss(0.25, 2) + 0.5 * DiceLoss (README.md:1949)."""
    feats = [16, 32]
    sdn = S.seeded_state_dict(feats, seed=9)
    sd_t = O.to_torch_state(sdn)
    n, hh, ww = 2, 32, 32
    frames, _ = _tie_free_frames(sd_t, n, hh, ww)
    tgt = torch.from_numpy(S.synthetic_targets(n, hh, ww, seed=5))
    args = (0.0, 0.5, 0.5, 3.0, 0.25, 2.0)
    loss, grads, _, logits = O.loss_and_grads(sd_t, O.normalize_u8_nhwc(frames), tgt,
                                              loss_fn=lambda lg, t: compose(lg, t, *args)[0])
    want = [float(v) for v in compose(logits, tgt, *args)]
    from unet_lane_detection_amd.trainer import UNetTrainer
    tr = UNetTrainer(sdn, device=0)
    tr.set_loss("focal_dice")
    tr.profile(True)
    tr.forward_backward(torch.from_numpy(frames), tgt)
    names = [r[0] for r in tr.profile_records()]
    tr.profile(False)
    assert names.count("focal_loss_grad") == 1 and "bce_dice_loss_grad" not in names and "bce_loss_grad" not in names
    lt = tr.loss_terms.cpu().numpy()
    print("focal_dice through the network: terms", lt, "oracle", want)
    for got, w in zip(lt, want):
        assert abs(got - w) < 2e-5, (lt, want)
    _check_grads(tr, {k: v.numpy() for k, v in grads.items()}, float(loss), 1e-3)
    tr.release()


@pytest.mark.parametrize("tag", ["ref", "amp"])
def test_adamw_focal_dice_two_steps_vs_reference_golden(golden_dir, tag):
    """Two AdamW steps of the reference UNet([4, 8]) under 0.5 * FocalLoss(0.25, 2) + 0.5 * DiceLoss
    (tests/golden/make_golden_focal.py), with the tolerances of test_adamw_bcedice_two_steps_vs_reference_golden."""
    from unet_lane_detection_amd.trainer import UNetTrainer
    g = np.load(os.path.join(golden_dir, "tiny_f4_8_focal2.npz"))
    lr, wd = float(g[f"{tag}/lr"]), float(g[f"{tag}/wd"])
    x, t = torch.from_numpy(g["input"]), torch.from_numpy(g["target"])
    tr = UNetTrainer(S.seeded_state_dict([4, 8], seed=1), device=0, lr=lr, weight_decay=wd, decoupled=True)
    tr.set_loss("focal_dice")
    for step in range(2):
        tr.step(x, t)
        got = tr.loss_terms.cpu().numpy().astype(np.float64)        # (total, bce with pos_weight 3, dice, focal)
        assert np.abs(got - g[f"{tag}/loss{step}"]).max() < 2e-5, (step, got, g[f"{tag}/loss{step}"])
    sd = tr.state_dict()
    tr.release()
    tol = 6e-6 if tag == "ref" else 3e-5
    worst = 0.0
    for k in g.files:
        if k.startswith(f"{tag}/post/") and not k.endswith("num_batches_tracked"):
            name = k[len(tag) + 6:]
            d = np.abs(sd[name].numpy().astype(np.float64) - g[k]).max()
            worst = max(worst, d)
            assert d < tol, (name, d)
    print(f"AdamW focal_dice {tag}: worst post-step difference {worst:.2e} (tolerance {tol:.0e})")


def test_validate_reports_the_general_loss():
    """validate() under focal_dice over three batches: loss, bce, dice_loss and focal are the means of what
    unet_op_loss_grad gives per batch for the same logits - exactly, the sums come from the same code; the confusion
    counts and the Dice score equal the existing entry point's; uint8 0 / 255 and float 0 / 1 targets agree."""
    L, lib = _lib()
    feats, n, hh, ww = [16, 32], 2, 32, 32
    tr = _trainer(feats, seed=6, lr=1e-3)
    tr.set_loss("focal_dice")
    for i in range(2):
        tr.step(torch.from_numpy(S.synthetic_frames(n, hh, ww, seed=20 + i)),
                torch.from_numpy(S.synthetic_targets(n, hh, ww, seed=20 + i)))
    batches = [(torch.from_numpy(S.synthetic_frames(n, hh, ww, seed=40 + i)),
                torch.from_numpy(S.synthetic_targets(n, hh, ww, seed=40 + i))) for i in range(3)]
    m, logits = tr.validate(batches, return_logits=True)
    per = []
    for (_, tb), lg in zip(batches, logits):
        terms, _ = op_loss_grad(lg.reshape(-1).contiguous(), tb.cuda().float().reshape(-1).contiguous(),
                                0.0, 0.5, 0.5, 3.0, 0.25, 2.0)
        per.append(terms.cpu().numpy().astype(np.float64))
    per = np.asarray(per)
    assert m.batches == 3 and m.pixels == 3 * n * hh * ww
    assert (m.loss, m.bce, m.dice_loss, m.focal) == tuple(per[:, k].sum() / 3 for k in range(4)), (m.as_dict(), per)
    assert m.focal > 0 and abs(m.loss - (0.5 * m.focal + 0.5 * m.dice_loss)) < 1e-6
    # the existing entry point on the same logits: counts and Dice score
    acc = torch.zeros(metrics.NUM_ACCUMULATORS, dtype=torch.float64, device="cuda")
    for (_, tb), lg in zip(batches, logits):
        metrics.accumulate(lib, 0, lg, tb, acc, C.c_void_p(torch.cuda.current_stream(tr.device).cuda_stream), loss_cfg=None)
    torch.cuda.synchronize()
    old = metrics.SegMetrics(acc.cpu().numpy())
    assert (m.tp, m.fp, m.fn, m.tn) == (old.tp, old.fp, old.fn, old.tn) and m.dice == old.dice and old.focal == 0.0
    assert m.tp + m.fn == int(sum(float(tb.sum()) for _, tb in batches))
    # uint8 masks
    m8 = tr.validate([(fb, (tb * 255).to(torch.uint8)) for fb, tb in batches])
    assert m8.as_dict() == m.as_dict()
    # a validation pass under the older kinds keeps going through the older entry point
    tr.set_loss("bce_dice", 0.5, 0.5, 3.0)
    mo = tr.validate(batches)
    assert mo.focal == 0.0 and (mo.tp, mo.fp, mo.fn, mo.tn) == (m.tp, m.fp, m.fn, m.tn)
    tr.release()


def test_training_with_focal_dice_reduces_loss():
    """test_training_reduces_loss (tests/test_train_gpu.py) under focal_dice, with its criterion: ten Adam steps on one
    fixed batch take the loss below 0.9 of its first value.  (torch.optim.Adam on the CPU oracle, same weights and
    batch, reaches 0.74 of it.)"""
    tr = _trainer([16, 32, 64], seed=8, lr=1e-3)
    tr.set_loss("focal_dice")
    frames = torch.from_numpy(S.synthetic_frames(4, 32, 32, seed=4))
    tgt = torch.from_numpy(S.synthetic_targets(4, 32, 32, seed=4))
    losses = [float(tr.step(frames, tgt).item()) for _ in range(10)]
    print("focal_dice training losses:", losses)
    assert losses[-1] < losses[0] * 0.9, losses
    tr.release()
