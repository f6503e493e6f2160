"""Validation pass on the training handle: eval-mode forward (unet_train_eval_*), the device reduction of the
segmentation metrics and the validation loss (unet_seg_metrics_accumulate), UNetTrainer.validate and UNetHIP.evaluate,
against the CPU oracle, the committed goldens and the reference's own validate() (tests/golden/make_golden_val.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from unet_lane_detection_amd import metrics, state as S

pytestmark = pytest.mark.gpu

# the configurations of tests/test_train_gpu.py::test_mid_config_grads_vs_oracle: the exact-fp32 path, planes mode, the
# split-operand path without planes, a width that is not a multiple of 16
MID_CONFIGS = [([16, 32, 64], (3, 24, 32)), ([8, 16], (2, 32, 48)), ([32, 64], (5, 28, 28)), ([16, 32, 64], (3, 48, 64)),
               ([64, 128], (2, 32, 48)), ([64, 128, 256], (1, 16, 32)), ([64, 128], (1, 16, 40)), ([64, 128], (2, 28, 28))]
PLANES_CONFIG = ([64, 128], (2, 32, 48))
NARROW_CONFIG = ([8, 16], (2, 32, 48))


def _lib():
    from unet_lane_detection_amd import _lib as L
    return L.load(build_if_missing=False)


@pytest.fixture(params=[1, 0], ids=["f16x3_convs", "fp32_convs"])
def train_conv_mode(request):
    """Both settings of unet_set_train_x3."""
    lib = _lib()
    prev = lib.unet_set_train_x3(request.param)
    yield request.param
    lib.unet_set_train_x3(prev)


def _round_shape(feats, shape):
    n, hh, ww = shape
    m = 1 << len(feats)
    return n, hh // m * m, ww // m * m


def _stepped_trainer(feats, shape, steps=2, seed=6, loss=None):
    """Trainer from seeded weights after `steps` optimizer steps: parameters, operand packs and running statistics
    that no host code has seen."""
    from unet_lane_detection_amd.trainer import UNetTrainer
    n, hh, ww = _round_shape(feats, shape)
    tr = UNetTrainer(S.seeded_state_dict(feats, seed=seed), device=0, lr=1e-3)
    if loss:
        tr.set_loss(*loss)
    for i in range(steps):
        tr.step(torch.from_numpy(S.synthetic_frames(n, hh, ww, seed=20 + i)),
                torch.from_numpy(S.synthetic_targets(n, hh, ww, seed=20 + i)))
    return tr, (n, hh, ww)


# ---- 1. eval logits against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("feats,shape", MID_CONFIGS)
def test_eval_logits_vs_oracle_after_two_steps(feats, shape, train_conv_mode):
    tr, (n, hh, ww) = _stepped_trainer(feats, shape)
    frames = S.synthetic_frames(n, hh, ww, seed=5)
    sd_t = O.to_torch_state(tr.state_dict())
    with torch.no_grad():
        ref = O.forward(sd_t, O.normalize_u8_nhwc(frames), training=False)
    got = tr.eval_logits(torch.from_numpy(frames)).cpu()
    assert tr.device_error() == 0
    err = (got - ref).abs().max().item()
    print("eval logits vs oracle: max |d| %.3e (feats %s, %s)" % (err, feats, "f16x3" if train_conv_mode else "fp32"))
    assert err < 1e-4, err
    tr.release()


# ---- 2. model A against the committed golden ----------------------------------------------------------------------
def test_modelA_validate_vs_reference_golden(golden_dir, train_conv_mode):
    from unet_lane_detection_amd.trainer import UNetTrainer
    g = np.load(os.path.join(golden_dir, "modelA_frame_001410.npz"))
    frame = np.fromfile(os.path.join(golden_dir, "frame_001410_rgb_u8.bin"), dtype=np.uint8).reshape(1, 224, 224, 3)
    tr = UNetTrainer(S.seeded_state_dict(seed=0), device=0)
    tr.profile(True)
    target = torch.from_numpy(g["mask"].reshape(1, 1, 224, 224))          # uint8 0 / 255
    m, logits = tr.validate([(torch.from_numpy(frame), target)], return_logits=True)
    names = [r[0] for r in tr.profile_records()]
    tr.profile(False)
    # per-launch profiling labels the eval launches: 17 of the 18 convolutions on the split-operand kernels, no
    # statistics or BatchNorm passes behind them
    assert names.count("eval_bn_fold") == 1, names
    assert names.count("eval_conv3x3_f16x3") + names.count("eval_conv3x3_pool_f16x3") == (17 if train_conv_mode else 0), names
    assert "bn_stats" not in names and ("bn_apply_relu" not in names)
    lg = logits[0].cpu().numpy()[0, 0]
    err = np.abs(lg - g["logits"]).max()
    print("model A eval on the reference frame: max |dlogit| %.3e" % err)
    assert err < 2e-4, err
    sure = np.abs(g["logits"]) > 2e-4
    mask = O.logits_to_mask(lg)
    assert np.array_equal(mask[sure], g["mask"][sure])                   # identical mask off ties
    assert m.fp + m.fn <= int((~sure).sum())
    assert m.pixels == 224 * 224 and m.batches == 1
    tr.release()


# ---- 3. agreement with the inference handle ----------------------------------------------------------------------
@pytest.mark.parametrize("feats,shape", [PLANES_CONFIG, NARROW_CONFIG, ([64, 128], (2, 28, 28))])
def test_eval_agrees_with_inference_handle(feats, shape):
    from unet_lane_detection_amd.model import UNetHIP
    tr, (n, hh, ww) = _stepped_trainer(feats, shape)
    x = O.normalize_u8_nhwc(S.synthetic_frames(n, hh, ww, seed=5))       # the float entry point
    got = tr.eval_logits(x)
    net = UNetHIP(tr.state_dict(), device=0)
    ref = net.forward(x.cuda(), precision="fp32")
    err = (got - ref).abs().max().item()
    print("eval vs UNetHIP fp32: max |d| %.3e" % err)
    assert err < 2e-4, err
    net.release()
    tr.release()


# ---- 4. validation leaves no trace ---------------------------------------------------------------------------------
def _snapshot(tr):
    return {k: getattr(tr, k).clone() for k in ("params", "bn", "grads", "exp_avg", "exp_avg_sq")}, \
        (tr.step_count, tr.num_batches_tracked)


@pytest.mark.parametrize("feats,shape", [PLANES_CONFIG, NARROW_CONFIG], ids=["planes", "narrow"])
def test_validate_leaves_no_trace(feats, shape):
    from unet_lane_detection_amd.trainer import UNetTrainer
    lib = _lib()
    prev_side = lib.unet_set_train_side(1)
    try:
        n, hh, ww = _round_shape(feats, shape)
        loss = ("bce_dice", 0.5, 0.5, 3.0)
        batches = [(torch.from_numpy(S.synthetic_frames(n, hh, ww, seed=30 + i)),
                    torch.from_numpy(S.synthetic_targets(n, hh, ww, seed=30 + i))) for i in range(2)]
        # validation batches of the training shape and of a larger one (the workspace grows)
        val = [(torch.from_numpy(S.synthetic_frames(n, hh, ww, seed=40)),
                torch.from_numpy(S.synthetic_targets(n, hh, ww, seed=40))),
               (torch.from_numpy(S.synthetic_frames(n + 1, hh, ww, seed=41)),
                torch.from_numpy((S.synthetic_targets(n + 1, hh, ww, seed=41) * 255).astype(np.uint8)))]
        a = UNetTrainer(S.seeded_state_dict(feats, seed=6), device=0, lr=1e-3)
        b = UNetTrainer(S.seeded_state_dict(feats, seed=6), device=0, lr=1e-3)
        a.set_loss(*loss)
        b.set_loss(*loss)
        la = [a.step(*batches[0]).clone()]
        lb = [b.step(*batches[0]).clone()]
        before, counters = _snapshot(b)
        m = b.validate(val)
        torch.cuda.synchronize()
        after, counters_after = _snapshot(b)
        assert counters == counters_after
        for k in before:
            assert torch.equal(before[k], after[k]), k
        assert m.batches == 2 and m.pixels == (2 * n + 1) * hh * ww and 0.0 < m.loss < 10.0
        la.append(a.step(*batches[1]).clone())
        lb.append(b.step(*batches[1]).clone())
        torch.cuda.synchronize()
        for k in ("params", "bn", "grads", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert torch.equal(torch.cat(la), torch.cat(lb))
        assert torch.equal(a.loss_terms, b.loss_terms)
        assert a.step_count == b.step_count == 2 and a.num_batches_tracked == b.num_batches_tracked == 2
        a.release()
        b.release()
    finally:
        lib.unet_set_train_side(prev_side)


# ---- 5. the metrics kernel against numpy, exact -----------------------------------------------------------------
def _acc_call(lib, logits, targets, acc, thr, loss_cfg):
    metrics.accumulate(lib, 0, logits, targets, acc, C.c_void_p(torch.cuda.current_stream().cuda_stream), threshold=thr,
                       loss_cfg=loss_cfg)


def _np_counts(x, t, thr):
    thr_logit = np.float32(math.log(thr / (1.0 - thr)))       # the float the entry point receives
    pred = x.reshape(-1) > thr_logit
    truth = t.reshape(-1) > 0.5
    return [int((pred & truth).sum()), int((pred & ~truth).sum()), int((~pred & truth).sum()), int((~pred & ~truth).sum())]


@pytest.mark.parametrize("u8", [False, True], ids=["float_targets", "u8_targets"])
@pytest.mark.parametrize("thr", [0.3, 0.5, 0.7])
def test_metrics_kernel_vs_numpy_and_oracle(thr, u8):
    lib = _lib()
    gen = torch.Generator().manual_seed(11)
    sizes = [(3, 37, 53), (1, 224, 224), (5, 61, 7)]           # not multiples of the block size, unequal batches
    loss_cfg = ("bce_dice", 0.5, 0.5, 3.0, 1e-6)
    acc = torch.zeros(16, dtype=torch.float64, device="cuda")
    acc_bce = torch.zeros(16, dtype=torch.float64, device="cuda")
    want = np.zeros(4, dtype=np.int64)
    per = []
    for i, (n, hh, ww) in enumerate(sizes):
        x = torch.randn(n, 1, hh, ww, generator=gen) * 3
        x[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 1e-3, -1e-3])
        t = torch.from_numpy(S.synthetic_targets(n, hh, ww, seed=50 + i))
        td = (t * 255).to(torch.uint8) if u8 else t
        prev = acc.cpu().numpy().copy()
        _acc_call(lib, x.cuda(), td.cuda(), acc, thr, loss_cfg)
        _acc_call(lib, x.cuda(), td.cuda(), acc_bce, thr, None)
        now = acc.cpu().numpy()
        want += np.asarray(_np_counts(x.numpy(), t.numpy(), thr))
        assert [int(v) for v in now[:4]] == list(want), (i, now[:4], want)
        total, bce, dice = O.bce_dice_loss(x, t, 0.5, 0.5, pos_weight=3.0)
        d = now - prev
        print("batch %d: total %.7f (oracle %.7f) bce %.7f (%.7f) dice loss %.7f (%.7f)" %
              (i, d[4], total.item(), d[5], bce.item(), d[6], dice.item()))
        assert abs(d[4] - total.item()) < 2e-5 and abs(d[5] - bce.item()) < 2e-5 and abs(d[6] - dice.item()) < 2e-5
        thr_logit = np.float32(math.log(thr / (1.0 - thr)))
        ref_dice = O.compute_dice(x > float(thr_logit), t)
        print("batch %d: dice %.8f (oracle %.8f)" % (i, d[7], ref_dice.item()))
        assert abs(d[7] - ref_dice.item()) < 1e-6
        per.append((total.item(), ref_dice.item(), O.bce_with_logits(x, t).item()))
        assert now[8] == i + 1 and now[9] == sum(a * b * c for a, b, c in sizes[:i + 1])
        assert not now[10:].any()
    m = metrics.SegMetrics(acc.cpu().numpy())
    per = np.asarray(per)
    assert abs(m.loss - per[:, 0].mean()) < 2e-5 and abs(m.dice - per[:, 1].mean()) < 1e-6
    tp, fp, fn, tn = want
    assert m.iou == tp / (tp + fp + fn) and m.pixel_accuracy == (tp + tn) / want.sum()
    # plain BCE-with-logits (the default loss): total = bce, no dice term
    mb = metrics.SegMetrics(acc_bce.cpu().numpy())
    assert abs(mb.loss - per[:, 2].mean()) < 2e-5 and mb.bce == mb.loss and mb.dice_loss == 0.0
    assert (mb.tp, mb.fp, mb.fn, mb.tn) == (m.tp, m.fp, m.fn, m.tn)


def test_metrics_kernel_all_zero_all_one_and_counts_beyond_2_24():
    lib = _lib()
    n = 64 * 224 * 224                                          # one batch of the flagship shape: 3.2 M pixels
    ones_t = torch.ones(n, device="cuda")
    zeros_t = torch.zeros(n, device="cuda")
    pos = torch.full((n,), 4.0, device="cuda")
    neg = torch.full((n,), -4.0, device="cuda")
    cases = {"tp": (pos, ones_t), "fp": (pos, zeros_t), "fn": (neg, ones_t), "tn": (neg, zeros_t)}
    for i, (name, (x, t)) in enumerate(cases.items()):
        acc = torch.zeros(16, dtype=torch.float64, device="cuda")
        _acc_call(lib, x, t, acc, 0.5, None)
        a = acc.cpu().numpy()
        assert a[i] == n and a[:4].sum() == n, (name, a[:4])
        dice = {"tp": 1.0, "tn": 1.0}.get(name)                  # all-one / all-zero: (2I + s) / (P + T + s)
        if dice is not None:
            assert abs(a[7] - dice) < 1e-6
        else:
            assert a[7] < 1e-9
    # seven such batches into one accumulator, uint8 targets: the pooled count passes 2^24 and is odd
    acc = torch.zeros(16, dtype=torch.float64, device="cuda")
    ones_u8 = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    pos[:1] = -1.0                                               # one false negative per batch
    for _ in range(7):
        _acc_call(lib, pos, ones_u8, acc, 0.5, None)
    a = acc.cpu().numpy()
    assert 7 * (n - 1) > (1 << 24)
    assert (a[0], a[1], a[2], a[3]) == (7 * (n - 1), 0, 7, 0) and a[8] == 7 and a[9] == 7 * n
    assert float(np.float32(a[0])) != a[0]                       # a float32 accumulator could not have held it


# ---- 6. validate end to end against the reference's own function -------------------------------------------------
def test_validate_vs_reference_validate_golden(golden_dir, train_conv_mode):
    from unet_lane_detection_amd.trainer import UNetTrainer
    g = np.load(os.path.join(golden_dir, "tiny_f4_8_validate.npz"), allow_pickle=False)
    assert np.abs(g["logits"]).min() >= 1e-4                     # the fixture's own condition: no tie allowance below
    tr = UNetTrainer(S.seeded_state_dict([4, 8], seed=1), device=0)
    tr.set_loss("bce_dice", 0.5, 0.5, 3.0)
    x, mk = torch.from_numpy(g["input"]), torch.from_numpy(g["mask_u8"])
    batches = [(x[i:i + 2], mk[i:i + 2]) for i in range(0, 6, 2)]
    m, logits = tr.validate(batches, return_logits=True)
    err = (torch.cat(logits).cpu() - torch.from_numpy(g["logits"])).abs().max().item()
    print("tiny validate: avg_loss %.7f (reference %.7f), avg_dice %.8f (reference %.8f), max |dlogit| %.2e" %
          (m.loss, float(g["avg_loss"]), m.dice, float(g["avg_dice"]), err))
    assert err < 1e-4
    assert abs(m.loss - float(g["avg_loss"])) < 2e-5
    assert abs(m.dice - float(g["avg_dice"])) < 1e-6
    assert abs(m.bce - g["batch_bce"].mean()) < 2e-5 and abs(m.dice_loss - g["batch_dice_loss"].mean()) < 2e-5
    # float 0/1 targets give the same numbers as the uint8 masks
    m2 = tr.validate([(a, (b.float() / 255.0)) for a, b in batches])
    assert m2.as_dict() == m.as_dict()
    tr.release()


# ---- 7. counts against the oracle with a stated tie allowance -----------------------------------------------------
def test_validate_counts_vs_oracle_with_tie_allowance():
    feats, (n, hh, ww) = PLANES_CONFIG[0], (4, 64, 96)
    tr, _ = _stepped_trainer(feats, (n, hh, ww))
    sd_t = O.to_torch_state(tr.state_dict())
    tgt = S.synthetic_targets(n, hh, ww, seed=3)
    chosen = None
    for seed in range(2, 2 + 32):                                # a condition on the input, decided on the CPU
        frames = S.synthetic_frames(n, hh, ww, seed=seed)
        with torch.no_grad():
            ref = O.forward(sd_t, O.normalize_u8_nhwc(frames), training=False).numpy()
        ties = int((np.abs(ref) < 1e-4).sum())
        if ties <= 1e-3 * ref.size:
            chosen = (frames, ref, ties)
            break
    if chosen is None:
        pytest.fail("no input among 32 seeds with at most 0.1 % of its pixels within 1e-4 of the threshold")
    frames, ref, ties = chosen
    m = tr.validate([(torch.from_numpy(frames), torch.from_numpy(tgt))])
    want = _np_counts(ref, tgt, 0.5)
    got = [m.tp, m.fp, m.fn, m.tn]
    print("counts %s, oracle %s, %d pixels within 1e-4 of the threshold" % (got, want, ties))
    assert sum(got) == ref.size
    assert max(abs(a - b) for a, b in zip(got, want)) <= ties, (got, want, ties)
    tr.release()


# ---- 8. UNetHIP.evaluate per tier ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def modelA():
    from unet_lane_detection_amd.model import UNetHIP
    net = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    yield net
    net.release()


def _modelA_frames_and_masks(golden_dir):
    g = np.load(os.path.join(golden_dir, "modelA_frame_001410.npz"))
    gs = np.load(os.path.join(golden_dir, "modelA_synth2.npz"))
    frame = np.fromfile(os.path.join(golden_dir, "frame_001410_rgb_u8.bin"), dtype=np.uint8).reshape(1, 224, 224, 3)
    frames = np.concatenate([S.synthetic_frames(2, seed=0), frame])
    logits = np.concatenate([gs["logits"], g["logits"][None]])
    return frames, logits, O.logits_to_mask(logits)


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "bf16"])
def test_unethip_evaluate_per_tier(modelA, golden_dir, precision):
    frames, glogits, gmask = _modelA_frames_and_masks(golden_dir)
    fd = torch.from_numpy(frames).cuda()
    m = modelA.evaluate(fd, torch.from_numpy(gmask), precision=precision, batch=2)
    assert modelA.device_error() == 0
    assert m.batches == 2 and m.pixels == 3 * 224 * 224
    # the same tier's masks on the host: the kernel is under test here, not the tier
    host = torch.cat([modelA.run_u8(fd[i:i + 2], precision=precision) for i in (0, 2)]).cpu().numpy()[:, 0]
    iou = O.mask_iou(O.logits_to_mask(host), gmask)
    print("%s: IoU %.6f precision %.6f recall %.6f" % (precision, m.iou, m.precision, m.recall))
    assert abs(m.iou - iou) < 1e-12
    assert [m.tp, m.fp, m.fn, m.tn] == _np_counts(host, gmask, 0.5)
    if precision in ("fp32", "f16x3"):                            # IoU 1.0 off ties
        ties = int((np.abs(glogits) <= 2e-4).sum())
        assert m.fp + m.fn <= ties
        if ties == 0:
            assert m.iou == 1.0


def test_int8_evaluate_matches_host_masks():
    from unet_lane_detection_amd import quant
    from unet_lane_detection_amd.int8 import UNetInt8, calibrate
    from unet_lane_detection_amd.model import UNetHIP
    feats = [32, 64, 128]
    sdn = S.seeded_state_dict(feats, seed=0)
    fm = UNetHIP(sdn, device=0)
    ranges = calibrate(fm, torch.from_numpy(S.synthetic_frames(6, 64, 64, seed=1)), batch=4)
    net = UNetInt8(quant.quantize_model(sdn, ranges), device=0)
    frames = torch.from_numpy(S.synthetic_frames(3, 64, 64, seed=3)).cuda()
    ref_mask = O.logits_to_mask(fm.run_u8(frames).cpu().numpy()[:, 0])   # the float model's masks as the truth
    m = net.evaluate(frames, torch.from_numpy(ref_mask), batch=2)
    host = net.run_u8(frames).cpu().numpy()[:, 0]
    assert abs(m.iou - O.mask_iou(O.logits_to_mask(host), ref_mask)) < 1e-12
    assert [m.tp, m.fp, m.fn, m.tn] == _np_counts(host, ref_mask, 0.5)
    net.release()
    fm.release()


# ---- 9. errors ----------------------------------------------------------------------------------------------------
def test_eval_errors():
    from unet_lane_detection_amd import _lib as L
    from unet_lane_detection_amd.model import UNetHIP
    from unet_lane_detection_amd.trainer import UNetTrainer
    lib = _lib()
    frames = torch.from_numpy(S.synthetic_frames(1, 32, 32, seed=0)).cuda()
    out = torch.empty(1, 1, 32, 32, device="cuda")
    # a handle nothing is attached to
    net = UNetHIP(S.seeded_state_dict([4, 8], seed=1), device=0)
    rc = lib.unet_train_eval_u8(net._h, C.c_void_p(frames.data_ptr()), 1, 32, 32, C.c_void_p(out.data_ptr()), None)
    assert L.STATUS[rc] == "UNET_ERR_STATE"
    net.release()
    tr = UNetTrainer(S.seeded_state_dict([4, 8], seed=1), device=0)
    # a size the network cannot take (not a multiple of 2^depth)
    rc = lib.unet_train_eval_u8(tr._h, C.c_void_p(frames.data_ptr()), 1, 30, 32, C.c_void_p(out.data_ptr()), None)
    assert L.STATUS[rc] == "UNET_ERR_SHAPE"
    with pytest.raises(L.UnetError) as e:
        tr.eval_logits(torch.zeros(1, 3, 32, 34))
    assert e.value.code == 2
    # the range word set in the error block (nothing on the device is made to fail): validate raises, no metrics
    tgt = torch.from_numpy(S.synthetic_targets(1, 32, 32, seed=0))
    assert L.check(lib.unet_debug_set_error_block(tr._h, 1, 1), "unet_debug_set_error_block") is None
    with pytest.raises(L.UnetError) as e:
        tr.validate([(frames, tgt)])
    assert e.value.code == L.UNET_ERR_RANGE
    # ... reported once: the next pass is clean
    m = tr.validate([(frames, tgt)])
    assert m.batches == 1 and m.pixels == 32 * 32
    tr.release()
