"""K-class models on the int8 tier, on the GPU (csrc/i8_classes_kernels.h): the forward bit-exact against the integer
oracle (oracle/int8_oracle.py, one call per class: tests/int8_classes_model.py), the hybrid head within the derived bound of
quant.hybrid_bound, the calibration of a K-class float model, compare_outputs, evaluate_classes, the video pipeline, and
the single-class head left as it was.

Labels are compared on every pixel: the logits are exact, so np.argmax (first maximum) and the device's tie rule (lowest
class) agree everywhere."""
import numpy as np
import pytest
import torch

from int8_classes_model import sliced_reference, softmax64
from oracle import int8_oracle as Q
from unet_lane_detection_amd import _lib, quant, state as S

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # fp32 unit roundoff
# (features, K, n, H, W): both narrow-layer int8 paths (32- and 64-channel levels), a block that is not full, a pixel
# count that is no multiple of 256, the largest K
CASES = [([32, 64], 3, 2, 16, 32), ([32, 64], 2, 1, 8, 12), ([32, 64, 128], 8, 3, 16, 24), ([64, 128], 4, 2, 16, 20)]

_made = {}


def made(i):
    """(state dict, frames, ranges, quantised model, oracle logits) of case i, built once"""
    if i not in _made:
        feats, k, n, h, w = CASES[i]
        sd = S.seeded_state_dict(feats, seed=k, out_channels=k)
        frames = S.synthetic_frames(n, h, w, seed=10 + k)
        ranges = Q.float_ranges(sd, frames)
        qm = quant.quantize_model(sd, ranges)
        ref = sliced_reference(qm, frames)
        ref.setflags(write=False)
        _made[i] = (sd, frames, ranges, qm, ref)
    return _made[i]


def _classes_direct(net, frames, want, mask_class):
    """unet_i8_forward_classes_u8 with exactly the outputs of `want`; every buffer is pre-filled"""
    n, h, w, _ = frames.shape
    k = net.out_channels
    out = {}
    for name in want:
        if name in ("logits", "probs"):
            out[name] = torch.full((n, k, h, w), float("nan"), device="cuda")
        else:
            out[name] = torch.full((n, h, w), 77, dtype=torch.uint8, device="cuda")
    p = _lib.ptr
    rc = net._lib.unet_i8_forward_classes_u8(net._h, p(frames), n, h, w, p(out.get("logits")), p(out.get("probs")),
                                             p(out.get("labels")), mask_class, p(out.get("mask")), _lib.stream(net.device))
    net._check(rc, "unet_i8_forward_classes_u8")
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{'-'.join(map(str, c[0]))}-K{c[1]}-{c[2]}x{c[3]}x{c[4]}" for c in CASES])
def test_k_class_forward_is_bit_exact(i):
    from unet_lane_detection_amd.int8 import UNetInt8
    feats, k, n, h, w = CASES[i]
    _, frames, _, qm, ref = made(i)
    net = UNetInt8(qm, device=0)
    try:
        assert net.out_channels == k
        fd = torch.from_numpy(frames).cuda()
        c = k - 1
        logits, probs, labels, mask = (t.cpu().numpy() for t in net.run_u8(fd, return_probs=True, return_labels=True, mask_class=c))
        assert logits.shape == (n, k, h, w) and labels.shape == (n, h, w) and mask.shape == (n, h, w)
        assert np.array_equal(logits, ref), f"{(logits != ref).sum()} of {ref.size} logits differ, max {np.abs(logits - ref).max()}"
        assert labels.dtype == np.uint8 and np.array_equal(labels, np.argmax(ref, 1))
        assert np.array_equal(mask, np.where(labels == c, 255, 0).astype(np.uint8))
        err = np.abs(probs.astype(np.float64) - softmax64(ref))
        print(f"softmax: largest error {err.max() / U:.2f} U")
        assert err.max() <= 4 * U
        # an output does not depend on the others: labels alone and the mask alone write one byte per pixel
        for want in (("labels",), ("mask",), ("logits",), ("probs",), ("labels", "mask")):
            got = _classes_direct(net, fd, want, c)
            for name in want:
                assert np.array_equal(got[name], {"logits": logits, "probs": probs, "labels": labels, "mask": mask}[name]), want
        assert np.array_equal(net.predict_labels(fd).cpu().numpy(), labels)
        # the head alone, on the tensor the forward left behind
        lab2 = torch.full((n, h, w), 77, dtype=torch.uint8, device="cuda")
        net._check(net._lib.unet_i8_run_head(net._h, None, None, _lib.ptr(lab2), 0, None, 0.0, _lib.stream(net.device)), "run_head")
        assert np.array_equal(lab2.cpu().numpy(), labels)
        for other in range(k - 1):
            assert np.array_equal(net.run_u8(fd, mask_class=other)[1].cpu().numpy(), np.where(labels == other, 255, 0))
    finally:
        net.release()


# ---- hybrid ---------------------------------------------------------------------------------------------------------
def _check_hybrid_head(net, qm, frames, ref_int8):
    n, h, w, _ = frames.shape
    d = len(qm["features"])
    fd = torch.from_numpy(frames).cuda()
    logits, probs, labels, mask = (t.cpu().numpy() for t in net.run_u8(fd, return_probs=True, return_labels=True, mask_class=1))
    x = net.read_tensor(f"dec{d - 1}.b", n, h, w)                 # the device's own input of the head
    out = quant.unit_model(qm, "output", x)
    assert out["dtype"] == "fp32" and logits.shape == out["v"].shape
    bound = quant.hybrid_bound(out)
    excess = np.abs(logits.astype(np.float64) - out["v"]) - bound
    assert int((excess > 0).sum()) == 0, f"{int((excess > 0).sum())} of {logits.size} logits outside the bound, worst by {excess.max():.3g}"
    # the other outputs follow from the device's own logits
    assert np.array_equal(labels, np.argmax(logits, 1)) and np.array_equal(mask, np.where(labels == 1, 255, 0))
    assert np.abs(probs.astype(np.float64) - softmax64(logits)).max() <= 4 * U
    assert not np.array_equal(logits, ref_int8)                   # the mark is honoured
    return x


def test_hybrid_k_class_head():
    from unet_lane_detection_amd.int8 import UNetInt8
    feats, k, n, h, w = CASES[0]
    sd, frames, ranges, qm_int8, ref = made(0)
    # the head alone hybrid: it reads an int8 tensor
    qm = quant.quantize_model(sd, ranges, hybrid=("output",))
    net = UNetInt8(qm, device=0)
    try:
        assert net.out_channels == k and net.tensor_dtype("dec1.b") == "int8"
        x = _check_hybrid_head(net, qm, frames, ref)
        assert x.dtype == np.int8
    finally:
        net.release()
    # every unit hybrid: it reads an fp16 tensor
    qa = quant.quantize_model(sd, ranges, hybrid=quant.unit_names(feats))
    net = UNetInt8(qa, device=0)
    try:
        assert net.tensor_dtype("dec1.b") == "fp16"
        x = _check_hybrid_head(net, qa, frames, ref)
        assert x.dtype == np.float32
    finally:
        net.release()
    # the hybrid file as pure int8: the pure model, and the oracle
    pure = UNetInt8(qa, device=0, hybrid=False)
    try:
        got = pure.run_u8(torch.from_numpy(frames).cuda()).cpu().numpy()
        assert all(pure.tensor_dtype(t) == "int8" for t in quant.tensor_names(len(feats)))
    finally:
        pure.release()
    assert np.array_equal(got, ref)


# ---- calibration ----------------------------------------------------------------------------------------------------
def test_calibration_of_a_k_class_model_is_that_of_its_body():
    from unet_lane_detection_amd.int8 import calibrate
    from unet_lane_detection_amd.model import UNetHIP
    feats, k = [32, 64], 3
    sdk = S.seeded_state_dict(feats, seed=0, out_channels=k)
    sd1 = S.seeded_state_dict(feats, seed=0)
    body = [key for key in sd1 if not key.startswith("output.")]
    assert all(np.array_equal(np.asarray(sdk[key]), np.asarray(sd1[key])) for key in body)
    frames = torch.from_numpy(S.synthetic_frames(5, 32, 48, seed=2))
    fk, f1 = UNetHIP(sdk, device=0), UNetHIP(sd1, device=0)
    try:
        assert fk.out_channels == k
        rk, r1 = calibrate(fk, frames, batch=2), calibrate(f1, frames, batch=2)
        assert rk == r1                                                     # exact: the same floats
        ref = Q.float_ranges(sdk, frames.numpy())
        assert set(rk) == set(ref)
        for name in ref:                                                    # the bound of tests/test_int8_gpu.py
            span = ref[name][1] - ref[name][0]
            assert abs(rk[name][0] - ref[name][0]) < 1e-4 * span + 1e-5, (name, rk[name], ref[name])
            assert abs(rk[name][1] - ref[name][1]) < 1e-4 * span + 1e-5, (name, rk[name], ref[name])
        (mk, hk), (m1, h1) = (calibrate(m, frames, batch=2, algorithm="mmse", return_histograms=True) for m in (fk, f1))
        assert mk == m1 and set(hk) == set(h1)
        for name in hk:
            assert np.array_equal(hk[name][0], h1[name][0]) and hk[name][1:] == h1[name][1:], name
    finally:
        fk.release()
        f1.release()


# ---- the Python layer -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    """The K-class fp32 tier and its int8 model (case 0's weights), calibrated on the device"""
    from unet_lane_detection_amd.int8 import UNetInt8, calibrate
    from unet_lane_detection_amd.model import UNetHIP
    sd = made(0)[0]
    fm = UNetHIP(sd, device=0)
    ranges = calibrate(fm, torch.from_numpy(S.synthetic_frames(6, 64, 64, seed=1)), batch=6)
    net = UNetInt8(quant.quantize_model(sd, ranges), device=0)
    yield fm, net
    net.release()
    fm.release()


def test_compare_outputs_on_softmax_tensors(pair):
    from unet_lane_detection_amd.int8 import compare_outputs
    fm, net = pair
    frames = torch.from_numpy(S.synthetic_frames(3, 32, 32, seed=9)).cuda()
    cmp = compare_outputs(fm, net, frames, batch=2)
    pf = fm.run_u8(frames, return_probs=True)[1].cpu().numpy().astype(np.float64)
    pq = net.run_u8(frames, return_probs=True)[1].cpu().numpy().astype(np.float64)
    assert pf.shape == (3, 3, 32, 32)
    want = np.abs(pf - pq).reshape(3, -1).mean(axis=1)
    print(cmp)
    assert np.abs(cmp.per_frame - want).max() <= 1e-6
    assert cmp.grade == "GOOD"


def _confusion(pred, truth, k, ignore=None):
    keep = truth < k
    if ignore is not None:
        keep &= truth != ignore
    return np.bincount(truth[keep].astype(np.int64) * k + pred[keep], minlength=k * k).reshape(k, k)


def test_evaluate_classes_equals_a_numpy_confusion_matrix(pair):
    fm, net = pair
    k = 3
    frames = torch.from_numpy(S.synthetic_frames(5, 32, 32, seed=12)).cuda()
    rng = np.random.default_rng(4)
    truth = rng.integers(0, k, size=(5, 32, 32)).astype(np.uint8)
    truth[rng.random(truth.shape) < 0.1] = 255
    tq = torch.from_numpy(truth)
    for model, labels in ((net, net.run_u8(frames, return_labels=True)[1]), (fm, fm.run_u8(frames, return_labels=True)[1])):
        pred = labels.cpu().numpy()
        for ignore in (None, 255):
            m = model.evaluate_classes(frames, tq, batch=2, ignore_index=ignore)
            want = _confusion(pred, truth, k, ignore)
            assert np.array_equal(m.counts, want), (type(model).__name__, ignore)
            tp = np.diag(want).astype(np.float64)
            den = want.sum(0) + want.sum(1) - tp
            assert np.allclose(m.iou, np.where(den == 0, 1.0, tp / np.maximum(den, 1)), rtol=0, atol=1e-15)
            assert m.miou == float(m.iou.mean()) and abs(m.pixel_acc - np.trace(want) / want.sum()) <= 1e-15
    with pytest.raises(ValueError):
        net.evaluate_classes(frames, tq.to(torch.float32))


def test_frame_pipeline_takes_the_class_mask(pair):
    from unet_lane_detection_amd.video import FramePipeline
    _, net = pair
    rng = np.random.default_rng(5)
    frames = torch.from_numpy(rng.integers(0, 256, size=(2, 48, 64, 3), dtype=np.uint8)).cuda()
    pipe = FramePipeline(net, mask_class=1, input_size=(32, 32))
    overlay, mask = pipe.process(frames)
    small = pipe._resize(frames)
    by_hand = net.run_u8(small, mask_class=1)[-1]
    assert by_hand.shape == (2, 32, 32) and by_hand.dtype == torch.uint8 and 0 < int((by_hand == 255).sum()) < by_hand.numel()
    o2, m2 = torch.empty_like(frames), torch.empty(frames.shape[:3], dtype=torch.uint8, device="cuda")
    pipe._overlay(frames, by_hand, o2, m2)
    torch.cuda.synchronize()
    assert torch.equal(overlay, o2) and torch.equal(mask, m2)
    host = list(pipe.run([frames.cpu().numpy()]))
    assert len(host) == 1 and np.array_equal(host[0][0], o2.cpu().numpy()) and np.array_equal(host[0][1], m2.cpu().numpy())


def test_single_class_model_runs_what_it_ran():
    """The head dispatch: a quantised model with one row goes through head_i8_kernel as before"""
    from unet_lane_detection_amd.int8 import UNetInt8
    feats, _, n, h, w = CASES[0]
    sd = S.seeded_state_dict(feats, seed=0)
    frames = S.synthetic_frames(n, h, w, seed=3)
    qm = quant.quantize_model(sd, Q.float_ranges(sd, frames))
    ref = Q.forward(qm, frames)
    net = UNetInt8(qm, device=0)
    try:
        assert net.out_channels == 1
        fd = torch.from_numpy(frames).cuda()
        logits, probs, mask = net.run_u8(fd, return_probs=True, return_mask=True)
        assert np.array_equal(logits.cpu().numpy(), ref)
        assert np.array_equal(mask.cpu().numpy(), ((ref[:, 0] > 0) * 255).astype(np.uint8))
        assert np.abs(probs.cpu().numpy() - 1 / (1 + np.exp(-ref.astype(np.float64)))).max() < 1e-6
        # the head alone writes the same bits
        l2, p2, m2 = torch.empty_like(logits), torch.empty_like(probs), torch.empty_like(mask)
        p = _lib.ptr
        net._check(net._lib.unet_i8_run_head(net._h, p(l2), p(p2), None, 0, p(m2), 0.0, _lib.stream(net.device)), "run_head")
        assert torch.equal(l2, logits) and torch.equal(p2, probs) and torch.equal(m2, mask)
        with pytest.raises(ValueError):
            net.run_u8(fd, return_labels=True)
        with pytest.raises(_lib.UnetError, match="single-class"):
            net._check(net._lib.unet_i8_forward_classes_u8(net._h, p(fd), n, h, w, p(l2), None, None, 0, None, None), "classes")
    finally:
        net.release()
