"""The augmentation kernel (unet_augment_u8 behind augment.Augmenter.apply) against the numpy model of
unet_lane_detection_amd/augment.py: np.array_equal on images and on targets, tolerance zero - every step is integer
arithmetic or a fixed sequence of separately rounded IEEE operations.

Shapes: (3, 16x16) a tile smaller than a block, the blur halo folds on all four sides; (5, 37x53) odd, no multiple of
the 32 x 16 tile nor of four pixels, so rows start off dword boundaries; (4, 8x64) the minimum height; (2, 224x224) the
training size.  The model's outputs are computed once per shape and table and shared."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from unet_lane_detection_amd import augment as A

pytestmark = pytest.mark.gpu

SHAPES = [(3, 16, 16), (5, 37, 53), (4, 8, 64), (2, 224, 224)]


def frames(ns, h, w):
    rng = np.random.default_rng(1000 + h * w)
    y, x = np.mgrid[0:h, 0:w]
    img = rng.integers(0, 256, (ns, h, w, 3), dtype=np.uint8)
    # frame 0: smooth saturated gradients (every hue sector, interpolation between unlike neighbours)
    img[0] = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), 255 - ((x + y) * 255) // (h + w - 2)], axis=-1)
    msk = np.zeros((ns, h, w), dtype=np.uint8)
    for i in range(ns):
        msk[i][np.abs(x - w // 3 - (i + 1) * y // 4) <= 1] = 255
    msk[ns - 1] = rng.integers(0, 256, (h, w), dtype=np.uint8)       # values either side of the threshold
    return img, msk


def hand_table(ns):
    """16 records: everything off; each operation alone; everything on with blur 3, 5 and 7; angles -15, 0, +15 and 90;
    flip with and without rotation; extreme alpha / beta and +-30 shifts; source indices repeated and out of order."""
    rows = [  # flip, angle, (alpha, beta) or None, (dh, ds, dv) or None, blur
        (False, 0.0, None, None, 1), (True, 0.0, None, None, 1), (False, 15.0, None, None, 1), (False, -15.0, None, None, 1),
        (False, 90.0, None, None, 1), (True, 15.0, None, None, 1), (False, 0.0, (1.3, 0.3), None, 1),
        (False, 0.0, (0.7, -0.3), None, 1), (False, 0.0, None, (30.0, 30.0, 30.0), 1), (False, 0.0, None, (-30.0, -30.0, -30.0), 1),
        (False, 0.0, None, None, 3), (False, 0.0, None, None, 5), (False, 0.0, None, None, 7),
        (True, -15.0, (1.3, -0.3), (30.0, -30.0, 30.0), 3), (False, 15.0, (0.7, 0.3), (-30.0, 30.0, -30.0), 5),
        (True, 7.3, (1.17, 0.11), (13.7, -21.3, 8.9), 7)]
    src = [ns - 1, 0, 1, 0, ns - 1, 1, 0, 0, 0, ns - 1, 1, 0, ns - 1, 0, 1, ns - 1]
    p = A.identity_params(len(rows), [s % ns for s in src])
    for i, (flip, angle, bc, hsv, blur) in enumerate(rows):
        A.set_geometry(p[i], flip, angle)
        if bc:
            p["flags"][i] |= A.FLAG_BC
            p["alpha"][i], p["beta255"][i] = bc[0], bc[1] * 255.0
        if hsv:
            p["flags"][i] |= A.FLAG_HSV
            p["dh"][i], p["ds"][i], p["dv"][i] = hsv
        p["blur"][i] = blur
    return p


def table(kind, ns):
    if kind == "hand":
        return hand_table(ns)
    # drawn: operations on more often than the defaults, so 12 records exercise every one of them
    aug = A.Augmenter(seed=11, p_brightness_contrast=0.8, p_hsv=0.8, p_blur=0.6)
    return aug.sample_params(12, ns, np.random.default_rng(4).integers(0, ns, 12))


@functools.lru_cache(maxsize=None)
def reference(ns, h, w, kind):
    img, msk = frames(ns, h, w)
    p = table(kind, ns)
    out, tgt = A.apply_model(img, msk, p)
    for a in (img, msk, out, tgt):
        a.setflags(write=False)
    return img, msk, p, out, tgt


def _cuda(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("kind", ["hand", "drawn"])
@pytest.mark.parametrize("ns,h,w", SHAPES)
def test_kernel_equals_model(ns, h, w, kind):
    img, msk, p, want_img, want_tgt = reference(ns, h, w, kind)
    dimg, dmsk = _cuda(img, msk)
    out, tgt = A.Augmenter().apply(dimg, dmsk, p)
    assert out.shape == want_img.shape and tgt.shape == want_tgt.shape and tgt.dtype.is_floating_point
    got_img, got_tgt = out.cpu().numpy(), tgt.cpu().numpy()
    for i in range(p.size):       # per record, so a failure names the operation
        assert np.array_equal(got_img[i], want_img[i]), (i, p[i])
        assert np.array_equal(got_tgt[i], want_tgt[i]), (i, p[i])


def test_images_only_and_preallocated_unaligned_output():
    import torch
    ns, h, w = SHAPES[1]
    img, msk, p, want_img, want_tgt = reference(ns, h, w, "hand")
    dimg, dmsk = _cuda(img, msk)
    out, none = A.Augmenter().apply(dimg, None, p)
    assert none is None and np.array_equal(out.cpu().numpy(), want_img)
    # out=: written in place; a base one byte off a dword boundary moves every row's head and tail bytes
    n = p.size
    raw = torch.full((n * h * w * 3 + 5,), 0xAB, dtype=torch.uint8, device="cuda")
    oimg = raw[1:1 + n * h * w * 3].view(n, h, w, 3)
    otgt = torch.empty((n, 1, h, w), dtype=torch.float32, device="cuda")
    r = A.Augmenter().apply(dimg, dmsk, p, out=(oimg, otgt))
    assert r[0] is oimg and r[1] is otgt
    assert np.array_equal(oimg.cpu().numpy(), want_img) and np.array_equal(otgt.cpu().numpy(), want_tgt)
    edge = raw.cpu().numpy()
    assert edge[0] == 0xAB and (edge[-4:] == 0xAB).all()          # nothing written outside the samples


def test_golden_fixture_through_the_kernel(golden_dir):
    g = np.load(os.path.join(golden_dir, "augment.npz"))
    params = np.frombuffer(g["params"].tobytes(), dtype=A.PARAMS_DTYPE).copy()
    dimg, dmsk = _cuda(g["images"], g["masks"])
    out, tgt = A.Augmenter(mask_threshold=int(g["mask_threshold"])).apply(dimg, dmsk, params)
    assert np.array_equal(out.cpu().numpy(), g["out_images"]) and np.array_equal(tgt.cpu().numpy(), g["out_targets"])


def test_abi_rejects_bad_arguments():
    import torch
    from unet_lane_detection_amd import _lib
    lib = _lib.load()
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(img)
    (tab,) = _cuda(A.identity_params(1).view(np.uint8))

    def ptr(t):
        return C.c_void_p(t.data_ptr())
    assert lib.unet_augment_u8(0, None, None, 1, 8, 8, ptr(tab), 1, 127, ptr(out), None, None) != 0
    assert lib.unet_augment_u8(0, ptr(img), None, 1, 8, 8, ptr(tab), 0, 127, ptr(out), None, None) != 0
    assert lib.unet_augment_u8(0, ptr(img), None, 1, 7, 8, ptr(tab), 1, 127, ptr(out), None, None) != 0
    assert lib.unet_augment_u8(0, ptr(img), None, 1, 8, 8, ptr(tab), 1, 127, ptr(out), None, None) == 0
    torch.cuda.synchronize()
    assert lib.unet_augment_param_bytes() == A.PARAMS_DTYPE.itemsize


def test_python_rejects_bad_tables():
    dimg, dmsk = _cuda(*frames(3, 16, 16))
    p = A.identity_params(2)
    p["src"][1] = 3
    with pytest.raises(ValueError):
        A.Augmenter().apply(dimg, dmsk, p)
    p = A.identity_params(2)
    p["blur"][0] = 4
    with pytest.raises(ValueError):
        A.Augmenter().apply(dimg, dmsk, p)
    with pytest.raises(TypeError):
        A.Augmenter().apply(dimg.cpu(), dmsk.cpu(), A.identity_params(2))     # host tensors: neither path


def test_batches_and_fit_end_to_end():
    import math

    from unet_lane_detection_amd import state as S
    from unet_lane_detection_amd.metrics import SegMetrics
    from unet_lane_detection_amd.trainer import UNetTrainer
    n, size, batch = 12, 32, 4
    img, msk = frames(n, size, size)
    ds = A.DeviceDataset(img, msk, device=0)
    assert len(ds) == n and ds.images.is_cuda and ds.masks.shape == (n, size, size)
    # all probabilities 0: exactly the permuted raw frames and the thresholded masks
    off = A.Augmenter(seed=5, p_flip=0, p_rotate=0, p_brightness_contrast=0, p_hsv=0, p_blur=0)
    ab = A.AugmentedBatches(ds, batch, off)
    got = [(i.cpu().numpy(), t.cpu().numpy()) for i, t in ab()]
    order = ab.last_order
    assert sorted(order.tolist()) == list(range(n)) and len(got) == 3
    assert np.array_equal(np.concatenate([g[0] for g in got]), img[order])
    assert np.array_equal(np.concatenate([g[1] for g in got])[:, 0], (msk[order] > 127).astype(np.float32))
    # the defaults: one epoch of fit with the validation batches
    tr = UNetTrainer(S.seeded_state_dict([4, 8], seed=1), device=0, lr=1e-3)
    hist = tr.fit(A.AugmentedBatches(ds, batch, A.Augmenter(seed=6)), A.val_batches(ds, batch), epochs=1)
    assert len(hist) == 1 and math.isfinite(hist[0]["train_loss"]) and isinstance(hist[0]["val"], SegMetrics)
    assert hist[0]["val"].pixels == n * size * size and hist[0]["val"].batches == 3
    assert tr.device_error() == 0
    tr.release()
