"""The augmentation stage on the host: the parameter table, the numpy model of every operation (the specification the
kernel is held to in tests/test_augment_gpu.py), the committed fixture that pins the model, and the batch iterables."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from unet_lane_detection_amd import augment as A
from unet_lane_detection_amd import loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    msk = (rng.integers(0, 256, (n, h, w), dtype=np.uint8))
    return img, msk


# ---- parameter table ------------------------------------------------------------------------------------------
def test_same_seed_same_table_other_seed_other_table():
    a = A.Augmenter(seed=7).sample_params(64, 10)
    b = A.Augmenter(seed=7).sample_params(64, 10)
    c = A.Augmenter(seed=8).sample_params(64, 10)
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert a.dtype == A.PARAMS_DTYPE and a.dtype.itemsize == 80
    assert np.array_equal(a["src"], np.arange(64) % 10)
    idx = np.array([3, 3, 0, 9])
    assert np.array_equal(A.Augmenter(seed=1).sample_params(4, 10, idx)["src"], idx)
    # one stream: the second table of an augmenter differs from its first
    aug = A.Augmenter(seed=7)
    assert aug.sample_params(64, 10).tobytes() != aug.sample_params(64, 10).tobytes()


def test_limits_and_enable_counts():
    n = 4000
    p = A.Augmenter(seed=123).sample_params(n, 5)
    angle = np.degrees(np.arctan2(p["m"][:, 3], p["m"][:, 4]))       # row 1 is (sin, cos) with or without the flip
    assert (np.abs(angle) <= 15.0 + 1e-9).all() and np.abs(angle).max() > 10.0
    assert (np.abs(p["alpha"] - 1.0) <= 0.3 + 1e-6).all() and (np.abs(p["beta255"] / 255.0) <= 0.3 + 1e-6).all()
    assert (np.abs(p["dh"]) <= 30).all() and (np.abs(p["ds"]) <= 30).all() and (np.abs(p["dv"]) <= 30).all()
    assert set(np.unique(p["blur"])) == {1, 3, 5, 7}
    flip, rot = (p["flags"] & A.FLAG_FLIP) != 0, (p["flags"] & A.FLAG_ROTATE) != 0
    assert np.array_equal(flip, p["m"][:, 0] < 0) and np.array_equal(rot, angle != 0)
    bc, hsv, blur = (p["flags"] & A.FLAG_BC) != 0, (p["flags"] & A.FLAG_HSV) != 0, p["blur"] > 1
    # five binomial standard deviations: 158 for p = 0.5, 145 for 0.7 and 0.3
    for on, prob, tol in ((flip, 0.5, 158), (rot, 0.5, 158), (bc, 0.7, 145), (hsv, 0.7, 145), (blur, 0.3, 145)):
        assert tol == round(5 * math.sqrt(n * prob * (1 - prob)))
        assert abs(int(on.sum()) - n * prob) <= tol
    # a switched-off operation leaves neutral parameters; the sizes of a switched-on blur are spread over 3, 5, 7
    assert (p["alpha"][~bc] == 1).all() and (p["beta255"][~bc] == 0).all() and (p["dh"][~hsv] == 0).all()
    sizes = np.bincount(p["blur"][blur], minlength=8)[[3, 5, 7]]
    assert (np.abs(sizes - blur.sum() / 3) <= 5 * math.sqrt(blur.sum() * 2 / 9)).all()


def test_record_size_matches_the_library():
    from unet_lane_detection_amd import _lib
    lib = _lib.load()
    assert lib.unet_augment_param_bytes() == A.PARAMS_DTYPE.itemsize
    # the argument checks come before any device call
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    assert lib.unet_augment_u8(0, None, None, 1, 16, 16, p, 1, 127, p, None, None) != 0
    assert lib.unet_augment_u8(0, p, None, 1, 16, 16, p, 0, 127, p, None, None) != 0
    assert lib.unet_augment_u8(0, p, None, 0, 16, 16, p, 1, 127, p, None, None) != 0
    assert lib.unet_augment_u8(0, p, None, 1, 7, 16, p, 1, 127, p, None, None) != 0
    assert lib.unet_augment_u8(0, p, None, 1, 16, 7, p, 1, 127, p, None, None) != 0
    assert lib.unet_augment_u8(0, p, p, 1, 16, 16, p, 1, 127, p, None, None) != 0     # masks without targets


def test_table_validation():
    img, msk = _frames(3, 8, 8, 0)
    for field, value in (("src", 3), ("src", -1), ("blur", 4), ("blur", 9), ("dh", np.nan), ("alpha", np.inf)):
        p = A.identity_params(2)
        p[field][1] = value
        with pytest.raises(ValueError):
            A.apply_model(img, msk, p)
    p = A.identity_params(2)
    p["m"][0, 2] = np.inf
    with pytest.raises(ValueError):
        A.apply_model(img, msk, p)
    with pytest.raises(ValueError):
        A.apply_model(img[:, :7], msk[:, :7], A.identity_params(2))


# ---- the model, operation by operation ------------------------------------------------------------------------
def test_all_off_copies_images_and_thresholds_masks():
    img, msk = _frames(3, 9, 13, 1)
    msk[0, 0, :4] = [126, 127, 128, 255]
    out, tgt = A.apply_model(img, msk, A.identity_params(5, [2, 0, 1, 1, 2]))
    assert np.array_equal(out, img[[2, 0, 1, 1, 2]])
    assert tgt.dtype == np.float32 and tgt.shape == (5, 1, 9, 13)
    assert np.array_equal(tgt[:, 0], (msk[[2, 0, 1, 1, 2]] > 127).astype(np.float32))
    assert tgt[1, 0, 0, :4].tolist() == [0, 0, 1, 1]
    out2, none = A.apply_model(img, None, A.identity_params(3))
    assert none is None and np.array_equal(out2, img)


def test_flip_and_exact_rotations():
    for h, w in ((9, 9), (16, 16), (8, 11)):
        img, msk = _frames(1, h, w, 2)
        p = A.identity_params(3, [0, 0, 0])
        A.set_geometry(p[0], flip=True)
        A.set_geometry(p[1], angle_deg=180.0)
        A.set_geometry(p[2], flip=True, angle_deg=180.0)
        out, tgt = A.apply_model(img, msk, p)
        t = (msk[0] > 127).astype(np.float32)
        assert np.array_equal(out[0], img[0][:, ::-1]) and np.array_equal(tgt[0, 0], t[:, ::-1])
        assert np.array_equal(out[1], img[0][::-1, ::-1]) and np.array_equal(tgt[1, 0], t[::-1, ::-1])
        assert np.array_equal(out[2], img[0][::-1]) and np.array_equal(tgt[2, 0], t[::-1])      # flip, then half a turn
    for n in (9, 16):
        img, msk = _frames(1, n, n, 3)
        p = A.identity_params(2, [0, 0])
        A.set_geometry(p[0], angle_deg=90.0)          # positive = counter-clockwise
        A.set_geometry(p[1], angle_deg=-90.0)
        out, tgt = A.apply_model(img, msk, p)
        t = (msk[0] > 127).astype(np.float32)
        assert np.array_equal(out[0], np.rot90(img[0], 1)) and np.array_equal(tgt[0, 0], np.rot90(t, 1))
        assert np.array_equal(out[1], np.rot90(img[0], -1)) and np.array_equal(tgt[1, 0], np.rot90(t, -1))


def test_small_rotation_interpolates_and_reflects():
    # a linear ramp in x stays the same ramp under bilinear interpolation wherever all four taps are inside the frame
    h = w = 33
    img = np.repeat((np.arange(w, dtype=np.uint8) * 4)[None, :, None], h, axis=0).repeat(3, axis=2)[None]
    p = A.identity_params(1)
    A.set_geometry(p[0], angle_deg=15.0)
    out, _ = A.apply_model(img, None, p)
    cx = (w - 1) / 2
    a, b = math.cos(math.radians(15)), math.sin(math.radians(15))
    y, x = np.mgrid[0:h, 0:w]
    xs = a * (x - cx) - b * (y - cx) + cx
    inside = (xs >= 0) & (xs <= w - 1)
    want = 4 * xs
    assert np.abs(out[0, ..., 0].astype(np.float64) - want)[inside].max() <= 0.5 + 4 / 64 + 1e-9   # rounding + 1/32 pixel
    assert np.array_equal(A.reflect101(np.arange(-9, 12), 5), [1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3])


def test_brightness_contrast_lookup_closed_form():
    v = np.arange(256)
    for alpha, beta in ((1.0, 0.0), (1.3, 0.3), (0.7, -0.3)):
        a32, b32 = np.float32(alpha), np.float32(np.float32(beta) * np.float32(255))
        want = np.array([int(min(max(np.float32(np.float32(x) * a32) + b32, np.float32(0)), np.float32(255))) for x in v])
        lut = A.brightness_contrast_lut(alpha, b32)
        assert np.array_equal(lut, want)
        exact = np.clip(v * float(a32) + float(b32), 0, 255)
        assert np.abs(lut - exact).max() < 1.0 + 1e-4 and (lut <= exact + 1e-4).all()     # truncation, never above
    assert np.array_equal(A.brightness_contrast_lut(1.0, 0.0), v)
    img, _ = _frames(1, 8, 8, 4)
    p = A.identity_params(1)
    p["flags"], p["alpha"], p["beta255"] = A.FLAG_BC, 1.3, 0.3 * 255
    out, _ = A.apply_model(img, None, p)
    assert np.array_equal(out[0], A.brightness_contrast_lut(p["alpha"][0], p["beta255"][0])[img[0]])


PRIMARIES = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]], dtype=np.uint8)


def test_hsv_round_trip_and_shifts():
    greys = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    fixed = np.concatenate([greys, PRIMARIES])
    assert np.array_equal(A.hue_saturation_value(fixed, 0.0, 0.0, 0.0), fixed)
    assert A.rgb_to_hsv(PRIMARIES)[:, 0].tolist() == [0, 30, 60, 90, 120, 150]
    assert (A.rgb_to_hsv(PRIMARIES)[:, 1:] == 255).all() and (A.rgb_to_hsv(greys)[:, :2] == 0).all()
    # value shift on greys: clip(g + dv)
    for dv in (-30.0, 17.0, 30.0):
        want = np.clip(greys.astype(np.int64) + int(dv), 0, 255)
        assert np.array_equal(A.hue_saturation_value(greys, 0.0, 0.0, dv), want)
    # hue: +90 twice is the identity on H; +60 turns every primary into the next but one
    lut = A.hue_lut(90.0)
    assert np.array_equal(lut[lut], np.arange(180)) and lut[0] == 90 and lut[100] == 10
    assert np.array_equal(A.hue_lut(-30.0), (np.arange(180) - 30) % 180)
    assert np.array_equal(A.hue_lut(0.0), np.arange(180)) and A.hue_lut(-1e-7).max() <= 179
    assert np.array_equal(A.hue_saturation_value(PRIMARIES, 60.0, 0.0, 0.0), np.roll(PRIMARIES, -2, axis=0))
    assert np.array_equal(A.shift_lut(-30.0), np.clip(np.arange(256) - 30, 0, 255))
    # the 8-bit round trip of arbitrary colours stays close, as the library's own does: S and H are quantised
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (4096, 3), dtype=np.uint8)
    back = A.hsv_to_rgb(A.rgb_to_hsv(rgb))
    assert np.abs(back.astype(int) - rgb.astype(int)).max() <= 6
    hsv = A.rgb_to_hsv(rgb)
    assert hsv[:, 0].max() < 180 and np.array_equal(hsv[:, 2], rgb.max(axis=1))


def test_blur_constant_impulse_and_corner():
    const = np.full((1, 12, 10, 3), 201, dtype=np.uint8)
    for k in (3, 5, 7):
        assert np.array_equal(A.gaussian_blur(const[0], k), const[0])
        taps, shift = A.BLUR_TAPS[k]
        assert taps.sum() ** 2 == 1 << shift
        r = k // 2
        img = np.zeros((15, 15, 3), dtype=np.uint8)
        img[7, 7] = 255
        out = A.gaussian_blur(img, k)
        want = (np.outer(taps, taps) * 255 + (1 << (shift - 1))) >> shift
        assert np.array_equal(out[7 - r:8 + r, 7 - r:8 + r, 1], want)
        out[7 - r:8 + r, 7 - r:8 + r] = 0
        assert not out.any()
        # an impulse in the corner: reflect-101 folds taps -1..-r onto +1..+r (the corner itself is not doubled)
        img = np.zeros((15, 15, 3), dtype=np.uint8)
        img[0, 0] = 255
        out = A.gaussian_blur(img, k)
        fold = taps[r:]          # position j sees the impulse at 0 through tap -j only
        want = (np.outer(fold, fold) * 255 + (1 << (shift - 1))) >> shift
        assert np.array_equal(out[:r + 1, :r + 1, 0], want)
        # ... while an impulse one pixel in is seen twice from position 0 (taps +1 and the reflected -1)
        img = np.zeros((15, 15, 3), dtype=np.uint8)
        img[1, 1] = 255
        out = A.gaussian_blur(img, k)
        assert out[0, 0, 0] == ((2 * taps[r + 1]) ** 2 * 255 + (1 << (shift - 1))) >> shift
    p = A.identity_params(1)
    p["blur"] = 5
    img, _ = _frames(1, 10, 12, 6)
    assert np.array_equal(A.apply_model(img, None, p)[0][0], A.gaussian_blur(img[0], 5))


def test_golden_fixture_pins_the_model(golden_dir):
    g = np.load(os.path.join(golden_dir, "augment.npz"))
    params = np.frombuffer(g["params"].tobytes(), dtype=A.PARAMS_DTYPE)
    assert g["images"].shape == (2, 24, 40, 3) and params.size >= 4
    assert ((params["flags"] & (A.FLAG_BC | A.FLAG_HSV)) == (A.FLAG_BC | A.FLAG_HSV)).all() and (params["blur"] > 1).all()
    out, tgt = A.apply_model(g["images"], g["masks"], params.copy(), int(g["mask_threshold"]))
    assert np.array_equal(out, g["out_images"]) and np.array_equal(tgt, g["out_targets"])


# ---- batches --------------------------------------------------------------------------------------------------
def _tagged(n, h=8, w=8):
    """frame i is filled with the value i, mask i is 255 where i is odd"""
    img = np.empty((n, h, w, 3), dtype=np.uint8)
    img[:] = np.arange(n, dtype=np.uint8)[:, None, None, None]
    msk = np.zeros((n, h, w), dtype=np.uint8)
    msk[1::2] = 255
    return img, msk


def _off(seed=0):
    return A.Augmenter(seed=seed, p_flip=0, p_rotate=0, p_brightness_contrast=0, p_hsv=0, p_blur=0)


def test_batches_cover_every_index_once_and_reshuffle():
    img, msk = _tagged(10)
    ab = A.AugmentedBatches((img, msk), 4, _off(3), rank=0)
    assert len(ab) == 3
    epochs = []
    for _ in range(2):
        seen = []
        sizes = []
        for images, targets in ab():
            assert images.dtype == np.uint8 and targets.dtype == np.float32 and targets.shape[1:] == (1, 8, 8)
            ids = images[:, 0, 0, 0]
            assert (images == ids[:, None, None, None]).all()
            assert np.array_equal(targets[:, 0, 0, 0], (ids % 2).astype(np.float32))
            seen += ids.tolist()
            sizes.append(len(ids))
        assert sorted(seen) == list(range(10)) and sizes == [4, 4, 2]
        assert seen == ab.last_order.tolist()
        epochs.append(seen)
    assert epochs[0] != epochs[1]
    dl = A.AugmentedBatches((img, msk), 4, _off(3), drop_last=True, rank=0)
    assert len(dl) == 2 and [len(i) for i, _ in dl()] == [4, 4]
    # ranks draw different streams, the same rank the same one
    r0 = A.AugmentedBatches((img, msk), 4, _off(3), rank=0)
    r1 = A.AugmentedBatches((img, msk), 4, _off(3), rank=1)
    list(r0()), list(r1())
    assert r0.last_order.tolist() == epochs[0] and r1.last_order.tolist() != epochs[0]


def test_batches_follow_a_sampler():
    img, msk = _tagged(6)
    sampler = [5, 5, 0, 3, 3, 3, 1]
    got = [i[:, 0, 0, 0].tolist() for i, _ in A.AugmentedBatches((img, msk), 3, _off(), sampler=sampler, rank=0)()]
    assert got == [[5, 5, 0], [3, 3, 3], [1]]
    import torch
    from unet_lane_detection_amd import imbalance
    weights = imbalance.sample_weights(counts=(msk > 127).sum(axis=(1, 2)), pixels=64)
    ws = torch.utils.data.WeightedRandomSampler(weights, len(weights), replacement=True)
    ab = A.AugmentedBatches((img, msk), 4, _off(), sampler=ws, rank=0)
    assert len(ab) == 2 and sum(len(i) for i, _ in ab()) == 6


def test_val_batches_are_the_plain_frames_in_order():
    img, msk = _frames(5, 8, 9, 8)
    got = list(A.val_batches((img, msk), 2)())
    assert [len(i) for i, _ in got] == [2, 2, 1]
    assert np.array_equal(np.concatenate([i for i, _ in got]), img)
    assert np.array_equal(np.concatenate([t for _, t in got])[:, 0], (msk > 127).astype(np.float32))


class _Val:
    def __init__(self, dice, loss):
        self.dice, self.loss = dice, loss


class _StubTrainer:
    """The stub of tests/test_validate_cpu.py, taking arrays: the loss of a step is the mean of its targets."""

    def __init__(self):
        self.lr, self.steps, self.validated = 1e-3, [], []

    def step(self, images, targets):
        assert images.dtype == np.uint8 and images.shape[1:] == (8, 8, 3) and targets.shape == (len(images), 1, 8, 8)
        self.steps.append(len(images))
        return float(targets.mean())

    def validate(self, batches):
        self.validated.append(sum(len(i) for i, _ in batches))
        return _Val(0.5, 0.5)

    def save_checkpoint(self, path, epoch=0, best_dice=None, with_optimizer=True):
        pass


def test_fit_runs_on_augmented_batches():
    img, msk = _tagged(10)
    tr = _StubTrainer()
    hist = loop.fit(tr, A.AugmentedBatches((img, msk), 4, A.Augmenter(seed=2), rank=0), A.val_batches((img, msk), 4), epochs=2)
    assert tr.steps == [4, 4, 2, 4, 4, 2] and tr.validated == [10, 10]
    assert len(hist) == 2 and all(0.0 <= h["train_loss"] <= 1.0 for h in hist)
