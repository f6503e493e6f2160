"""Training-time augmentation: the reference's `train_transform` (README.md:2035-2055, `get_transforms`)

  Resize -> HorizontalFlip(0.5) -> Rotate(+-15 deg, 0.5) -> RandomBrightnessContrast(0.3, 0.3, p=0.7)
         -> HueSaturationValue(30, 30, 30, p=0.7) -> GaussianBlur((3, 7), p=0.3) -> Normalize

as one GPU stage between a device-resident data set and `trainer.step(images, targets)`: uint8 NHWC frames in, uint8
NHWC frames and float32 (N,1,H,W) targets out.  Resize stays `CameraStage.resize` (frames arrive at training size) and
Normalize stays fused into the first convolution.  GaussNoise, ColorJitter and RandomCrop, which only the reference's
documentation-only variants use, are not here.

This module states the arithmetic once, in plain numpy (`apply_model`): it is the specification the kernel
(csrc/augment_kernels.cpp, `unet_augment_u8`) is tested against bit for bit, and it is what numpy inputs run through.
Every 8-bit intermediate is rounded to uint8 between operations, as the reference's library does.  Bit parity with
albumentations / cv2 themselves is UNPINNED: neither is installed here, and the reference has no fixture for this
stage.  What is pinned is the kernel against this model, with tolerance zero - every step is integer arithmetic or a
fixed sequence of separately rounded IEEE operations:

  geometry    output pixel (x, y) -> source coordinate through the sample's inverse affine, in double, on offsets from
              the image centre ((W-1)/2, (H-1)/2):  xs = (m0 dx + m1 dy + m2) + cx,  ys = (m3 dx + m4 dy + m5) + cy.
              Flip and rotation are composed on the host (`inverse_affine`); the device never evaluates cos or sin.  A
              positive angle turns the picture counter-clockwise, as cv2.getRotationMatrix2D defines it.  Coordinates are
              rounded to 1/32 pixel (rint of 32 xs); the image is interpolated bilinearly with the fixed-point weights
              of `warp_pixel` in csrc/camera_stage.h (weights 32*32*32, then (acc + 2^14) >> 15), the mask is taken at
              the nearest source pixel ((X + 16) >> 5); both with reflect-101 borders, applied to every tap on its own.
              An identity or a pure flip lands on integer coordinates and copies exactly, and so do 90 and 180 degrees
              on a square image.
  brightness  the library's 8-bit lookup, trunc(clip(fp32(v) * alpha + beta255, 0, 255)), beta255 = beta * 255: two
  / contrast  separately rounded fp32 operations.
  hue / sat   RGB -> 8-bit HSV (H in [0, 180)) in integers with round-half-up, the library's three lookups
  / value     trunc(mod(h + dh, 180)), trunc(clip(s + ds, 0, 255)), trunc(clip(v + dv, 0, 255)) in fp32, HSV -> RGB in
              integers.  Greys and the six pure primaries and secondaries survive the round trip unchanged.
  blur        OpenCV's fixed small kernels [1,2,1]/4, [1,4,6,4,1]/16, [2,7,14,18,14,7,2]/64, separable, in exact
              integers with one rounding of the 2-D sum, (acc + half) >> shift; reflect-101 borders on the already
              rotated and coloured image.
  masks       only the geometry touches them; `> threshold` (127, README.md:2022) gives the float32 targets.

Parameters are one record per output sample (`PARAMS_DTYPE`, the C struct `unet::AugmentParams`), drawn on the host by
`Augmenter.sample_params` from numpy.random.default_rng(seed).
"""
from __future__ import annotations

import math

import numpy as np

FLAG_FLIP, FLAG_ROTATE, FLAG_BC, FLAG_HSV = 1, 2, 4, 8   # the first two are informative: the matrix carries them

# struct unet::AugmentParams of csrc/augment_kernels.h, 80 bytes
PARAMS_DTYPE = np.dtype([("m", "<f8", (6,)), ("src", "<i4"), ("flags", "<u4"), ("alpha", "<f4"), ("beta255", "<f4"),
                         ("dh", "<f4"), ("ds", "<f4"), ("dv", "<f4"), ("blur", "<i4")], align=True)
assert PARAMS_DTYPE.itemsize == 80

BLUR_TAPS = {3: (np.array([1, 2, 1], dtype=np.int64), 4),
             5: (np.array([1, 4, 6, 4, 1], dtype=np.int64), 8),
             7: (np.array([2, 7, 14, 18, 14, 7, 2], dtype=np.int64), 12)}   # taps, shift of the 2-D sum
MIN_SIDE = 8          # reflect-101 with the blur's 3-pixel halo stays single-bounce
_COORD_LIMIT = float(1 << 30)


def inverse_affine(flip=False, angle_deg=0.0):
    """The six doubles of a record's `m`: HorizontalFlip (if flip) followed by a rotation by angle_deg, inverted
    (output -> source), on offsets from the image centre."""
    a, b = (1.0, 0.0) if angle_deg == 0 else (math.cos(math.radians(angle_deg)), math.sin(math.radians(angle_deg)))
    sx = -1.0 if flip else 1.0
    # inverse rotation about the centre: xf = a dx - b dy, yf = b dx + a dy; the flip negates the source x offset
    return np.array([sx * a, -sx * b, 0.0, b, a, 0.0], dtype=np.float64)


def identity_params(n, indices=None):
    """n records that switch every operation off: sample i copies source i (or indices[i])."""
    p = np.zeros(int(n), dtype=PARAMS_DTYPE)
    p["m"] = inverse_affine()
    p["src"] = np.arange(n) if indices is None else np.asarray(indices)
    p["alpha"] = 1.0
    p["blur"] = 1
    return p


def set_geometry(record, flip=False, angle_deg=0.0):
    """Writes flip / rotation into one record (an element of a table): matrix and the two informative flags."""
    record["m"] = inverse_affine(flip, angle_deg)
    record["flags"] = (int(record["flags"]) & ~(FLAG_FLIP | FLAG_ROTATE)) | (FLAG_FLIP if flip else 0) | \
        (FLAG_ROTATE if angle_deg != 0 else 0)


def validate_params(params, n_source):
    """ValueError unless the table is a 1-d PARAMS_DTYPE array with indices in [0, n_source), blur sizes in
    {1, 3, 5, 7}, a finite matrix and colour parameters of a sane magnitude."""
    if not isinstance(params, np.ndarray) or params.dtype != PARAMS_DTYPE or params.ndim != 1 or params.size == 0:
        raise ValueError("params must be a non-empty 1-d array of augment.PARAMS_DTYPE")
    if (params["src"] < 0).any() or (params["src"] >= int(n_source)).any():
        raise ValueError("source index outside [0, %d)" % int(n_source))
    if not np.isin(params["blur"], (1, 3, 5, 7)).all():
        raise ValueError("blur size must be 1, 3, 5 or 7")
    if not np.isfinite(params["m"]).all():
        raise ValueError("the affine matrix must be finite")
    for k, limit in (("alpha", 1e6), ("beta255", 1e6), ("dh", 1024.0), ("ds", 1024.0), ("dv", 1024.0)):
        if not (np.abs(params[k]) <= limit).all():     # false for NaN as well
            raise ValueError("%s must lie within +-%g" % (k, limit))


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def reflect101(p, n):
    """Index p (any integer array) folded into [0, n) the way BORDER_REFLECT_101 does: ... 2 1 | 0 1 2 ... n-1 | n-2 ..."""
    period = 2 * (n - 1)
    t = np.mod(p, period)
    return np.where(t < n, t, period - t)


def _fixed_coords(m, height, width):
    cx, cy = (width - 1) * 0.5, (height - 1) * 0.5
    dy, dx = np.meshgrid(np.arange(height, dtype=np.float64) - cy, np.arange(width, dtype=np.float64) - cx, indexing="ij")
    fx = ((m[0] * dx + m[1] * dy + m[2]) + cx) * 32.0
    fy = ((m[3] * dx + m[4] * dy + m[5]) + cy) * 32.0
    X = np.rint(np.clip(fx, -_COORD_LIMIT, _COORD_LIMIT)).astype(np.int64)
    Y = np.rint(np.clip(fy, -_COORD_LIMIT, _COORD_LIMIT)).astype(np.int64)
    return X, Y


def warp_image(img, m):
    """(H,W,3) uint8 -> (H,W,3) uint8 through the inverse affine m: bilinear, 1/32-pixel coordinates, reflect-101."""
    h, w = img.shape[:2]
    X, Y = _fixed_coords(m, h, w)
    sx, sy, fa, fb = X >> 5, Y >> 5, X & 31, Y & 31
    wgt = ((32 - fb) * (32 - fa) * 32, (32 - fb) * fa * 32, fb * (32 - fa) * 32, fb * fa * 32)
    acc = np.zeros((h, w, 3), dtype=np.int64)
    src = img.astype(np.int64)
    for t in range(4):
        yy, xx = reflect101(sy + (t >> 1), h), reflect101(sx + (t & 1), w)
        acc += wgt[t][..., None] * src[yy, xx]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def warp_mask(mask, m):
    """(H,W) uint8 -> (H,W) uint8: the nearest source pixel, reflect-101."""
    h, w = mask.shape
    X, Y = _fixed_coords(m, h, w)
    return mask[reflect101((Y + 16) >> 5, h), reflect101((X + 16) >> 5, w)]


def brightness_contrast_lut(alpha, beta255):
    """The 256-entry lookup of RandomBrightnessContrast: trunc(clip(fp32(v) * alpha + beta255, 0, 255))."""
    v = np.arange(256, dtype=np.float32) * np.float32(alpha)
    v = v + np.float32(beta255)
    return np.clip(v, np.float32(0), np.float32(255)).astype(np.uint8)


def hue_lut(dh):
    """trunc(mod(h + dh, 180)) for h = 0..179 in fp32: t = h + dh; t -= floor(t / 180) * 180; one fold back into [0, 180), the integer clamped to [0, 179]."""
    c = np.float32(180)
    t = np.arange(180, dtype=np.float32) + np.float32(dh)
    k = np.floor(t / c)
    t = t - k * c
    t = np.where(t >= c, t - c, t)
    t = np.where(t < np.float32(0), t + c, t)
    return np.clip(t.astype(np.int32), 0, 179).astype(np.uint8)


def shift_lut(d):
    """trunc(clip(v + d, 0, 255)) for v = 0..255 in fp32 (saturation and value)."""
    t = np.arange(256, dtype=np.float32) + np.float32(d)
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.uint8)


def rgb_to_hsv(rgb):
    """(...,3) uint8 RGB -> (...,3) uint8 HSV, H in [0,180): integers, round-half-up.
    S = round(255 diff / V); H = round(30 num / diff) + {0, 60, 120} for V == R, G, B in that order of preference."""
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (510 * diff + v) // np.maximum(2 * v, 1)
    is_r, is_g = v == r, (v != r) & (v == g)
    num = np.where(is_r, g - b, np.where(is_g, b - r, r - g))
    off = np.where(is_r, 0, np.where(is_g, 60, 120))
    d = np.maximum(diff, 1)
    h = off - 30 + (60 * (num + d) + d) // (2 * d)
    h = np.where(h < 0, h + 180, h)
    h = np.where(h >= 180, h - 180, h)
    h = np.where(diff == 0, 0, h)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def hsv_to_rgb(hsv):
    """(...,3) uint8 HSV (H in [0,180)) -> (...,3) uint8 RGB: integers, round-half-up."""
    h, s, v = (hsv[..., c].astype(np.int64) for c in range(3))
    sector, fr = h // 30, h % 30
    p = (2 * v * (255 - s) + 255) // 510
    q = (2 * v * (7650 - s * fr) + 7650) // 15300
    t = (2 * v * (7650 - s * (30 - fr)) + 7650) // 15300
    r = np.choose(sector, [v, q, p, p, t, v])
    g = np.choose(sector, [t, v, v, q, p, p])
    b = np.choose(sector, [p, p, t, v, v, q])
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def hue_saturation_value(img, dh, ds, dv):
    hsv = rgb_to_hsv(img)
    out = np.stack([hue_lut(dh)[hsv[..., 0]], shift_lut(ds)[hsv[..., 1]], shift_lut(dv)[hsv[..., 2]]], axis=-1)
    return hsv_to_rgb(out)


def gaussian_blur(img, ksize):
    """(H,W,3) uint8, ksize in {3,5,7}: separable integer taps, reflect-101, one rounding of the 2-D sum."""
    taps, shift = BLUR_TAPS[int(ksize)]
    r = len(taps) // 2
    h, w = img.shape[:2]
    pad = np.pad(img.astype(np.int64), ((r, r), (r, r), (0, 0)), mode="reflect")
    rows = sum(int(taps[k]) * pad[:, k:k + w] for k in range(len(taps)))
    acc = sum(int(taps[k]) * rows[k:k + h] for k in range(len(taps)))
    return ((acc + (1 << (shift - 1))) >> shift).astype(np.uint8)


def apply_model(images, masks, params, mask_threshold=127, labels=False):
    """images (n_source,H,W,3) uint8, masks (n_source,H,W) uint8 or None, params a PARAMS_DTYPE table ->
    (images (n,H,W,3) uint8, targets (n,1,H,W) float32 or None).  labels=True (multi-class training): the masks hold
    class labels and the second output is the warped byte itself, (n,H,W) uint8 - no threshold."""
    images = np.asarray(images)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
        raise ValueError("images must be (n, H, W, 3) uint8")
    ns, h, w = images.shape[:3]
    if h < MIN_SIDE or w < MIN_SIDE:
        raise ValueError("height and width must be at least %d" % MIN_SIDE)
    if masks is not None:
        masks = np.asarray(masks)
        if masks.dtype != np.uint8 or masks.size != ns * h * w:
            raise ValueError("masks must be uint8 with one (H, W) mask per image")
        masks = masks.reshape(ns, h, w)
    validate_params(params, ns)
    out = np.empty((params.size, h, w, 3), dtype=np.uint8)
    if labels and masks is None:
        raise ValueError("labels=True needs the label planes")
    tgt = None
    if masks is not None:
        tgt = np.empty((params.size, h, w), dtype=np.uint8) if labels else np.empty((params.size, 1, h, w), dtype=np.float32)
    for i, p in enumerate(params):
        img = warp_image(images[p["src"]], p["m"])
        if p["flags"] & FLAG_BC:
            img = brightness_contrast_lut(p["alpha"], p["beta255"])[img]
        if p["flags"] & FLAG_HSV:
            img = hue_saturation_value(img, p["dh"], p["ds"], p["dv"])
        if p["blur"] > 1:
            img = gaussian_blur(img, p["blur"])
        out[i] = img
        if tgt is not None and labels:
            tgt[i] = warp_mask(masks[p["src"]], p["m"])
        elif tgt is not None:
            tgt[i, 0] = warp_mask(masks[p["src"]], p["m"]) > mask_threshold
    return out, tgt


# ---------------------------------------------------------------------------------------------------------------
# the kernel behind torch tensors
# ---------------------------------------------------------------------------------------------------------------
def _apply_device(images, masks, params, mask_threshold, out, labels=False):
    import torch

    from . import _lib
    if int(_lib.load().unet_augment_param_bytes()) != PARAMS_DTYPE.itemsize:
        raise RuntimeError("augment.PARAMS_DTYPE does not match the library's record")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError("images must be a contiguous (n, H, W, 3) uint8 tensor")
    ns, h, w = (int(v) for v in images.shape[:3])
    if h < MIN_SIDE or w < MIN_SIDE:
        raise ValueError("height and width must be at least %d" % MIN_SIDE)
    if masks is not None and (masks.dtype != torch.uint8 or masks.numel() != ns * h * w or not masks.is_contiguous()
                              or masks.device != images.device):
        raise ValueError("masks must be a contiguous uint8 tensor on the images' device, one (H, W) mask per image")
    validate_params(params, ns)
    n = int(params.size)
    dev = images.device
    if labels and masks is None:
        raise ValueError("labels=True needs the label planes")
    tgt_shape, tgt_dtype = ((n, h, w), torch.uint8) if labels else ((n, 1, h, w), torch.float32)
    if out is None:
        out_img = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        out_tgt = torch.empty(tgt_shape, dtype=tgt_dtype, device=dev) if masks is not None else None
    else:
        out_img, out_tgt = out
        if out_img.shape != (n, h, w, 3) or out_img.dtype != torch.uint8 or not out_img.is_contiguous() or out_img.device != dev:
            raise ValueError("out[0] must be a contiguous (n, H, W, 3) uint8 tensor on the images' device")
        if masks is not None and (out_tgt is None or out_tgt.shape != tgt_shape or out_tgt.dtype != tgt_dtype
                                  or not out_tgt.is_contiguous() or out_tgt.device != dev):
            raise ValueError("out[1] must be a contiguous (n, 1, H, W) float32 tensor - with labels=True (n, H, W) uint8 - "
                             "on the images' device")
    # the table goes up on the launch's own stream, ahead of it
    table = torch.from_numpy(np.ascontiguousarray(params).view(np.uint8).copy()).to(dev)
    if labels:
        _lib.call("unet_augment_u8_labels", dev, images, masks, ns, h, w, table, n, out_img, out_tgt)
        return out_img, out_tgt
    _lib.call("unet_augment_u8", dev, images, masks, ns, h, w, table, n, int(mask_threshold), out_img,
              out_tgt if masks is not None else None)
    return out_img, (out_tgt if masks is not None else None)


class Augmenter:
    """Draws the parameter tables and applies them.  Defaults are the reference's limits and probabilities
    (README.md:2041-2049)."""

    def __init__(self, seed=0, p_flip=0.5, rotate_limit=15.0, p_rotate=0.5, brightness_limit=0.3, contrast_limit=0.3,
                 p_brightness_contrast=0.7, hue_shift_limit=30.0, sat_shift_limit=30.0, val_shift_limit=30.0, p_hsv=0.7,
                 blur_limit=(3, 7), p_blur=0.3, mask_threshold=127):
        lo, hi = (int(v) for v in blur_limit)
        self.blur_sizes = [k for k in (3, 5, 7) if lo <= k <= hi]
        if not self.blur_sizes:
            raise ValueError("blur_limit must include one of the sizes 3, 5, 7")
        for p in (p_flip, p_rotate, p_brightness_contrast, p_hsv, p_blur):
            if not 0.0 <= p <= 1.0:
                raise ValueError("probabilities must lie in [0, 1]")
        self.seed = int(seed)
        self.kw = dict(p_flip=p_flip, rotate_limit=rotate_limit, p_rotate=p_rotate, brightness_limit=brightness_limit,
                       contrast_limit=contrast_limit, p_brightness_contrast=p_brightness_contrast,
                       hue_shift_limit=hue_shift_limit, sat_shift_limit=sat_shift_limit, val_shift_limit=val_shift_limit,
                       p_hsv=p_hsv, blur_limit=blur_limit, p_blur=p_blur, mask_threshold=mask_threshold)
        self.mask_threshold = int(mask_threshold)
        self.rng = np.random.default_rng(self.seed)

    def reseeded(self, seed):
        """A fresh Augmenter with the same limits and another seed (AugmentedBatches: seed + rank)."""
        return Augmenter(seed=seed, **self.kw)

    def sample_params(self, n, n_source, indices=None):
        """n records; sample i reads source indices[i] (default i mod n_source).  Every operation is switched by its
        own Bernoulli draw; a fixed number of draws per call, so the same seed gives the same table."""
        n, k, rng = int(n), self.kw, self.rng
        src = np.arange(n) % int(n_source) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
        if src.size != n:
            raise ValueError("indices must hold n entries")
        p = identity_params(n, src)
        flip = rng.random(n) < k["p_flip"]
        rot = rng.random(n) < k["p_rotate"]
        angle = rng.uniform(-k["rotate_limit"], k["rotate_limit"], n)
        bc = rng.random(n) < k["p_brightness_contrast"]
        alpha = 1.0 + rng.uniform(-k["contrast_limit"], k["contrast_limit"], n)
        beta = rng.uniform(-k["brightness_limit"], k["brightness_limit"], n)
        hsv = rng.random(n) < k["p_hsv"]
        dh = rng.uniform(-k["hue_shift_limit"], k["hue_shift_limit"], n)
        ds = rng.uniform(-k["sat_shift_limit"], k["sat_shift_limit"], n)
        dv = rng.uniform(-k["val_shift_limit"], k["val_shift_limit"], n)
        blur = rng.random(n) < k["p_blur"]
        size = np.asarray(self.blur_sizes)[rng.integers(0, len(self.blur_sizes), n)]
        for i in range(n):
            set_geometry(p[i], bool(flip[i]), float(angle[i]) if rot[i] else 0.0)
        p["flags"] |= np.where(bc, FLAG_BC, 0).astype(np.uint32) | np.where(hsv, FLAG_HSV, 0).astype(np.uint32)
        p["alpha"] = np.where(bc, alpha, 1.0)
        p["beta255"] = np.where(bc, beta * 255.0, 0.0)
        p["dh"], p["ds"], p["dv"] = np.where(hsv, dh, 0.0), np.where(hsv, ds, 0.0), np.where(hsv, dv, 0.0)
        p["blur"] = np.where(blur, size, 1)
        return p

    def apply(self, images, masks, params=None, out=None, labels=False):
        """-> (images uint8 (n,H,W,3), targets float32 (n,1,H,W) or None without masks).  Torch tensors on the device
        go through the kernel, numpy arrays through the model; anything else is an error.  params None draws one
        record per given image; out = (images, targets) tensors to write into (device path).  labels=True: the masks
        are class-label planes and come back warped as they are, uint8 (n,H,W), for a K-class trainer."""
        if params is None:
            params = self.sample_params(len(images), len(images))
        if isinstance(images, np.ndarray):
            if out is not None:
                raise ValueError("out= is for device tensors")
            return apply_model(images, masks, params, self.mask_threshold, labels=labels)
        import torch
        if not isinstance(images, torch.Tensor) or not images.is_cuda:
            raise TypeError("images must be a numpy array (the CPU model) or a torch tensor on the GPU (the kernel)")
        return _apply_device(images, masks, params, self.mask_threshold, out, labels=labels)


class DeviceDataset:
    """The whole training set resident on the GPU: images (n,H,W,3) uint8 and masks (n,H,W) uint8, copied once.  (The
    reference's 960 frames at 224 x 224 are 144 MB of images and 48 MB of masks.)"""

    def __init__(self, images_u8, masks_u8, device=0):
        import torch
        dev = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        self.images = torch.as_tensor(images_u8).to(dev).contiguous()
        self.masks = torch.as_tensor(masks_u8).to(dev).contiguous()
        if self.images.dtype != torch.uint8 or self.images.dim() != 4 or self.images.shape[3] != 3:
            raise ValueError("images must be (n, H, W, 3) uint8")
        n, h, w = self.images.shape[:3]
        if self.masks.dtype != torch.uint8 or self.masks.numel() != n * h * w:
            raise ValueError("masks must be uint8, one (H, W) mask per image")
        self.masks = self.masks.reshape(n, h, w)

    def __len__(self):
        return int(self.images.shape[0])


def _arrays(dataset):
    if isinstance(dataset, DeviceDataset):
        return dataset.images, dataset.masks
    images, masks = dataset
    return images, masks


def _batches(order, batch_size, drop_last):
    for i in range(0, len(order), batch_size):
        idx = order[i:i + batch_size]
        if len(idx) < batch_size and drop_last:
            return
        yield idx


class AugmentedBatches:
    """`train_batches` of loop.fit: calling it returns a fresh iterable of (images, targets) for one epoch.  dataset: a
    DeviceDataset (the kernel) or a pair (images, masks) of numpy arrays (the model).  Without a sampler every epoch is a
    new permutation of the data set; with one (any iterable of indices that can be iterated once per epoch, e.g. a
    torch WeightedRandomSampler over imbalance.sample_weights) its indices are used as they come.  The gather happens
    in the kernel through the parameter table's source index: no indexed copy precedes it.  Under an initialised
    process group the augmenter is re-seeded with seed + rank, so the ranks draw different streams."""

    def __init__(self, dataset, batch_size, augmenter, sampler=None, drop_last=False, rank=None, labels=False):
        """labels=True: the data set's masks are class-label planes; the batches carry uint8 (n,H,W) labels"""
        self.labels = bool(labels)
        self.images, self.masks = _arrays(dataset)
        self.batch_size, self.sampler, self.drop_last = int(batch_size), sampler, bool(drop_last)
        if self.batch_size <= 0 or len(self.images) == 0:
            raise ValueError("batch_size must be positive and the data set non-empty")
        if rank is None:
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.augmenter = augmenter.reseeded(augmenter.seed + int(rank)) if rank else augmenter
        self.last_order = None      # the indices of the epoch in progress, for inspection

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.images)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __call__(self):
        n = len(self.images)
        if self.sampler is None:
            order = self.augmenter.rng.permutation(n)
        else:
            order = np.asarray([int(i) for i in self.sampler], dtype=np.int64)
        self.last_order = order
        for idx in _batches(order, self.batch_size, self.drop_last):
            params = self.augmenter.sample_params(len(idx), n, idx)
            yield self.augmenter.apply(self.images, self.masks, params, labels=self.labels)


def val_batches(dataset, batch_size, mask_threshold=127, labels=False):
    """The reference's `val_transform` (README.md:2051-2055): no augmentation, frames in order, masks thresholded to
    targets (labels=True: class-label planes passed through as uint8 (n,H,W)).  Returns a callable for loop.fit /
    trainer.validate."""
    images, masks = _arrays(dataset)
    plain = Augmenter(mask_threshold=mask_threshold)

    def epoch():
        for idx in _batches(np.arange(len(images)), int(batch_size), False):
            yield plain.apply(images, masks, identity_params(len(idx), idx), labels=labels)
    return epoch
