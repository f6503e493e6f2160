"""Mask statistics for sparse lanes (reference README.md:2506-2558, "handling class imbalance"): the positive-pixel
count of every mask on the device, and the two numbers the reference derives from it on the host -

  pos_weight_from_masks   `calculate_pos_weight` (README.md:2514-2530): pos_ratio = positive / total pixels over the
                          mask set, pos_weight = (1 - pos_ratio) / pos_ratio, for BCE(pos_weight);
  sample_weights          `get_sample_weights` (README.md:2544-2553): 1 + 5 * lane_ratio per image, for
                          torch.utils.data.WeightedRandomSampler(weights, len(weights), replacement=True).

Masks are the dataset's uint8 images, binarised with `> 127` as the reference does (README.md:2022, :2522).  The
counting runs in libunet_hip.so (unet_mask_positive_counts); the host arithmetic is plain numpy on the counts, so both
functions also take counts made elsewhere (`counts=`, `pixels=`) and then need neither a GPU nor the library.
"""
from __future__ import annotations

import numpy as np


def positive_counts(masks_u8, threshold=127, device=0):
    """masks_u8: (n, ...) uint8, numpy array or torch tensor (host or device) -> int64 numpy array of n counts of
    pixels with mask > threshold.  One device pass, exact."""
    import torch

    from . import _lib
    if not torch.cuda.is_available():
        raise RuntimeError("positive_counts needs a HIP device; there is no CPU fallback (pass counts= to the host helpers)")
    m = torch.as_tensor(masks_u8)
    if m.dtype != torch.uint8:
        raise TypeError(f"masks must be uint8, got {m.dtype}")
    if m.dim() < 1 or m.shape[0] == 0 or m.numel() == 0:
        raise ValueError("masks must hold at least one non-empty image")
    if not m.is_cuda:
        m = m.to(torch.device("cuda", int(device)))
    m = m.contiguous()
    n = int(m.shape[0])
    counts = torch.empty(n, dtype=torch.int64, device=m.device)
    _lib.call("unet_mask_positive_counts", m.device, m, n, m.numel() // n, int(threshold), counts)
    return counts.cpu().numpy()


def _counts_and_pixels(batches, threshold, counts, pixels, device):
    if counts is None:
        if batches is None:
            raise ValueError("give the masks (batches) or their counts (counts=, pixels=)")
        cs, ps = [], []
        for b in batches:
            c = positive_counts(b, threshold=threshold, device=device)
            cs.append(c)
            ps.append(np.full(c.size, int(np.prod(tuple(b.shape)[1:], dtype=np.int64)), dtype=np.int64))
        if not cs:
            raise ValueError("no masks")
        return np.concatenate(cs), np.concatenate(ps)
    if pixels is None:
        raise ValueError("counts= needs pixels= (per image, or one number for all)")
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    p = np.broadcast_to(np.asarray(pixels, dtype=np.int64), c.shape) if np.ndim(pixels) == 0 else \
        np.asarray(pixels, dtype=np.int64).reshape(-1)
    if p.shape != c.shape or c.size == 0 or (p <= 0).any() or (c < 0).any() or (c > p).any():
        raise ValueError("counts and pixels must be non-empty, of one length, with 0 <= count <= pixels and pixels > 0")
    return c, p


def pos_weight_from_masks(batches=None, threshold=127, counts=None, pixels=None, device=0):
    """-> (pos_ratio, pos_weight) over the whole mask set, as `calculate_pos_weight` returns and prints them.
    batches: an iterable of (n, ...) uint8 mask arrays.  A set without one positive pixel gives (0.0, inf)."""
    c, p = _counts_and_pixels(batches, threshold, counts, pixels, device)
    positive, total = int(c.sum()), int(p.sum())
    pos_ratio = positive / total
    neg_ratio = 1 - pos_ratio
    return pos_ratio, (neg_ratio / pos_ratio if positive else float("inf"))


def sample_weights(batches=None, gain=5.0, threshold=127, counts=None, pixels=None, device=0):
    """-> float64 numpy array, 1 + gain * lane_ratio per image in the order of the batches, as `get_sample_weights`
    (gain 5) returns them."""
    c, p = _counts_and_pixels(batches, threshold, counts, pixels, device)
    return 1.0 + float(gain) * (c.astype(np.float64) / p.astype(np.float64))
