"""Host arithmetic of unet_lane_detection_amd.imbalance on given counts - no GPU, no library - against the output of the
reference's `get_sample_weights` (tests/golden/tiny_f4_8_focal2.npz, made by make_golden_focal.py) and against
`calculate_pos_weight`'s arithmetic."""
import os

import numpy as np
import pytest

import unet_lane_detection_amd as pkg
from unet_lane_detection_amd import imbalance


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "tiny_f4_8_focal2.npz"))


def test_sample_weights_match_the_reference_function(fixture):
    masks = fixture["masks_u8"]
    counts = (masks > 127).reshape(masks.shape[0], -1).sum(1)
    assert np.array_equal(counts, fixture["positive_counts"])
    assert counts.min() == 0 and counts.max() == masks[0].size          # an empty and a full mask are in the set
    assert (masks == 127).any() and (masks == 128).any()                # both sides of the `> 127` border
    w = imbalance.sample_weights(counts=counts, pixels=masks[0].size)
    assert w.dtype == np.float64 and w.shape == (masks.shape[0],)
    # the reference takes mask.mean() of a float32 tensor: its ratio carries fp32 rounding (2^-24 relative), times 5
    assert np.abs(w - fixture["sample_weights"]).max() <= 5 * 2.0 ** -23
    assert w[counts == 0][0] == 1.0 and w[counts == masks[0].size][0] == 6.0
    # per-image pixel counts, another gain
    w2 = imbalance.sample_weights(counts=counts, pixels=np.full(counts.size, masks[0].size), gain=2.0)
    assert np.allclose(w2 - 1.0, (w - 1.0) * 0.4, rtol=1e-15, atol=0)


def test_sample_weights_feed_a_weighted_random_sampler(fixture):
    import torch
    from torch.utils.data import WeightedRandomSampler
    w = imbalance.sample_weights(counts=fixture["positive_counts"], pixels=fixture["masks_u8"][0].size)
    g = torch.Generator().manual_seed(0)
    picks = list(WeightedRandomSampler(w, 4000, replacement=True, generator=g))
    hist = np.bincount(picks, minlength=w.size) / 4000.0
    assert np.abs(hist - w / w.sum()).max() < 0.03


def test_pos_weight_is_the_reference_arithmetic(fixture):
    """`calculate_pos_weight` (reference README.md:2514-2530) reads its masks with cv2, which is not installed here, so
    its arithmetic is restated: total_pixels += mask.size; positive_pixels += (mask > 127).sum();
    pos_ratio = positive_pixels / total_pixels; neg_ratio = 1 - pos_ratio; pos_weight = neg_ratio / pos_ratio."""
    masks = fixture["masks_u8"]
    total_pixels = positive_pixels = 0
    for mask in masks:
        total_pixels += mask.size
        positive_pixels += (mask > 127).sum()
    pos_ratio = positive_pixels / total_pixels
    neg_ratio = 1 - pos_ratio
    pos_weight = neg_ratio / pos_ratio
    got = imbalance.pos_weight_from_masks(counts=fixture["positive_counts"], pixels=masks[0].size)
    assert got == (pos_ratio, pos_weight)
    # the reference's own example: 8.5 % positives -> 10.76 (README.md:2534)
    r, pw = imbalance.pos_weight_from_masks(counts=[85, 85], pixels=1000)
    assert r == 0.085 and f"{pw:.2f}" == "10.76"
    assert imbalance.pos_weight_from_masks(counts=[0, 0], pixels=[10, 20]) == (0.0, float("inf"))


def test_argument_checks_and_exports():
    with pytest.raises(ValueError):
        imbalance.sample_weights()
    with pytest.raises(ValueError):
        imbalance.sample_weights(counts=[1, 2])
    with pytest.raises(ValueError):
        imbalance.sample_weights(counts=[11], pixels=10)
    with pytest.raises(ValueError):
        imbalance.pos_weight_from_masks(counts=[1, 2], pixels=[10])
    with pytest.raises(ValueError):
        imbalance.pos_weight_from_masks(counts=[], pixels=10)
    assert pkg.sample_weights is imbalance.sample_weights and pkg.pos_weight_from_masks is imbalance.pos_weight_from_masks
    assert pkg.positive_counts is imbalance.positive_counts
