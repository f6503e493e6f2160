"""Mask statistics on the device (unet_mask_positive_counts behind imbalance.positive_counts): exact counts against
numpy, and the two host helpers fed from device counts against the reference's `get_sample_weights`
(tests/golden/tiny_f4_8_focal2.npz)."""
import os

import numpy as np
import pytest
import torch

from unet_lane_detection_amd import imbalance

pytestmark = pytest.mark.gpu


def _want(masks, thr=127):
    return (masks > thr).reshape(masks.shape[0], -1).sum(1).astype(np.int64)


@pytest.mark.parametrize("shape", [(1,), (224, 224), (640, 640), (7, 9)], ids=["1px", "224x224", "640x640", "7x9"])
@pytest.mark.parametrize("n", [1, 3, 64])
def test_positive_counts_are_exact(n, shape):
    rng = np.random.default_rng(n * 1000 + shape[0])
    masks = np.where(rng.random((n,) + shape) < 0.085, 255, 0).astype(np.uint8)
    # grey levels on both sides of the border, an empty and a full image
    border = rng.random((n,) + shape)
    masks[border < 0.05] = 127
    masks[border > 0.95] = 128
    masks[0] = 0
    if n > 1:
        masks[1] = 255
    got = imbalance.positive_counts(masks)
    assert got.dtype == np.int64 and got.shape == (n,)
    assert np.array_equal(got, _want(masks))
    assert got[0] == 0 and (n == 1 or got[1] == masks[1].size)
    # a device tensor goes in as it is; another threshold
    got2 = imbalance.positive_counts(torch.from_numpy(masks).cuda(), threshold=127)
    assert np.array_equal(got2, got)
    assert np.array_equal(imbalance.positive_counts(masks, threshold=200), _want(masks, 200))
    assert np.array_equal(imbalance.positive_counts(masks, threshold=255), np.zeros(n, dtype=np.int64))
    assert np.array_equal(imbalance.positive_counts(masks, threshold=-1), np.full(n, masks[0].size, dtype=np.int64))


def test_all_127_and_all_128():
    m = np.full((2, 224, 224), 127, dtype=np.uint8)
    m[1] = 128
    assert imbalance.positive_counts(m).tolist() == [0, 224 * 224]


def test_unaligned_view_takes_the_bytewise_path():
    rng = np.random.default_rng(5)
    buf = torch.from_numpy((rng.random(3 * 64 * 64 + 1) < 0.3).astype(np.uint8) * 255).cuda()
    view = buf[1:].view(3, 64, 64)            # one byte into the allocation
    assert view.data_ptr() % 16 != 0
    assert np.array_equal(imbalance.positive_counts(view), _want(view.cpu().numpy()))


def test_sample_weights_and_pos_weight_from_device_counts(golden_dir):
    g = np.load(os.path.join(golden_dir, "tiny_f4_8_focal2.npz"))
    masks = g["masks_u8"]
    batches = [masks[:5], masks[5:]]
    w = imbalance.sample_weights(batches)
    assert np.abs(w - g["sample_weights"]).max() <= 5 * 2.0 ** -23     # the reference's ratio is a float32 mean
    assert np.array_equal(w, imbalance.sample_weights(counts=g["positive_counts"], pixels=masks[0].size))
    ratio, pw = imbalance.pos_weight_from_masks(batches)
    pos = int((masks > 127).sum())
    assert ratio == pos / masks.size and pw == (1 - pos / masks.size) / (pos / masks.size)


def test_bad_masks_are_refused():
    with pytest.raises(TypeError):
        imbalance.positive_counts(np.zeros((2, 4, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        imbalance.positive_counts(np.zeros((0, 4, 4), dtype=np.uint8))
