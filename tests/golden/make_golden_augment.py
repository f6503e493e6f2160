"""Writes tests/golden/augment.npz from this project's own model of the augmentation stage
(unet_lane_detection_amd/augment.py): two 24 x 40 frames and their masks, a table that switches every operation on, and
the model's outputs.  The fixture pins the model; tests/test_augment_gpu.py runs the same table through the kernel.

  python tests/golden/make_golden_augment.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from unet_lane_detection_amd import augment as A  # noqa: E402


def main():
    rng = np.random.default_rng(20)
    h, w = 24, 40
    y, x = np.mgrid[0:h, 0:w]
    # smooth colour gradients plus noise, and one frame with saturated patches: every hue sector occurs
    base = np.stack([x * 6, y * 10, (x + y) * 4], axis=-1)
    images = np.stack([np.clip(base + rng.integers(-20, 21, base.shape), 0, 255),
                       rng.integers(0, 256, base.shape)]).astype(np.uint8)
    images[1, :6, :18] = np.repeat(np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]],
                                            dtype=np.uint8), 3, axis=0)[None].repeat(6, axis=0)
    masks = np.zeros((2, h, w), dtype=np.uint8)
    masks[0][np.abs(x - 10 - y // 2) <= 1] = 255          # two lane-like stripes
    masks[1][np.abs(x - 30 + y // 3) <= 1] = 200
    masks[1, 20:, :5] = 127                               # at the threshold: not a lane
    p = A.identity_params(6, [1, 0, 0, 1, 1, 0])
    for i, (flip, angle, alpha, beta, dh, ds, dv, blur) in enumerate((
            (False, 15.0, 1.3, 0.3, 30.0, 30.0, 30.0, 3), (True, -15.0, 0.7, -0.3, -30.0, -30.0, -30.0, 5),
            (True, 7.25, 1.12, -0.08, 11.5, -7.75, 19.25, 7), (False, 90.0, 0.91, 0.21, -17.5, 23.0, -4.5, 7),
            (True, 0.0, 1.05, 0.0, 90.0, 0.0, 0.0, 3), (False, -3.5, 1.0, 0.1, 3.0, 12.0, -25.0, 5))):
        A.set_geometry(p[i], flip, angle)
        p["flags"][i] |= A.FLAG_BC | A.FLAG_HSV
        p["alpha"][i], p["beta255"][i] = alpha, beta * 255.0
        p["dh"][i], p["ds"][i], p["dv"][i], p["blur"][i] = dh, ds, dv, blur
    out, tgt = A.apply_model(images, masks, p, 127)
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, images=images, masks=masks, params=np.frombuffer(p.tobytes(), dtype=np.uint8), mask_threshold=127,
                        out_images=out, out_targets=tgt)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
