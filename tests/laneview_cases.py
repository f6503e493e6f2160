"""TEST INFRASTRUCTURE ONLY - the small inputs of the lane view's tests, shared by tests/test_laneview_cpu.py (which
shows that they tell the model's mutants from the definition) and tests/test_laneview_gpu.py (which runs them).

Every small case has n = 3 frames and k = 4 records a frame, a different table per frame:
  frame 0   no curve: four absent records
  frame 1   one curve, which enters at the left border: x = -0.52 + 0.05 y is 16.64 / 32 below zero on row 0, where the
            floor of `>> 32` (-17: out of a thickness of 1) and a truncating division (-16: a hit) differ
  frame 2   a left curve that fills up to its neighbour and a right curve that crosses it inside the image (the area
            is empty on the crossed rows), a curve whose coefficients `quantise` refuses (recorded absent) and a curve
            that lies wholly outside the image; every curve's rows start and end inside the image
The matrix is the identity (a camera pixel is its own bird's-eye pixel) or HORIZON, whose w = m6 x + m7 y + m8 changes
sign inside the frame: rows above the horizon have w < 0 and would, divided all the same, land inside the bird's-eye
image."""
from __future__ import annotations

import numpy as np

import laneview_model as M
from unet_lane_detection_amd import laneview as LV

K = 4

# 37 x 53 and 32 x 64 camera frames onto a 48 x 40 bird's-eye image: w = 0 close to camera row 12, the rows below map
# to the bird's-eye rows 24 .. 40, the rows above (w < 0) would map to rows 0 .. 16
HORIZON = np.array([[1.7, 2.0, -68.2], [0.01, 2.0, -16.0], [0.0005, 1.0 / 12.0, -1.0]], dtype=np.float64)
HORIZON_WARP = (48, 40)

PLAIN = M.Style()
LOUD = M.Style(alpha=0.6, beta=0.5, gamma=-3.5, area=(10, 200, 30), marking=(250, 5, 128), thickness=1)


def view_config(style, **kw):
    """the ViewConfig that carries a model Style"""
    return LV.ViewConfig(alpha=style.alpha, beta=style.beta, gamma=style.gamma, area=style.area, marking=style.marking,
                         thickness=style.thickness, fill=style.draw_area, draw_mask=style.draw_marking, **kw)


def frames_of(seed, n, height, width):
    return np.random.default_rng(seed).integers(0, 256, (n, height, width, 3), dtype=np.uint8)


def masks_of(seed, n, warp_w, warp_h, level=127):
    """4 x 4 blocks of bytes on either side of the level, a third of them ON"""
    rng = np.random.default_rng(seed)
    on = rng.random((n, (warp_h + 3) // 4, (warp_w + 3) // 4)) < 0.33
    values = np.where(on, rng.choice([level + 1, 200, 255], size=on.shape), rng.choice([0, 64, level], size=on.shape))
    return np.repeat(np.repeat(values, 4, axis=1), 4, axis=2)[:, :warp_h, :warp_w].astype(np.uint8)


def _rec(coeffs, rows, fill, colour, draw=True):
    q = LV.quantise(coeffs)
    if q is None:
        return [0] * M.WORDS
    return M.record(True, fill, draw, rows[0], rows[1], q[0], q[1], q[2], colour)


def tables(warp_w, warp_h, rows=None):
    """(3, K, 8) int64: the three frames' tables for a bird's-eye image of that size; rows: the first and last row of
    frame 2's curves"""
    t = np.zeros((3, K, M.WORDS), dtype=np.int64)
    rows = (warp_h // 8, warp_h - 3) if rows is None else rows      # start and end inside the image
    t[1, 0] = _rec((0.0, 0.05, -0.52), (0, warp_h - 1), False, (255, 0, 0))
    mid = (rows[0] + rows[1]) / 2.0
    slope = 0.45 * warp_w / (rows[1] - rows[0])
    left = (0.0004, slope, 0.5 * warp_w - slope * mid - 0.0004 * mid * mid)        # crosses the right curve at `mid`
    right = (0.0, -slope, 0.5 * warp_w + slope * mid + 0.37)
    t[2, 0] = _rec(left, rows, True, (255, 0, 0))
    t[2, 1] = _rec(right, rows, True, (0, 0, 255))
    t[2, 2] = _rec((0.0, 0.0, warp_w + 40.0), rows, True, (7, 7, 7))               # right of the image on every row
    t[2, 3] = _rec((9.0, 0.0, 0.0), rows, False, (1, 2, 3))                        # a = 9 > 2^3: refused
    assert not t[2, 3].any()
    return t


def small(kind, matrix):
    """kind "scalar": 37 x 53 with step = 3 * 53 + 5; "vector": 32 x 64 dense.  matrix "identity" or "horizon".
    -> dict(frames (3, h, w, 3), step, m, warp (w, h), masks, curves)"""
    height, width = (37, 53) if kind == "scalar" else (32, 64)
    step = 3 * width + (5 if kind == "scalar" else 0)
    if matrix == "identity":
        m, warp, rows = np.eye(3), (width, height), None
    else:
        m, warp, rows = HORIZON, HORIZON_WARP, (27, 35)     # the camera sees the bird's-eye rows 24 .. 40 only
    seed = 100 * height + width + (7 if matrix == "identity" else 0)
    return dict(frames=frames_of(seed, 3, height, width), step=step, m=m, warp=warp,
                masks=masks_of(seed + 1, 3, warp[0], warp[1]), curves=tables(warp[0], warp[1], rows))


SMALL = [(kind, matrix) for kind in ("scalar", "vector") for matrix in ("identity", "horizon")]


def extreme_records():
    """coefficients at the domain bound, both signs: with Y at its largest the sums come closest to 2^63"""
    a, b, c = M.A_BOUND, M.B_BOUND, M.C_BOUND
    t = np.zeros((1, 4, M.WORDS), dtype=np.int64)
    t[0, 0] = M.record(True, True, True, 0, 2047, a, b, c, (255, 0, 0))
    t[0, 1] = M.record(True, True, True, 0, 2047, -a, -b, -c, (0, 255, 0))
    t[0, 2] = M.record(True, True, True, 0, 2047, a, -b, c, (0, 0, 255))
    t[0, 3] = M.record(True, False, True, 0, 2047, -a, b, -c, (9, 9, 9))
    return t
