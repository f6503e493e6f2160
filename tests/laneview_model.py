"""TEST INFRASTRUCTURE ONLY - numpy restatement of unet_lane_view_u8_batch (include/unet_hip.h), which the HIP kernel
is compared with bit for bit.

  the position   float64 operations in the stated order (numpy contracts nothing): w = m6 x + m7 y + m8, a pixel with
                 !(w > 0) is OUTSIDE; fx = (m0 x + m1 y + m2) * (32 / w), fy likewise; fmax / fmin clamp to
                 [-2^31, 2^31 - 1] (a NaN becomes -2^31, as C's fmax gives it); rint.
  the curves     int64 integers, after the clamp the header prints; A Y^2 + B Y + C stays below 2^63 (the CPU test
                 checks that bound in Python ints), `>> 32` is numpy's arithmetic shift.
  the mask       oracle.camera_oracle._sample: the one-channel bilinear sample of cv2.warpPerspective as the oracle
                 restates it, at the fixed-point position, thresholded.
  the blend      the fp32 steps of unet_overlay_u8_batch, one rounding each.

The keyword arguments after `style` switch single clauses of the definition to a plausible wrong reading; the CPU test
shows that its cases tell every such mutant from the definition.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import camera_oracle as K

WORDS = 8     # UNET_LANE_VIEW_WORDS
MAX = 8       # UNET_LANE_VIEW_MAX
A_BOUND, B_BOUND, C_BOUND = (1 << 30) - 1, (1 << 45) - 1, (1 << 57) - 1
Y_LIMIT = 1 << 16   # an INSIDE pixel has 0 <= Y < 32 * 2048


@dataclass(frozen=True)
class Style:
    """unet_lane_view_style; the defaults are those of a NULL style"""
    alpha: float = 0.7
    beta: float = 0.3
    gamma: float = 0.0
    area: tuple = (0, 255, 0)
    marking: tuple = (0, 255, 0)
    thickness: int = 4
    draw_area: bool = True
    draw_marking: bool = True


def record(present=True, fill=False, draw=True, y0=0, y1=0, A=0, B=0, C=0, colour=(255, 0, 0)):
    """one curve record as eight ints"""
    flags = (1 if present else 0) | (2 if fill else 0) | (4 if draw else 0)
    return [flags, int(y0), int(y1), int(A), int(B), int(C), int(colour[0]) | int(colour[1]) << 8 | int(colour[2]) << 16, 0]


def positions(m, width, height, horizon="gt"):
    """-> (valid, X, Y) of every camera pixel, (height, width) each: valid is w > 0, X and Y int64 in 1/32 pixel"""
    m = np.asarray(m, dtype=np.float64).reshape(3, 3)
    ys, xs = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    w = m[2, 0] * xs + m[2, 1] * ys + m[2, 2]
    valid = (w > 0.0) if horizon == "gt" else (w != 0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = 32.0 / w
        fx = (m[0, 0] * xs + m[0, 1] * ys + m[0, 2]) * s
        fy = (m[1, 0] * xs + m[1, 1] * ys + m[1, 2]) * s
    fx = np.fmin(np.fmax(fx, -2147483648.0), 2147483647.0)
    fy = np.fmin(np.fmax(fy, -2147483648.0), 2147483647.0)
    return valid, np.rint(fx).astype(np.int64), np.rint(fy).astype(np.int64)


def clamp_records(table, warp_h):
    """(k, 8) int64 words -> flags, lo, hi (rows in 1/32 pixel), A, B, C, colour as the kernel uses them"""
    t = np.asarray(table).astype(np.int64).reshape(-1, WORDS)
    flags = t[:, 0] & 7
    y0 = np.clip(t[:, 1], 0, warp_h - 1)
    y1 = np.clip(t[:, 2], 0, warp_h - 1)
    return (flags, 32 * y0, 32 * y1 + 31, np.clip(t[:, 3], -A_BOUND, A_BOUND), np.clip(t[:, 4], -B_BOUND, B_BOUND),
            np.clip(t[:, 5], -C_BOUND, C_BOUND), t[:, 6] & 0xFFFFFF)


def x32(A, B, C, Y, shift="arith"):
    v = A * Y * Y + B * Y + C
    if shift == "arith":
        return v >> 32
    return np.sign(v) * (np.abs(v) >> 32)      # the mutant: a division that truncates towards zero


def frame_layers(m, width, height, warp_w, warp_h, mask, level, table, style, shift="arith", priority="curves",
                 horizon="gt"):
    """-> (layers (height, width) uint8, colour (height, width, 3) uint8, meaningless on layer 0)"""
    valid, X, Y = positions(m, width, height, horizon)
    inside = valid & (X >= 0) & (X < 32 * warp_w) & (Y >= 0) & (Y < 32 * warp_h)
    Yc = np.where(inside, Y, 0)                      # the curves are evaluated on INSIDE pixels only: Y < 2^16
    layers = np.zeros((height, width), dtype=np.int64)
    colour = np.zeros((height, width, 3), dtype=np.uint8)

    def paint(where, number, rgb):
        layers[where] = number
        colour[where] = rgb

    k = 0 if table is None else int(np.asarray(table).reshape(-1, WORDS).shape[0])
    covers, xs = [], []
    if k:
        flags, lo, hi, A, B, C, cols = clamp_records(table, warp_h)
        for i in range(k):
            covers.append(inside & bool(flags[i] & 1) & (Y >= lo[i]) & (Y <= hi[i]))
            xs.append(x32(A[i], B[i], C[i], Yc, shift))
    area = np.zeros((height, width), dtype=bool)
    for i in range(k - 1):
        if flags[i] & 2:
            area |= covers[i] & covers[i + 1] & (xs[i] <= X) & (X <= xs[i + 1])
    if style.draw_area:
        paint(area, 1, style.area)
    marking = np.zeros((height, width), dtype=bool)
    if mask is not None and style.draw_marking:
        sample = K._sample(np.asarray(mask, dtype=np.uint8)[..., None], X, Y)[..., 0]
        marking = inside & (sample.astype(np.int64) > level)
    if priority == "curves":
        paint(marking, 2, style.marking)
    for i in reversed(range(k)):                     # the lowest i is painted last: it wins
        if flags[i] & 4:
            hit = covers[i] & (np.abs(X - xs[i]) <= 16 * style.thickness)
            paint(hit, 3 + i, [(int(cols[i]) >> (8 * c)) & 255 for c in range(3)])
    if priority != "curves":                         # the mutant: the mask over the curves
        paint(marking, 2, style.marking)
    return layers.astype(np.uint8), colour


def blend(frame, colour, style):
    f = frame.astype(np.float32)
    v = f * np.float32(style.alpha)
    v = v + colour.astype(np.float32) * np.float32(style.beta)
    v = v + np.float32(style.gamma)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def lane_view(frames, m, warp_w, warp_h, masks=None, level=127, curves=None, style=Style(), shift="arith",
              priority="curves", horizon="gt", blend_all=True):
    """frames (n, height, width, 3) uint8 (the pixels only: no row padding), masks (n, warp_h, warp_w) or None,
    curves (n, k, 8) int64 or None -> (view (n, height, width, 3) uint8, layers (n, height, width) uint8)"""
    frames = np.asarray(frames, dtype=np.uint8)
    n, height, width = frames.shape[:3]
    view = np.empty_like(frames)
    layers = np.empty((n, height, width), dtype=np.uint8)
    for f in range(n):
        lay, colour = frame_layers(m, width, height, warp_w, warp_h, None if masks is None else masks[f], level,
                                   None if curves is None else curves[f], style, shift, priority, horizon)
        colour = np.where((lay == 0)[..., None], frames[f], colour)
        out = blend(frames[f], colour, style)
        if not blend_all:                            # the mutant: layer-0 pixels are copied
            out = np.where((lay == 0)[..., None], frames[f], out)
        view[f], layers[f] = out, lay
    return view, layers
