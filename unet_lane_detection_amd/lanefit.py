"""Lane fit on the device: what the reference's bird's-eye warp is there for.

The reference warps every frame "to make the lane-line fit that follows easy" (README.md:3692) and lists the fit, a
curvature output and a confidence output on its roadmap (README.md:5138-5148); it has no code for them.  This is the
classic fit on the warped mask, made where the mask already is:

  the search   `unet_lane_fit_u8_batch`: a column histogram of the bottom half finds the two lane bases, windows slide
               upwards from them and recentre on the pixels they find - or, with a prior, a band around the last
               frame's curves is searched - and the lane pixels are reduced to the moment sums S_k = sum y^k and
               T_k = sum x y^k.  `lane_fit_records` enqueues it; 256 bytes per frame leave the device.
  the fit      `solve`: least squares x = a y^2 + b y + c from those exact integers, in exact rational arithmetic, each
               coefficient rounded once to double.
  the result   `LaneFits`: per frame and lane the coefficients, position, heading and radius of curvature at any row,
               a confidence (the share of windows, or of prior rows, that found pixels); per frame the lane centre
               (what `follow.LineFollower` steers on), the lane width and the lateral offset.
  tracking     `LaneTracker`: a window search on the first frame and whenever a lane was lost, the cheaper prior mode
               around the last fits otherwise.  `follow.LaneFollowPipeline(fit=FitConfig())` runs one.

The arithmetic is stated in include/unet_hip.h and, in numpy, in tests/lanefit_model.py.  There is no reference code to
be equal to: parity with any outside implementation of the sliding-window search is unpinned.  No CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

FIT_WORDS = 16            # UNET_LANE_FIT_WORDS
FIT_WINDOWS_MAX = 64      # UNET_LANE_FIT_WINDOWS_MAX
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


@dataclass(frozen=True)
class FitConfig:
    """n_windows, margin, min_pixels, level: the search (include/unet_hip.h).  min_fit_pixels: a lane with fewer pixels
    gets no coefficients.  xm_per_pix, ym_per_pix: metres per pixel of the warped image across and along the road;
    with both set `curvature_radius` is in metres."""
    n_windows: int = 9
    margin: int = 100
    min_pixels: int = 50
    level: int = 127
    min_fit_pixels: int = 3
    xm_per_pix: float | None = None
    ym_per_pix: float | None = None


def lane_fit_records(masks_dev, cfg=FitConfig(), prior=None):
    """masks (n,h,w) or (h,w) uint8 on the device -> the (n, 2, 16) record tensor of unet_lane_fit_u8_batch (int64
    storage of the unsigned words), still on the device; nothing is read back.  prior: None (window mode) or an
    (n, 2, h) int32 table, numpy or torch (prior mode); n_windows is capped at h."""
    if not isinstance(masks_dev, torch.Tensor) or not masks_dev.is_cuda or masks_dev.dtype != torch.uint8:
        raise TypeError("masks must be a uint8 torch tensor on the GPU")
    if masks_dev.dim() == 2:
        masks_dev = masks_dev[None]
    if masks_dev.dim() != 3:
        raise ValueError("masks must be (n, h, w)")
    masks_dev = masks_dev.contiguous()
    n, h, w = (int(v) for v in masks_dev.shape)
    table = None
    if prior is not None:
        table = torch.as_tensor(prior)
        if table.dtype != torch.int32 or tuple(table.shape) != (n, 2, h):
            raise ValueError("prior must be (n, 2, h) int32")
        table = table.to(masks_dev.device).contiguous()
    out = torch.empty((n, 2, FIT_WORDS), dtype=torch.int64, device=masks_dev.device)
    _lib.call("unet_lane_fit_u8_batch", masks_dev.device, masks_dev, n, h, w, int(cfg.level), min(int(cfg.n_windows), h),
              int(cfg.margin), int(cfg.min_pixels), table, out)
    return out


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def solve(S, T, min_fit_pixels=3):
    """The least-squares x = a y^2 + b y + c from S = (S0..S4), T = (T0, T1, T2): the normal equations
    [[S4,S3,S2],[S3,S2,S1],[S2,S1,S0]] (a,b,c) = (T2,T1,T0) by Cramer's rule on Python ints, each coefficient the exact
    rational rounded once to double (int / int is correctly rounded).  A singular system (fewer than three distinct
    rows) gives the exact straight line with a = 0.0, a singular line the constant T0 / S0.  None with fewer than
    min_fit_pixels pixels (or none at all)."""
    s0, s1, s2, s3, s4 = (int(v) for v in S)
    t0, t1, t2 = (int(v) for v in T)
    if s0 < max(int(min_fit_pixels), 1):
        return None
    m = [[s4, s3, s2], [s3, s2, s1], [s2, s1, s0]]
    rhs = [t2, t1, t0]
    d = _det3(m)
    if d != 0:
        num = []
        for col in range(3):
            mc = [[rhs[r] if k == col else m[r][k] for k in range(3)] for r in range(3)]
            num.append(_det3(mc))
        return num[0] / d, num[1] / d, num[2] / d
    d2 = s2 * s0 - s1 * s1
    if d2 != 0:
        return 0.0, (t1 * s0 - s1 * t0) / d2, (s2 * t0 - s1 * t1) / d2
    return 0.0, 0.0, t0 / s0


class LaneFit:
    """One lane of one frame: a record of unet_lane_fit_u8_batch and the curve fitted to it."""

    def __init__(self, words, height, cfg):
        w = [int(v) for v in np.asarray(words, dtype=np.uint64).reshape(FIT_WORDS)]
        self.words = w
        self.cfg = cfg
        self.present = bool(w[0] & 1)
        self.base, self.hit, self.tried, self.last_center = w[1], w[2], w[3], w[4]
        self.S, self.T = tuple(w[5:10]), tuple(w[10:13])
        self.pixels = w[5]
        self.y_range = (w[13], w[14]) if self.pixels else None
        self.confidence = self.hit / self.tried if self.tried else 0.0
        self.coeffs = solve(self.S, self.T, cfg.min_fit_pixels)

    def x_at(self, y):
        """a y^2 + b y + c, evaluated as a * y * y + b * y + c in float64; None without coefficients"""
        if self.coeffs is None:
            return None
        a, b, c = self.coeffs
        y = float(y)
        return a * y * y + b * y + c

    def heading(self, y):
        """atan(dx/dy) = atan(2 a y + b) in radians: 0 is straight up the image"""
        if self.coeffs is None:
            return None
        a, b, _ = self.coeffs
        return math.atan(2.0 * a * float(y) + b)

    def curvature_radius(self, y):
        """(1 + (2 a y + b)^2)^1.5 / |2 a| in pixels at row y, inf for a = 0; with cfg.xm_per_pix and cfg.ym_per_pix
        in metres, of A = a xm / ym^2, B = b xm / ym at y ym"""
        if self.coeffs is None:
            return None
        a, b, _ = self.coeffs
        y = float(y)
        xm, ym = self.cfg.xm_per_pix, self.cfg.ym_per_pix
        if xm is not None and ym is not None:
            a, b, y = a * xm / (ym * ym), b * xm / ym, y * ym
        if a == 0.0:
            return math.inf
        return (1.0 + (2.0 * a * y + b) ** 2) ** 1.5 / abs(2.0 * a)


class FrameFit:
    """The two lanes of one frame."""

    def __init__(self, left, right, height, width):
        self.left, self.right = left, right
        self.height, self.width = int(height), int(width)

    @property
    def lanes(self):
        return self.left, self.right

    def center_at(self, y):
        """the mean of the two lanes' x at row y; None unless both have coefficients"""
        xl, xr = self.left.x_at(y), self.right.x_at(y)
        if xl is None or xr is None:
            return None
        return (xl + xr) / 2.0

    def center_px(self, y):
        """int(floor(center_at(y))): what follow.LineFollower.update takes"""
        c = self.center_at(y)
        return None if c is None else int(math.floor(c))

    def lane_width(self, y):
        xl, xr = self.left.x_at(y), self.right.x_at(y)
        if xl is None or xr is None:
            return None
        return xr - xl

    def offset(self, y):
        """the lane centre's distance from the image centre width // 2 (positive: the lane lies to the right)"""
        c = self.center_at(y)
        return None if c is None else c - (self.width // 2)


class LaneFits:
    """The records of `unet_lane_fit_u8_batch` for n frames on the host, and what is read off them: `fits[i].left`,
    `fits[i].right` (LaneFit), `fits[i].center_px(y)`, ..."""

    def __init__(self, frames, words, height, width, cfg):
        self.frames, self.words = frames, words
        self.height, self.width, self.cfg = int(height), int(width), cfg

    @classmethod
    def from_records(cls, words, height, width, cfg=FitConfig()):
        """words: (n, 2, 16) - the device's int64 storage read back, or uint64"""
        w = np.ascontiguousarray(np.asarray(words)).view(np.uint64).reshape(-1, 2, FIT_WORDS)
        frames = [FrameFit(LaneFit(f[0], height, cfg), LaneFit(f[1], height, cfg), height, width) for f in w]
        return cls(frames, w, height, width, cfg)

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i]

    def __iter__(self):
        return iter(self.frames)


def prior_table(fits, height):
    """LaneFits -> the (n, 2, height) int32 table of prior mode: floor(x_at(y) + 0.5) in float64, clipped to int32;
    -1 (not searched) for a lane without coefficients."""
    height = int(height)
    ys = np.arange(height, dtype=np.float64)
    table = np.full((len(fits), 2, height), -1, dtype=np.int32)
    for i, frame in enumerate(fits):
        for s, lane in enumerate(frame.lanes):
            if lane.coeffs is None:
                continue
            a, b, c = (np.float64(v) for v in lane.coeffs)
            x = np.floor(a * ys * ys + b * ys + c + 0.5)
            table[i, s] = np.clip(x, float(INT32_MIN), float(INT32_MAX)).astype(np.int64).astype(np.int32)
    return table


def lane_fits(masks_dev, cfg=FitConfig(), prior=None):
    """masks on the device -> LaneFits; 256 bytes per frame are read back."""
    h, w = int(masks_dev.shape[-2]), int(masks_dev.shape[-1])
    return LaneFits.from_records(lane_fit_records(masks_dev, cfg, prior).cpu().numpy(), h, w, cfg)


class LaneTracker:
    """One frame at a time: a window search on the first frame and whenever a lane of the last result has no
    coefficients or a confidence below min_confidence, prior mode around the last fits otherwise.  `mode` is what ran
    last ("window" or "prior"), `modes` the whole sequence.  source(mask, cfg, prior) -> (1, 2, 16) words replaces the
    device call (tests)."""

    def __init__(self, cfg=FitConfig(), min_confidence=0.5, source=None):
        self.cfg, self.min_confidence = cfg, float(min_confidence)
        self._source = source if source is not None else (lambda mask, c, prior: lane_fit_records(mask, c, prior).cpu().numpy())
        self.last = None
        self.mode = None
        self.modes = []

    def _trusted(self):
        if self.last is None:
            return False
        return all(l.coeffs is not None and l.confidence >= self.min_confidence for l in self.last[0].lanes)

    def update(self, mask_dev):
        """mask (h, w) -> LaneFits of that one frame"""
        h, w = int(mask_dev.shape[-2]), int(mask_dev.shape[-1])
        prior = prior_table(self.last, h) if self._trusted() else None
        self.mode = "window" if prior is None else "prior"
        self.modes.append(self.mode)
        self.last = LaneFits.from_records(self._source(mask_dev, self.cfg, prior), h, w, self.cfg)
        return self.last

    def reset(self):
        self.last = None
