"""Lane view on the device: the bird's-eye results drawn where the camera looks.

The lane fit and the lane instances live in the 1055x685 warped image.  The reference's own pictures of a result are
camera-view overlays (assets/demo/normal_unet.jpg), its debugging advice is `visualize_output` (README.md:4563-4593:
green where the mask is set, cv2.addWeighted(img, 0.7, overlay, 0.3, 0)) and its roadmap lists "lane + drivable
area" (README.md:5150-5153); it has no code that goes back through the IPM.  This is the step that closes a
sliding-window lane fit, made where the frame, the mask and the curves already are:

  the kernel    `unet_lane_view_u8_batch`: per camera pixel forward through the perspective matrix, then the curves
                (fixed point, 64-bit integers), the mask (the bilinear sample of warpPerspective, thresholded) and the
                area between neighbouring curves decide its layer, and the layer's colour is blended onto the frame
                with the addWeighted of `unet_overlay_u8_batch`.  `lane_view` enqueues it; nothing is read back.
  the table     `curve_table`: `lanefit.LaneFits` (left and right, the lane area between them) or the lists of
                `instances.lane_instances` (any number of markings, the area between neighbours) as the kernel's
                64-byte records; `quantise` turns one curve's float coefficients into its integers.
  the pipeline  `follow.LaneFollowPipeline(view=ViewConfig())`.

The arithmetic is stated in include/unet_hip.h and, in numpy, in tests/laneview_model.py.  Parity of the mask layer
with cv2.warpPerspective itself is unpinned.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

VIEW_WORDS = 8            # UNET_LANE_VIEW_WORDS
VIEW_MAX = 8              # UNET_LANE_VIEW_MAX
LAYER_AREA, LAYER_MARKING, LAYER_CURVE = 1, 2, 3      # the layer plane: 3 + i is curve record i
A_LIMIT, B_LIMIT, C_LIMIT = 1 << 30, 1 << 45, 1 << 57     # |A|, |B|, |C| stay below these


@dataclass(frozen=True)
class ViewConfig:
    """alpha, beta, gamma, area, marking, thickness: the style (include/unet_hip.h); colours are in the frame's own
    channel order.  curve_colours: the colour of curve i is curve_colours[i % len].  extent "frame": a curve is valid
    on every row of the bird's-eye image; "pixels": only on the rows its pixels span (LaneFit.y_range, or the box of
    an instance).  draw_mask, draw_curves, fill: the marking layer, the curve layers and the area layer.  level: a
    mask sample above it is a marking."""
    alpha: float = 0.7
    beta: float = 0.3
    gamma: float = 0.0
    area: tuple = (0, 255, 0)
    marking: tuple = (0, 255, 0)
    curve_colours: tuple = ((255, 0, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255))
    thickness: int = 4
    extent: str = "frame"
    draw_mask: bool = True
    draw_curves: bool = True
    fill: bool = True
    level: int = 127

    def __post_init__(self):
        if self.extent not in ("frame", "pixels"):
            raise ValueError(f"extent={self.extent!r}: \"frame\" or \"pixels\"")

    def style(self):
        """the unet_lane_view_style the kernel's entry point takes"""
        s = _lib.LaneViewStyle()
        s.alpha, s.beta, s.gamma = float(self.alpha), float(self.beta), float(self.gamma)
        for c in range(3):
            s.area[c], s.marking[c] = int(self.area[c]), int(self.marking[c])
        s.thickness = int(self.thickness)
        s.layers = (1 if self.fill else 0) | (2 if self.draw_mask else 0)
        return s


def quantise(coeffs):
    """(a, b, c) of x = a y^2 + b y + c in pixels -> the record's (A, B, C) = (rint(a 2^27), rint(b 2^32),
    rint(c 2^37)) as Python ints, round half to even; None where one of them is not finite or leaves the kernel's
    domain |A| < 2^30, |B| < 2^45, |C| < 2^57 (such a lane is recorded absent)."""
    if coeffs is None:
        return None
    out = []
    for value, bits, limit in zip(coeffs, (27, 32, 37), (A_LIMIT, B_LIMIT, C_LIMIT)):
        value = float(value)
        if not math.isfinite(value):
            return None
        try:
            scaled = math.ldexp(value, bits)    # exact: a power of two
        except OverflowError:
            return None
        if not math.isfinite(scaled):
            return None
        q = round(scaled)                       # Python rounds a float half to even, exactly
        if abs(q) >= limit:
            return None
        out.append(q)
    return tuple(out)


def orient(matrix, warp_size):
    """A perspective matrix is defined up to a factor, the kernel's horizon test `w > 0` is not: -M is the same
    homography with the other side of the horizon in front.  cv2.getPerspectiveTransform fixes m8 = 1, which for the
    reference's calibration makes w negative on the whole road.  Returns M or -M (the negation is exact), whichever
    has w > 0 at the camera position of the bird's-eye image's centre."""
    m = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
    p = np.linalg.solve(m, np.array([warp_size[0] / 2.0, warp_size[1] / 2.0, 1.0]))
    # p = the camera position (homogeneous) up to the factor 1 / w: M p = (X, Y, 1), so w of the pixel p / p[2] is 1 / p[2]
    return m.copy() if p[2] > 0.0 else -m


def _record(coeffs, rows, fill, cfg, index, warp_h):
    q = quantise(coeffs)
    if q is None or rows is None:
        return [0] * VIEW_WORDS
    y0, y1 = (0, warp_h - 1) if cfg.extent == "frame" else (int(rows[0]), int(rows[1]))
    y0, y1 = max(0, min(y0, warp_h - 1)), max(0, min(y1, warp_h - 1))
    if y0 > y1:
        return [0] * VIEW_WORDS
    colour = cfg.curve_colours[index % len(cfg.curve_colours)]
    flags = 1 | (2 if fill and cfg.fill else 0) | (4 if cfg.draw_curves else 0)
    return [flags, y0, y1, q[0], q[1], q[2], int(colour[0]) | int(colour[1]) << 8 | int(colour[2]) << 16, 0]


def curve_table(fits_or_instances, warp_size, cfg=ViewConfig()):
    """-> the (n, k, 8) int64 numpy table `lane_view` takes.  warp_size: (width, height) of the bird's-eye image.
    From `lanefit.LaneFits`: k = 2, the left lane then the right one, the area filled between them.  From the result
    of `instances.lane_instances` (per frame a list of LaneInstance, left to right): the first UNET_LANE_VIEW_MAX
    markings of every frame, the area filled between neighbours; k is the fullest frame's count (0 if there is none:
    pass `curves=None` then).  A curve without coefficients, or whose coefficients `quantise` refuses, is recorded
    absent, and so is one without pixels when extent is "pixels"."""
    from .lanefit import LaneFits
    warp_h = int(warp_size[1])
    frames = []
    if isinstance(fits_or_instances, LaneFits):
        for frame in fits_or_instances:
            rows = [lane.y_range if cfg.extent == "pixels" else (0, warp_h - 1) for lane in frame.lanes]
            frames.append([_record(lane.coeffs, rows[s], s == 0, cfg, s, warp_h) for s, lane in enumerate(frame.lanes)])
    else:
        for frame in fits_or_instances:
            kept = list(frame)[:VIEW_MAX]
            frames.append([_record(inst.fit.coeffs, (inst.bbox[2], inst.bbox[3]), i + 1 < len(kept), cfg, i, warp_h)
                           for i, inst in enumerate(kept)])
    k = max((len(f) for f in frames), default=0)
    table = np.zeros((len(frames), k, VIEW_WORDS), dtype=np.int64)
    for i, f in enumerate(frames):
        for j, words in enumerate(f):
            table[i, j] = words
    return table


def lane_view(frames_dev, matrix, warp_size, masks_dev=None, curves=None, cfg=ViewConfig(), step=None, layers=False,
              width=None):
    """The camera frames with the lane area, the markings and the curves blended onto them: the (n, height, width, 3)
    uint8 tensor on the device; with layers=True also the (n, height, width) uint8 layer plane (0 nothing, 1 the lane
    area - the drivable-area mask in camera view -, 2 a marking, 3 + i curve i).  Enqueued on torch's current stream;
    nothing is read back.

    frames_dev: (n, height, width, 3) or (height, width, 3) uint8 on the device.  With `step` it is raw rows instead:
    (n, height, step) or (height, step) uint8 together with `width=`, the first 3 * width bytes of a row being pixels
    (a sensor_msgs/Image with its step).  matrix: 3 x 3, camera -> bird's-eye (ros_bridge.get_perspective_transform);
    it is passed on as `orient` returns it, so that the ground the bird's-eye image shows lies below the horizon.
    warp_size: (width, height) of the bird's-eye image.  masks_dev: (n, warp_h, warp_w) or (warp_h, warp_w) uint8 on
    the device, or None.  curves: the table of `curve_table`, numpy or torch, or None.

    With matrix=np.eye(3) and warp_size=(width, height) a camera pixel is its own bird's-eye pixel: the same call
    draws onto the bird's-eye image itself."""
    if not isinstance(frames_dev, torch.Tensor) or not frames_dev.is_cuda or frames_dev.dtype != torch.uint8:
        raise TypeError("frames must be a uint8 torch tensor on the GPU")
    dev = frames_dev.device
    frames_dev = frames_dev.contiguous()
    if step is None:
        if frames_dev.dim() == 3:
            frames_dev = frames_dev[None]
        if frames_dev.dim() != 4 or frames_dev.shape[3] != 3:
            raise ValueError("frames must be (n, h, w, 3)")
        n, h, w = (int(v) for v in frames_dev.shape[:3])
        step = 3 * w
    else:
        if width is None:
            raise ValueError("raw rows need width=")
        if frames_dev.dim() == 2:
            frames_dev = frames_dev[None]
        if frames_dev.dim() != 3 or int(frames_dev.shape[2]) != int(step):
            raise ValueError("raw rows must be (n, h, step)")
        n, h = (int(v) for v in frames_dev.shape[:2])
        w, step = int(width), int(step)
    warp_w, warp_h = int(warp_size[0]), int(warp_size[1])
    if masks_dev is not None:
        if not isinstance(masks_dev, torch.Tensor) or masks_dev.dtype != torch.uint8 or masks_dev.device != dev:
            raise TypeError("masks must be a uint8 torch tensor on the frames' device")
        if masks_dev.dim() == 2:
            masks_dev = masks_dev[None]
        if tuple(masks_dev.shape) != (n, warp_h, warp_w):
            raise ValueError("masks must be (n, warp_h, warp_w)")
        masks_dev = masks_dev.contiguous()
    table, k = None, 0
    if curves is not None:
        table = torch.as_tensor(curves)
        if table.dtype != torch.int64 or table.dim() != 3 or table.shape[0] != n or table.shape[2] != VIEW_WORDS:
            raise ValueError("curves must be (n, k, 8) int64")
        k = int(table.shape[1])
        table = table.to(dev).contiguous() if k else None
    m = np.ascontiguousarray(orient(matrix, warp_size).reshape(9))
    style = cfg.style()
    view = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    plane = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if layers else None
    _lib.call("unet_lane_view_u8_batch", dev, frames_dev, n, h, w, step, m.ctypes.data_as(C.POINTER(C.c_double)), warp_w,
              warp_h, masks_dev, int(cfg.level), table, k, C.byref(style), view, plane)
    return (view, plane) if layers else view
