"""Lane following on the device: what the reference does with a frame besides the network.

  the baseline   `extract_white_lanes` of the reference's follow_line.py (README.md:206-227) - cvtColor(BGR2HSV),
                 inRange([0,0,185], [180,40,255]), morphologyEx CLOSE and OPEN with a 5x5 box - is the method the U-Net
                 is measured against ("U-Net 0.847 IoU against HSV 0.652", README.md:4208-4215).  `HSVLaneExtractor`
                 runs it in one kernel (`unet_hsv_lanes_u8_batch`) and scores it through the same counters as
                 `UNetHIP.sweep`, so both methods are graded on the same frames and targets.
  the consumer   `LineFollower` (README.md:4068-4126) reduces the published mask to one number - the mean x of the
                 pixels above 127 on the scan row at 70 % height, if there are more than 10 - and steers on it with a
                 PID.  `lane_centers` computes count and sum on the device (`unet_lane_center_u8_batch`): 8 bytes per
                 scan row leave it instead of the whole mask.  `LineFollower` here is that PID in plain Python.
  the callback   `LaneFollowPipeline`: ImageMsg -> centres, with the network ("IPM + U-Net") or with the extractor on
                 the warped frame ("IPM only", README.md:123-135).

The arithmetic is stated in include/unet_hip.h and, in numpy, in tests/follow_model.py.  The HSV plane is
`augment.rgb_to_hsv`; parity with cv2's own BGR2HSV is unpinned.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

LANE_ROWS_MAX = 64      # UNET_LANE_ROWS_MAX
BOX_SIZES = (1, 3, 5, 7)


class HSVLaneExtractor:
    """The reference's colour-threshold lane extractor on the device; the defaults are its constants."""

    def __init__(self, lower=(0, 0, 185), upper=(180, 40, 255), close_ksize=5, open_ksize=5, device=0):
        if not torch.cuda.is_available():
            raise RuntimeError("the extractor needs a HIP device; there is no CPU fallback")
        self.lower = np.ascontiguousarray(lower, dtype=np.uint8).reshape(3)
        self.upper = np.ascontiguousarray(upper, dtype=np.uint8).reshape(3)
        if int(close_ksize) not in BOX_SIZES or int(open_ksize) not in BOX_SIZES:
            raise ValueError(f"close_ksize and open_ksize must be one of {BOX_SIZES}")
        self.close_ksize, self.open_ksize = int(close_ksize), int(open_ksize)
        self._lib = _lib.load()
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))

    def extract(self, frames_u8, bgr=True):
        """frames (n,h,w,3) or (h,w,3) uint8, numpy or torch -> masks (n,h,w) uint8 of 0 / 255 on the device."""
        frames = torch.as_tensor(frames_u8)
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("frames must be (n, h, w, 3) uint8")
        frames = frames.to(self.device).contiguous()
        n, h, w = (int(v) for v in frames.shape[:3])
        out = torch.empty((n, h, w), dtype=torch.uint8, device=self.device)
        _lib.call("unet_hsv_lanes_u8_batch", self.device, frames, n, h, w, 1 if bgr else 0,
                  self.lower.ctypes.data_as(C.c_void_p), self.upper.ctypes.data_as(C.c_void_p), self.close_ksize,
                  self.open_ksize, out)
        return out

    def evaluate(self, frames, targets, batch=None, bgr=True):
        """The baseline's confusion counts on frames (n,h,w,3) uint8 and targets (anything UNetHIP.sweep takes, one
        value per pixel): a metrics.ThresholdSweep at the single threshold 0.5 over mask / 255, so `.at(0.5)` gives
        IoU, precision, recall and F1 next to `UNetHIP.sweep(...).at(0.5)`."""
        from . import metrics
        return metrics.sweep_batches(self._lib, self.device, frames, targets, batch, (0.5,), "probability",
                                     lambda: _lib.stream(self.device),
                                     lambda f: self.extract(f, bgr=bgr).to(torch.float32) / 255.0)


def lane_sums(masks_dev, scan_rows, level=127):
    """masks (n,h,w) uint8 on the device -> (n, rows, 2) uint32 device tensor: count and sum of the x above `level` on
    every scan row (unet_lane_center_u8_batch); nothing is read back."""
    if not isinstance(masks_dev, torch.Tensor) or not masks_dev.is_cuda or masks_dev.dtype != torch.uint8:
        raise TypeError("masks must be a uint8 torch tensor on the GPU")
    if masks_dev.dim() == 2:
        masks_dev = masks_dev[None]
    if masks_dev.dim() != 3:
        raise ValueError("masks must be (n, h, w)")
    masks_dev = masks_dev.contiguous()
    n, h, w = (int(v) for v in masks_dev.shape)
    rows = np.ascontiguousarray(scan_rows, dtype=np.int32).reshape(-1)
    out = torch.empty((n, rows.size, 2), dtype=torch.int32, device=masks_dev.device)   # the kernel's uint32 pairs
    _lib.call("unet_lane_center_u8_batch", masks_dev.device, masks_dev, n, h, w, rows.ctypes.data_as(C.POINTER(C.c_int)),
              int(rows.size), int(level), out)
    return out


def centers_from_sums(sums, min_pixels=10):
    """(n, rows, 2) counts and sums on the host -> list (n) of lists (rows): sum // count where count > min_pixels,
    else None.  int(np.mean(xs)) of the reference equals sum // count."""
    s = np.asarray(sums).astype(np.int64) & 0xFFFFFFFF
    return [[int(c[1] // c[0]) if c[0] > min_pixels else None for c in frame] for frame in s]


def lane_centers(masks_dev, scan_rows=None, level=127, min_pixels=10):
    """`find_lane_center` for every frame and scan row: list (n) of lists (rows) of the centre x or None.  The default
    row is int(h * 0.7).  8 bytes per (frame, row) are read back."""
    h = int(masks_dev.shape[-2])
    rows = [int(h * 0.7)] if scan_rows is None else [int(r) for r in np.asarray(scan_rows).reshape(-1)]
    return centers_from_sums(lane_sums(masks_dev, rows, level).cpu().numpy(), min_pixels)


class LineFollower:
    """The reference's PID around the lane centre (`mask_callback`, README.md:4087-4113), state included: plain Python
    arithmetic on the host."""

    def __init__(self, kp=0.005, ki=0.0001, kd=0.001, linear_x=0.3):
        self.kp, self.ki, self.kd, self.linear_x = kp, ki, kd, linear_x
        self.error_sum = 0
        self.last_error = 0

    def update(self, center_x, width):
        """-> (linear_x, angular_z), or None (and no change of state) when there is no centre."""
        if center_x is None:
            return None
        error = center_x - width // 2
        self.error_sum += error
        error_diff = error - self.last_error
        angular_z = -(self.kp * error + self.ki * self.error_sum + self.kd * error_diff)
        self.last_error = error
        return self.linear_x, angular_z


class LaneFollowPipeline:
    """ImageMsg -> the lane centre of every scan row (list of x or None), without the mask leaving the device.

    source "unet": LanePipelineGPU's steps up to the resized mask (warp + resize, network, threshold, resize back),
    then the centre kernel; `process(msg, return_mask=True)` also returns the mono8 message LanePipelineGPU.process
    publishes, byte for byte.  source "hsv": the warp at full warp size, the extractor, the centre - the reference's
    "IPM only" path; `model` may then be None (`device=` picks the GPU).

    diagnose=True: the message's rows, already on the device for the warp, are also measured there
    (diagnose.frame_records with the message's `step`; no second upload), and `process` returns (result,
    diagnose.FrameStats) - brightness and sharpness of the camera frame beside the centres.  The centres, the mask
    and every launch of the plain path are the same with it on or off.

    fit=lanefit.FitConfig(...): the mask the centres come from is also fitted where it lies (lanefit.LaneTracker: a
    window search, then the prior mode around the last fits), and `process` returns (result, lanefit.LaneFits) - both
    lanes' curves, heading, curvature and confidence beside the centres; 256 more bytes leave the device.  With
    `diagnose` that pair comes first of the outer pair.  fit=None: every launch and every return value as without it.

    clean=instances.CleanConfig(...): the mask is labelled on the device and only the components the config keeps
    (min_area, min_height, min_width, keep_largest) stay in it, before the scan-row centres, the fit and return_mask
    see it: speckle no longer counts.  Return shapes are unchanged; `last_components` holds the frame's
    instances.Components (128 bytes per recorded component and 32 per frame leave the device).  clean=None: every
    launch and every return value as without it.

    view=laneview.ViewConfig(...): after the centres, the fit and the clean-up, the message's rows (still on the
    device), the pipeline's `matrix`, the mask and the curves go through laneview.lane_view: the lane area, the
    markings and the curves drawn in the camera frame.  The curves are the tracker's fits if there is a `fit`,
    otherwise the kept components of `clean`; with neither, only the mask layer is drawn.  `last_view` holds the
    (1, height, width, 3) device tensor and `last_view_layers` the layer plane, as `last_components` holds the
    components; `view_msg()` returns the view as an ImageMsg in the message's encoding.  Return shapes are unchanged.
    view=None: every launch and every return value as without it.

    correct=correct.CorrectConfig(...): the message's rows are corrected on the device (correct.FrameCorrector: white
    balance, stretch, tone, CLAHE, decided from the frame's own histograms) into a buffer of the pipeline's own, and
    the warp reads that buffer - for both sources.  `diagnose` still measures the raw rows (it diagnoses the camera)
    and `view` still draws on them (what the camera saw).  `last_correction` holds the frame's correct.Plan (32
    bytes leave the device when it is read).  Return shapes are unchanged.  correct=None: every launch, every buffer
    and every return value as without it."""

    def __init__(self, model, source="unet", extractor=None, scan_rows=None, level=127, min_pixels=10, device=None,
                 diagnose=False, fit=None, clean=None, view=None, correct=None, **pipeline_kwargs):
        from .ros_bridge import REF_DST_POINTS, REF_SRC_POINTS, REF_WARP_SIZE, CameraStage, LanePipelineGPU, \
            get_perspective_transform
        if source not in ("unet", "hsv"):
            raise ValueError(f"source={source!r}: \"unet\" or \"hsv\"")
        self.source = source
        self.scan_rows = None if scan_rows is None else [int(r) for r in scan_rows]
        self.level, self.min_pixels = int(level), int(min_pixels)
        self.diagnose = bool(diagnose)
        self._frame_records = None   # diagnose: the record of the message in flight, on the device
        self.fit = fit
        self.tracker = None
        if fit is not None:
            from .lanefit import LaneTracker
            self.tracker = LaneTracker(fit)
        self.clean = clean
        self.last_components = None
        self.view = view
        self.last_view = self.last_view_layers = None
        self._rows = self._view_msg = None   # view: the rows of the message in flight, and what view_msg() copies from it
        if source == "unet":
            if model is None:
                raise ValueError("source \"unet\" needs a model")
            self.pipe = LanePipelineGPU(model, **pipeline_kwargs)
            self.stage, self.matrix, self.warp_size = self.pipe.stage, self.pipe.matrix, self.pipe.warp_size
            self.extractor = None
        else:
            self.pipe = None
            index = model.device.index if model is not None else int(device or 0)
            self.stage = CameraStage(index)
            self.matrix = get_perspective_transform(pipeline_kwargs.get("src_points", REF_SRC_POINTS),
                                                    pipeline_kwargs.get("dst_points", REF_DST_POINTS))
            self.warp_size = tuple(pipeline_kwargs.get("warp_size", REF_WARP_SIZE))
            self.extractor = extractor if extractor is not None else HSVLaneExtractor(device=index)
        self.correct = correct
        self.corrector = self._corrected = None   # correct: the stage and the buffer the warp then reads
        if correct is not None:
            from .correct import FrameCorrector
            self.corrector = FrameCorrector(correct, device=self.stage.device)

    def _prestage(self, msg, out_size):
        """the message's bytes -> (1, out_h, out_w, 3) RGB on the device, as LanePipelineGPU does it"""
        from .ros_bridge import LanePipelineGPU
        rows = LanePipelineGPU.msg_to_device(self, msg)
        if self.view is not None:
            self._rows = rows
        if self.diagnose:
            from .diagnose import frame_records
            self._frame_records = frame_records(rows.view(-1), 1, msg.height, msg.width, msg.step,
                                                msg.encoding == "bgr8")
        if self.corrector is not None:
            if self._corrected is None or self._corrected.shape != rows.shape:
                self._corrected = torch.empty_like(rows)
            rows = self.corrector.correct(rows, bgr=msg.encoding == "bgr8", row_stride=msg.step, out=self._corrected,
                                          width=msg.width)
        frame = torch.empty((1, out_size[1], out_size[0], 3), dtype=torch.uint8, device=self.stage.device)
        minv = np.ascontiguousarray(np.linalg.inv(self.matrix))
        _lib.call("unet_ipm_prestage_u8", self.stage.device, rows, msg.height, msg.width, msg.step,
                  1 if msg.encoding == "bgr8" else 0, minv.ctypes.data_as(C.POINTER(C.c_double)), self.warp_size[0],
                  self.warp_size[1], out_size[0], out_size[1], frame)
        return frame

    def mask_on_device(self, msg):
        """(warp_h, warp_w) uint8 on the device: the mask the centre is taken from"""
        if self.source == "hsv":
            return self.extractor.extract(self._prestage(msg, self.warp_size), bgr=False)[0]
        frame = self._prestage(msg, self.pipe.input_size)
        mask = self.pipe._infer(frame, self.pipe.on_error == "reference")
        if mask is None:   # a guarded inference failure: the reference publishes zeros of the warped size
            return torch.zeros((self.warp_size[1], self.warp_size[0]), dtype=torch.uint8, device=self.stage.device)
        return self.stage.resize(mask[0], self.warp_size)

    def _draw_view(self, msg, mask, fits, keep):
        from .laneview import curve_table, lane_view
        curves = None
        if fits is not None:
            curves = curve_table(fits, self.warp_size, self.view)
        elif keep is not None:
            from .instances import instances_of
            m = self.last_components.recorded(0)
            curves = curve_table(instances_of(self.last_components, keep[:, :m].cpu().numpy()), self.warp_size, self.view)
        rows, self._rows = self._rows, None
        self.last_view, self.last_view_layers = lane_view(rows, self.matrix, self.warp_size, mask, curves, self.view,
                                                          step=msg.step, layers=True, width=msg.width)
        self._view_msg = (msg.encoding, msg.header)

    @property
    def last_correction(self):
        """correct: the correct.Plan of the last message (gains, lo, hi, corrected); None without `correct` or before
        the first callback"""
        return None if self.corrector is None else self.corrector.plan()

    def view_msg(self):
        """The last view as an ImageMsg in its message's encoding (height * width * 3 bytes leave the device); None
        before the first callback with `view`."""
        from .ros_bridge import ImageMsg
        if self.last_view is None:
            return None
        host = self.last_view[0].cpu().numpy()
        return ImageMsg(height=host.shape[0], width=host.shape[1], encoding=self._view_msg[0], data=host.tobytes(),
                        step=host.shape[1] * 3, is_bigendian=0, header=self._view_msg[1])

    def process(self, msg, return_mask=False):
        """One callback: the centres of the scan rows; with return_mask also the mono8 ImageMsg of the mask.  With
        `fit` that result comes first of a pair, the frame's lanefit.LaneFits second.  With `diagnose` all of that
        comes first of a pair, the message's diagnose.FrameStats second."""
        result = self._process(msg, return_mask)
        if not self.diagnose:
            return result
        from .diagnose import FRAME_WORDS, FrameStats
        words = self._frame_records.cpu().numpy().view(np.uint64).reshape(1, FRAME_WORDS)
        self._frame_records = None
        return result, FrameStats(words, msg.height, msg.width)

    def _process(self, msg, return_mask):
        from .ros_bridge import ImageMsg
        mask = self.mask_on_device(msg)
        keep = None
        if self.clean is not None:
            from .instances import clean
            cleaned, self.last_components, keep = clean(mask, self.clean)
            mask = cleaned[0]
        centres = lane_centers(mask, self.scan_rows, self.level, self.min_pixels)[0]
        fits = self.tracker.update(mask) if self.tracker is not None else None
        if self.view is not None:
            self._draw_view(msg, mask, fits, keep)
        result = centres
        if return_mask:
            host = mask.cpu().numpy()
            result = centres, ImageMsg(height=host.shape[0], width=host.shape[1], encoding="mono8", data=host.tobytes(),
                                       step=host.shape[1], is_bigendian=0, header=msg.header)
        return result if self.tracker is None else (result, fits)
