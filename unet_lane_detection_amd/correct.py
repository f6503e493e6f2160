"""Frame correction on the device: white balance, percentile stretch, a tone table and CLAHE, per frame.

The reference exists because of one failure: the white marking stops looking white when the camera's white balance
drifts, a shadow falls on it or glare washes it out (README.md:325-342: the HSV triple leaves [0..180, 0..40, 185..255]
under a cast; :380-429: the three failure cases).  `diagnose.frame_stats` can say that a frame is dark or burnt out;
`FrameCorrector` does something about it, where the frame already lies: the channel histograms of the frame decide a
gray-world gain per channel, a stretch between two percentiles and - through a caller-made table - a tone curve, a
CLAHE on the luminance (hue kept) follows, and one pass applies all of it (`unet_correct_u8_batch`).  Nothing but the
32-byte plan ever needs to leave the device, and only when `plan()` is asked for it.

`video.FramePipeline(correct=CorrectConfig(...))` corrects a chunk before the resize,
`follow.LaneFollowPipeline(correct=CorrectConfig(...))` the message's rows before the warp.

The arithmetic is stated in include/unet_hip.h and, in numpy, in tests/correct_model.py.  The reference has no such
code and cv2 is not installed where this is tested: parity with cv2.createCLAHE or any other implementation is
unpinned.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

PLAN_WORDS = 8
FLAG_CORRECTED, FLAG_STRETCH, FLAG_CLAHE = 1, 2, 4


def gamma_table(gamma):
    """uint8[256]: rint(255 (v / 255)^gamma), made once on the host - no pow runs on the device.  gamma < 1 brightens."""
    gamma = float(gamma)
    if not gamma > 0.0 or not np.isfinite(gamma):
        raise ValueError("gamma must be positive and finite")
    v = np.arange(256, dtype=np.float64) / 255.0
    return np.clip(np.rint(255.0 * v ** gamma), 0, 255).astype(np.uint8)


@dataclass
class Clahe:
    """clip_limit as cv2.createCLAHE's (a multiple of the mean bin count), grid = (tiles across, tiles down)"""
    clip_limit: float = 2.0
    grid: Tuple[int, int] = (8, 8)


@dataclass
class CorrectConfig:
    """What to correct.  white_balance: "gray_world" or None.  stretch: (lo_pct, hi_pct), the percentages of the
    samples clipped below and above, or None.  gamma: a float (see gamma_table) or None; tone: a uint8[256] table
    instead of it.  clahe: a Clahe or None.  max_gain: 1..8, the most (and 1 / the least) a channel is scaled by.
    only_flagged: correct only the frames whose mean brightness is below dark_limit or above bright_limit - the
    frames `diagnose.FrameStats` calls too_dark or overexposed; the others pass through byte for byte."""
    white_balance: Optional[str] = "gray_world"
    stretch: Optional[Tuple[float, float]] = None
    gamma: Optional[float] = None
    tone: Optional[np.ndarray] = None
    clahe: Optional[Clahe] = None
    max_gain: int = 4
    only_flagged: bool = False
    dark_limit: int = 50
    bright_limit: int = 200

    def grid(self):
        """(grid_x, grid_y) of the work buffer: the CLAHE grid, (1, 1) without CLAHE"""
        return (1, 1) if self.clahe is None else (int(self.clahe.grid[0]), int(self.clahe.grid[1]))

    def struct(self):
        """the unet_correct_config of this configuration"""
        if self.white_balance not in (None, "gray_world"):
            raise ValueError(f"white_balance={self.white_balance!r}: \"gray_world\" or None")
        if self.gamma is not None and self.tone is not None:
            raise ValueError("gamma and tone are two ways to give one table; give one of them")
        s = _lib.CorrectConfigStruct()
        s.white_balance = 1 if self.white_balance else 0
        s.max_gain = int(self.max_gain)
        if self.stretch is not None:
            lo, hi = (int(round(float(p) * 100.0)) for p in self.stretch)
            if lo == 0 and hi == 0:
                raise ValueError("stretch=(0, 0) clips nothing; pass None")
            s.lo_bp, s.hi_bp = lo, hi
        s.clahe = 0 if self.clahe is None else 1
        s.grid_x, s.grid_y = self.grid()
        s.clip_q8 = 512 if self.clahe is None else int(round(float(self.clahe.clip_limit) * 256.0))
        s.only_flagged = 1 if self.only_flagged else 0
        s.dark_limit, s.bright_limit = int(self.dark_limit), int(self.bright_limit)
        if self.tone is not None:
            tone = np.ascontiguousarray(self.tone)
            if tone.dtype != np.uint8 or tone.size != 256:
                raise ValueError("tone must be uint8[256]")
            tone = tone.reshape(256)
        else:
            tone = np.arange(256, dtype=np.uint8) if self.gamma is None else gamma_table(self.gamma)
        C.memmove(s.tone, tone.ctypes.data, 256)
        return s


@dataclass
class Plan:
    """The plan words of n frames on the host.  gains: (n, 3) float, per channel in memory order; lo, hi: (n,) int;
    corrected: (n,) bool; mean: (n,) float, the mean of the uncorrected frame; words: (n, 8) uint32 as the device
    wrote them."""
    words: np.ndarray
    gains: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    corrected: np.ndarray
    mean: np.ndarray


class FrameCorrector:
    """`config` applied to device frames on torch's current stream.  Owns and reuses its work buffer, so one corrector
    serves one stream at a time."""

    def __init__(self, config=None, device=0):
        if not torch.cuda.is_available():
            raise RuntimeError("the frame correction needs a HIP device; there is no CPU fallback")
        self.config = CorrectConfig() if config is None else config
        self._lib = _lib.load()
        if self._lib.unet_correct_config_bytes() != C.sizeof(_lib.CorrectConfigStruct):
            raise RuntimeError("unet_correct_config of the library and of the binding differ")
        self._cfg = self.config.struct()
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        self._work = None
        self.last_plan = None      # (n, 8) int32 storage of the unsigned plan words, on the device
        self._shape = None

    def work_bytes(self, n):
        return int(self._lib.unet_correct_work_bytes(int(n), self._cfg.grid_x, self._cfg.grid_y))

    def correct(self, frames_u8, bgr=True, row_stride=0, out=None, width=None):
        """frames: a uint8 device tensor, (n,h,w,3) or (h,w,3); with row_stride raw rows instead, (n,h,row_stride) or
        (h,row_stride) together with `width=` (a sensor_msgs/Image with its step).  Returns the corrected frames on
        the device, in the input's shape and stride: a new tensor, or `out` (which may be the input itself).  Only
        enqueues on torch's current stream."""
        if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8:
            raise TypeError("frames must be a uint8 torch tensor on the GPU")
        frames = frames_u8
        if row_stride:
            if width is None:
                raise ValueError("raw rows need width=")
            if frames.dim() == 2:
                frames = frames[None]
            if frames.dim() != 3 or int(frames.shape[2]) != int(row_stride):
                raise ValueError("raw rows must be (n, h, row_stride) uint8")
            n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(width)
        else:
            if frames.dim() == 3:
                frames = frames[None]
            if frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError("frames must be (n, h, w, 3) uint8")
            n, h, w = (int(v) for v in frames.shape[:3])
        if not frames.is_contiguous():
            raise ValueError("frames must be contiguous")
        if out is None:
            out = torch.empty_like(frames_u8)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != frames.device \
                or out.numel() != frames_u8.numel() or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 tensor of the input's size on the input's device")
        need = self.work_bytes(n)
        if self._work is None or self._work.numel() < need or self._work.device != frames.device:
            if self._work is not None:   # the last call may still be running on this stream
                self._work.record_stream(torch.cuda.current_stream(self._work.device))
            self._work = torch.empty(need, dtype=torch.uint8, device=frames.device)
        _lib.call("unet_correct_u8_batch", frames.device, frames, n, h, w, int(row_stride or 0), 1 if bgr else 0,
                  C.byref(self._cfg), out, int(row_stride or 0), self._work, self._work.numel())
        per = need // n
        self.last_plan = self._work[:need].view(n, per)[:, 3072:3072 + 4 * PLAN_WORDS].contiguous().view(torch.int32)
        self._shape = (h, w)
        return out

    def plan(self):
        """The last call's plan on the host (32 bytes per frame are read back); None before the first call."""
        if self.last_plan is None:
            return None
        words = self.last_plan.cpu().numpy().view(np.uint32).reshape(-1, PLAN_WORDS)
        h, w = self._shape
        total = words[:, 6].astype(np.uint64) | (words[:, 7].astype(np.uint64) << np.uint64(32))
        return Plan(words=words, gains=words[:, 1:4].astype(np.float64) / 65536.0, lo=words[:, 4].astype(np.int64),
                    hi=words[:, 5].astype(np.int64), corrected=(words[:, 0] & FLAG_CORRECTED) != 0,
                    mean=np.array([int(t) / (3 * h * w) for t in total], dtype=np.float64))
