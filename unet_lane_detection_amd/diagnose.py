"""Frame and output diagnostics on the device: what the reference tells a user to look at when "detection is poor".

  the input    `diagnose_input_image` (README.md:4476-4496): pixel range, mean brightness - it warns below 50 and above
               200 - and the variance of cv2.Laplacian(cvtColor(img, BGR2GRAY), CV_64F) as a sharpness figure, warned
               about below 100.  `frame_stats` reduces a batch of frames to 64 bytes each on the device
               (`unet_frame_stats_u8_batch`); `FrameStats` forms mean and variance from those exact integers.
  the output   `quick_test` (README.md:4615-4640): the output's range, its mean and the share of pixels above the
               threshold.  `output_stats` reduces probability planes to 32 bytes each (`unet_prob_stats_f32_batch`);
               `quick_test` here runs a model on a batch of frames and returns those figures with the mask.
  the data set `dataset_report`: how many frames of a device-resident data set are dark, overexposed or blurred.

`video.FramePipeline` and `follow.LaneFollowPipeline` take `diagnose=True` and then return the statistics of the
frames they were given, measured where the frames already are, beside their result.

The arithmetic is stated in include/unet_hip.h and, in numpy, in tests/diagnose_model.py.  The gray plane is OpenCV 4's
8-bit formula and the Laplacian its ksize = 1 kernel with the reflect-101 border; parity with cv2 itself is unpinned
(cv2 is not installed where this is tested and the reference ships no fixture).  No CPU fallback.
"""
from __future__ import annotations

import inspect

import numpy as np
import torch

from . import _lib

FRAME_WORDS, PROB_WORDS = 8, 4
DARK_LIMIT, BRIGHT_LIMIT, BLUR_LIMIT = 50.0, 200.0, 100.0     # the reference's


def _device_of(t, device):
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("the diagnostics need a HIP device; there is no CPU fallback")
    return device if isinstance(device, torch.device) else torch.device("cuda", int(device or 0))


def _words(records_dev, n, words):
    """the device's records (int64 storage) as (n, words) uint64 on the host"""
    return records_dev.cpu().numpy().view(np.uint64).reshape(n, words)


# ---- frames --------------------------------------------------------------------------------------------------------

class FrameStats:
    """The records of `unet_frame_stats_u8_batch` for n frames of height x width, on the host, and what the reference
    reads off a frame.  words: (n, 8) uint64.  The limits are the reference's and can be changed."""

    def __init__(self, words, height, width, dark_limit=DARK_LIMIT, bright_limit=BRIGHT_LIMIT, blur_limit=BLUR_LIMIT):
        self.words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, FRAME_WORDS)
        self.height, self.width = int(height), int(width)
        self.dark_limit, self.bright_limit, self.blur_limit = dark_limit, bright_limit, blur_limit

    def __len__(self):
        return int(self.words.shape[0])

    @property
    def min(self):
        return self.words[:, 0].astype(np.int64)

    @property
    def max(self):
        return self.words[:, 1].astype(np.int64)

    @property
    def mean(self):
        """img.mean(): sum / (3 h w), exact integers and one rounding"""
        size = 3 * self.height * self.width
        return np.array([int(w[2]) / size for w in self.words], dtype=np.float64)

    @property
    def sharpness(self):
        """Laplacian.var(): (N S2 - S1^2) / N^2, exact integers and one rounding"""
        n = self.height * self.width
        out = []
        for w in self.words:
            s1, s2 = int(w[3]), int(w[4])
            s1 = s1 - (1 << 64) if s1 >> 63 else s1
            out.append((n * s2 - s1 * s1) / (n * n))
        return np.array(out, dtype=np.float64)

    @property
    def too_dark(self):
        return self.mean < self.dark_limit

    @property
    def overexposed(self):
        return self.mean > self.bright_limit

    @property
    def blurry(self):
        return self.sharpness < self.blur_limit

    def report(self, i=0):
        """What the reference's `diagnose_input_image` prints for frame i, as a list of lines (same figures, formats
        and decisions; the wording is this project's)."""
        mean, sharp = float(self.mean[i]), float(self.sharpness[i])
        lines = [f"image size: ({self.height}, {self.width}, 3)", "data type: uint8",
                 f"pixel range: [{int(self.min[i])}, {int(self.max[i])}]", f"mean brightness: {mean:.1f}"]
        if mean < self.dark_limit:
            lines.append("warning: the image is too dark, detection may suffer")
        elif mean > self.bright_limit:
            lines.append("warning: the image is too bright / overexposed")
        else:
            lines.append("brightness is normal")
        lines.append(f"sharpness: {sharp:.1f}")
        if sharp < self.blur_limit:
            lines.append("warning: the image may be blurred")
        return lines


def frame_records(frames_dev, n, height, width, row_stride=0, bgr=True, out=None):
    """Enqueue `unet_frame_stats_u8_batch` on torch's current stream: frames_dev is a uint8 device tensor holding n
    frames of `height` rows of row_stride bytes (0: dense).  Returns the (n, 8) record tensor (int64 storage of the
    unsigned words), still on the device; nothing is read back."""
    if not isinstance(frames_dev, torch.Tensor) or not frames_dev.is_cuda or frames_dev.dtype != torch.uint8:
        raise TypeError("frames must be a uint8 torch tensor on the GPU")
    stride = int(row_stride) if row_stride else 3 * int(width)
    if frames_dev.numel() < (int(n) * int(height) - 1) * stride + 3 * int(width):
        raise ValueError("the frames tensor is shorter than n * height rows of row_stride bytes")
    if out is None:
        out = torch.empty((int(n), FRAME_WORDS), dtype=torch.int64, device=frames_dev.device)
    _lib.call("unet_frame_stats_u8_batch", frames_dev.device, frames_dev, int(n), int(height), int(width),
              int(row_stride or 0), 1 if bgr else 0, out)
    return out


def frame_stats(frames_u8, bgr=True, row_stride=None, width=None, device=None, **limits):
    """frames (n,h,w,3) or (h,w,3) uint8, numpy or torch, host or device -> FrameStats.  With row_stride the input is
    raw rows instead: (n,h,row_stride) or (h,row_stride) uint8 together with `width=`, the first 3 * width bytes of a
    row being pixels (a sensor_msgs/Image with its step).  `limits`: dark_limit, bright_limit, blur_limit of
    FrameStats.  64 bytes per frame are read back."""
    frames = torch.as_tensor(frames_u8)
    if frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8")
    if row_stride is None:
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("frames must be (n, h, w, 3) uint8")
        n, h, w = (int(v) for v in frames.shape[:3])
        stride = 0
    else:
        if width is None:
            raise ValueError("raw rows need width=")
        if frames.dim() == 2:
            frames = frames[None]
        if frames.dim() != 3 or int(frames.shape[2]) != int(row_stride):
            raise ValueError("raw rows must be (n, h, row_stride) uint8")
        n, h, w, stride = int(frames.shape[0]), int(frames.shape[1]), int(width), int(row_stride)
    dev = _device_of(frames, device)
    frames = frames.to(dev).contiguous()
    rec = frame_records(frames, n, h, w, stride, bgr)
    return FrameStats(_words(rec, n, FRAME_WORDS), h, w, **limits)


# ---- probability planes --------------------------------------------------------------------------------------------

class OutputStats:
    """The records of `unet_prob_stats_f32_batch` for n planes of `numel` probabilities, on the host.  words: (n, 4)
    uint64."""

    def __init__(self, words, numel, threshold):
        self.words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, PROB_WORDS)
        self.numel, self.threshold = int(numel), float(threshold)

    def __len__(self):
        return int(self.words.shape[0])

    @property
    def min(self):
        return (self.words[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)

    @property
    def max(self):
        return (self.words[:, 0] >> np.uint64(32)).astype(np.uint32).view(np.float32)

    @property
    def count_above(self):
        return self.words[:, 1].astype(np.int64)

    @property
    def share_above(self):
        return np.array([int(w[1]) / self.numel for w in self.words], dtype=np.float64)

    @property
    def mean(self):
        """the mean of clamp(p, 0, 1) to within 2^-32 (a NaN counts as 0)"""
        return np.array([int(w[2]) / ((1 << 32) * self.numel) for w in self.words], dtype=np.float64)

    @property
    def nan_count(self):
        return self.words[:, 3].astype(np.int64)

    def report(self, i=0):
        """What the reference's `quick_test` prints about plane i, as a list of lines."""
        return [f"output range: [{float(self.min[i]):.4f}, {float(self.max[i]):.4f}]", f"mean: {float(self.mean[i]):.4f}",
                f"share of pixels above the threshold: {float(self.share_above[i]) * 100:.1f}%"]


def prob_records(probs_dev, threshold=0.5, out=None):
    """Enqueue `unet_prob_stats_f32_batch` on torch's current stream: probs_dev (n, ...) float32 on the device ->
    the (n, 4) record tensor on the device."""
    if not isinstance(probs_dev, torch.Tensor) or not probs_dev.is_cuda or probs_dev.dtype != torch.float32:
        raise TypeError("probabilities must be a float32 torch tensor on the GPU")
    if probs_dev.dim() < 1 or probs_dev.numel() == 0:
        raise ValueError("probabilities must be (n, ...) and not empty")
    probs_dev = probs_dev.contiguous()
    n = int(probs_dev.shape[0])
    numel = probs_dev.numel() // n
    if out is None:
        out = torch.empty((n, PROB_WORDS), dtype=torch.int64, device=probs_dev.device)
    _lib.call("unet_prob_stats_f32_batch", probs_dev.device, probs_dev, n, numel, float(threshold), out)
    return out


def output_stats(probs, threshold=0.5, device=None):
    """probabilities (n, ...) float32, numpy or torch, host or device -> OutputStats; 32 bytes per plane are read back."""
    p = torch.as_tensor(probs)
    if p.dtype != torch.float32:
        raise ValueError("probabilities must be float32")
    p = p.to(_device_of(p, device))
    n = int(p.shape[0])
    return OutputStats(_words(prob_records(p, threshold), n, PROB_WORDS), p.numel() // n, threshold)


def quick_test(model, frames_u8, threshold=0.5, precision="f16x3"):
    """The reference's `quick_test` for a batch: frames (n,h,w,3) uint8 RGB through `model` - a `UNetHIP` (on the tier
    `precision`), a `UNetInt8` or an `ensemble.Ensemble` - and the statistics of its probabilities.  Returns
    (OutputStats, mask (n,h,w) uint8 on the device): the mask is the one the model writes at `threshold`."""
    frames = torch.as_tensor(frames_u8)
    if frames.dim() == 3:
        frames = frames[None]
    frames = frames.to(model.device)
    params = inspect.signature(model.run_u8).parameters
    kw = dict(return_mask=True, threshold=threshold)
    if "precision" in params:
        kw["precision"] = precision
    if "return_probs" in params:
        _, probs, mask = model.run_u8(frames, return_probs=True, **kw)
    else:                                   # an Ensemble: probabilities are what it returns
        probs, mask = model.run_u8(frames, **kw)
    return output_stats(probs, threshold), mask


# ---- a device-resident data set ------------------------------------------------------------------------------------

def dataset_report(dataset, batch=64, bgr=False, **limits):
    """Counts of dark, overexposed and blurred frames of an `augment.DeviceDataset` (its images are RGB: bgr=False),
    `batch` frames a launch; only the records are read back, once.  Returns a dict with the counts, the indices behind
    them and the FrameStats of the whole set."""
    images = dataset.images
    n, h, w = (int(v) for v in images.shape[:3])
    batch = int(batch)
    if batch <= 0 or n == 0:
        raise ValueError("batch must be positive and the data set non-empty")
    rec = torch.empty((n, FRAME_WORDS), dtype=torch.int64, device=images.device)
    for i in range(0, n, batch):
        k = min(batch, n - i)
        frame_records(images[i:i + k], k, h, w, 0, bgr, out=rec[i:i + k])
    stats = FrameStats(_words(rec, n, FRAME_WORDS), h, w, **limits)
    dark, bright, blurry = stats.too_dark, stats.overexposed, stats.blurry
    return {"frames": n, "too_dark": int(dark.sum()), "overexposed": int(bright.sum()), "blurry": int(blurry.sum()),
            "too_dark_idx": np.flatnonzero(dark).tolist(), "overexposed_idx": np.flatnonzero(bright).tolist(),
            "blurry_idx": np.flatnonzero(blurry).tolist(), "stats": stats}
