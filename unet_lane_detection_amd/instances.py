"""Lane instances on the device: which pixels of a mask belong together.

The reference lists "multi-lane detection", "confidence output" and "instance segmentation" on its roadmap
(README.md:5138-5153) and names "lots of noise pixels" as a failure it can only answer by retraining or a higher
threshold (README.md:4465, 4601); it has no code for either.  This is the classic answer - connected components with
statistics, small ones dropped, each remaining one a marking - made where the mask already is:

  the labels    `unet_label_u8_batch`: 4- or 8-connected components of a mask batch, ids in raster order of a
                component's first pixel (scipy.ndimage.label's numbering), and per component sixteen integer words:
                area, bounding box, the moment sums S_k = sum y^k and T_k = sum x y^k, first pixel, border flags.
                `label` enqueues it and brings 128 bytes per recorded component and 32 per frame to the host.
  the filter    `unet_keep_components_u8_batch`: min_area, min_height, min_width, keep_largest -> a keep table and a
                cleaned 0 / 255 mask, still on the device, for the scan-row centre and the lane fit.  `clean`.
  the result    `Components`: count, areas, boxes, centroids, border flags per frame, and `.fit(i, c)`: the curve
                x = a y^2 + b y + c of a component from its sums, by `lanefit.solve`.  `lane_instances`: the kept
                components of every frame as `LaneInstance`s, left to right - any number of markings, not two.
  the pipeline  `follow.LaneFollowPipeline(clean=CleanConfig(...))`.

The arithmetic is stated in include/unet_hip.h and, in numpy, in tests/label_model.py.  Parity with cv2's label
numbering is unpinned.  No CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .lanefit import FIT_WORDS, FitConfig, LaneFit

LABEL_WORDS = 16          # UNET_LABEL_WORDS
COMPONENTS_MAX = 65536


@dataclass(frozen=True)
class CleanConfig:
    """min_area, min_height, min_width, keep_largest: the filter (include/unet_hip.h; 0 switches a rule off).  level,
    connectivity, max_components: the labelling in front of it."""
    min_area: int = 64
    min_height: int = 0
    min_width: int = 0
    keep_largest: int = 0
    level: int = 127
    connectivity: int = 8
    max_components: int = 1024


class Components:
    """The header and records of `unet_label_u8_batch` for n frames on the host, `.labels` still on the device (None
    when built from host arrays alone).  Per-frame lists; a frame's arrays cover its recorded components, component c
    at index c - 1."""

    def __init__(self, labels, header, records, height, width):
        self.labels = labels
        self.header = np.ascontiguousarray(np.asarray(header)).view(np.uint64).reshape(-1, 4)
        n = self.header.shape[0]
        self.records = np.ascontiguousarray(np.asarray(records)).view(np.uint64).reshape(n, -1, LABEL_WORDS)
        self.height, self.width = int(height), int(width)

    def __len__(self):
        return self.header.shape[0]

    def recorded(self, i):
        """the number of components of frame i that have a record: min(K, max_components)"""
        return int(self.header[i, 2])

    def _rec(self, i):
        return self.records[i, :self.recorded(i)]

    @property
    def count(self):
        """K per frame: the true count, also where it exceeds max_components"""
        return [int(v) for v in self.header[:, 0]]

    @property
    def on_pixels(self):
        return [int(v) for v in self.header[:, 1]]

    @property
    def truncated(self):
        """K > max_components: the map is complete, the records of the last components are missing"""
        return [int(h[0]) > int(h[2]) for h in self.header]

    @property
    def area(self):
        return [self._rec(i)[:, 0].astype(np.int64) for i in range(len(self))]

    @property
    def bbox(self):
        """per frame (m, 4) int64: x_min, x_max, y_min, y_max (inclusive)"""
        return [self._rec(i)[:, 1:5].astype(np.int64) for i in range(len(self))]

    @property
    def centroid(self):
        """per frame a list of (sum x / area, sum y / area): each from the exact integers with one rounding"""
        return [[(int(r[5]) / int(r[0]), int(r[6]) / int(r[0])) for r in self._rec(i)] for i in range(len(self))]

    @property
    def touches(self):
        """per frame (m,) int64 border flags: bit 0 row 0, bit 1 row height - 1, bit 2 column 0, bit 3 column width - 1"""
        return [self._rec(i)[:, 13].astype(np.int64) for i in range(len(self))]

    @property
    def first_pixel(self):
        """per frame (m, 2) int64: (y, x) of the component's first pixel in raster order"""
        return [np.stack([self._rec(i)[:, 12].astype(np.int64) // self.width,
                          self._rec(i)[:, 12].astype(np.int64) % self.width], axis=1) for i in range(len(self))]

    def fit(self, i, c, cfg=FitConfig()):
        """component c (1-based) of frame i as a lanefit.LaneFit: x = a y^2 + b y + c by `lanefit.solve` from the
        record's S and T words, no coefficients below cfg.min_fit_pixels pixels.  The words a window search would
        fill (base, hit, tried, last centre) are 0, so the LaneFit's own `confidence` is 0.0; LaneInstance carries
        the instance's."""
        if not 1 <= c <= self.recorded(i):
            raise IndexError(f"frame {i} has records for components 1 .. {self.recorded(i)}, not {c}")
        r = [int(v) for v in self.records[i, c - 1]]
        words = [1, 0, 0, 0, 0, r[0], r[6], r[7], r[8], r[9], r[5], r[10], r[11], r[3], r[4], 0]
        assert len(words) == FIT_WORDS
        return LaneFit(np.array(words, dtype=np.uint64), self.height, cfg)


@dataclass
class LaneInstance:
    """One kept component of one frame.  confidence = area / (area of the frame's largest kept component), so the
    largest marking has 1.0.  bbox: x_min, x_max, y_min, y_max."""
    frame: int
    id: int
    fit: LaneFit
    area: int
    bbox: tuple
    confidence: float
    centroid: tuple

    def x_at(self, y):
        return self.fit.x_at(y)


_WORK = {}        # (device index, stream, n, h, w) -> the workspace of unet_label_u8_batch, kept for the next such call
_WORK_SLOTS = 16  # the oldest entry goes when there are more


def _workspace(device, n, h, w):
    """The call's scratch is only valid on the stream it is enqueued on, so the current stream is part of the key:
    calls of one shape on two streams get two buffers.  The buffer is allocated on that stream, so dropping the
    oldest entry is safe in stream order (torch's allocator reuses it behind the work already enqueued there)."""
    key = (device.index, int(torch.cuda.current_stream(device).cuda_stream), n, h, w)
    buf = _WORK.get(key)
    if buf is None:
        size = int(_lib.load().unet_label_work_bytes(n, h, w))
        if size == 0:
            raise ValueError(f"({n}, {h}, {w}) is outside the domain of unet_label_u8_batch")
        while len(_WORK) >= _WORK_SLOTS:
            del _WORK[next(iter(_WORK))]
        buf = _WORK[key] = torch.empty((size,), dtype=torch.uint8, device=device)
    return buf


def _masks(masks_dev):
    if not isinstance(masks_dev, torch.Tensor) or not masks_dev.is_cuda or masks_dev.dtype != torch.uint8:
        raise TypeError("masks must be a uint8 torch tensor on the GPU")
    if masks_dev.dim() == 2:
        masks_dev = masks_dev[None]
    if masks_dev.dim() != 3:
        raise ValueError("masks must be (n, h, w)")
    return masks_dev.contiguous()


def label_records(masks_dev, level=127, connectivity=8, max_components=1024):
    """-> (labels (n,h,w) int32, header (n,4) int64, records (n,cap,16) int64), all on the device (int64 storage of
    the unsigned words); nothing is read back."""
    masks_dev = _masks(masks_dev)
    n, h, w = (int(v) for v in masks_dev.shape)
    cap = int(max_components)
    if not 1 <= cap <= COMPONENTS_MAX:
        raise ValueError("max_components must lie in 1 .. 65536")
    dev = masks_dev.device
    work = _workspace(dev, n, h, w)
    labels = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    header = torch.empty((n, 4), dtype=torch.int64, device=dev)
    records = torch.empty((n, cap, LABEL_WORDS), dtype=torch.int64, device=dev)
    _lib.call("unet_label_u8_batch", dev, masks_dev, n, h, w, int(level), int(connectivity), labels, cap, header, records,
              work, work.numel())
    return labels, header, records


def _to_components(labels, header, records, h, w):
    head = header.cpu().numpy().view(np.uint64)
    m = int(head[:, 2].max()) if head.size else 0
    rec = records[:, :m].cpu().numpy().view(np.uint64) if m else np.zeros((head.shape[0], 0, LABEL_WORDS), np.uint64)
    return Components(labels, head, rec, h, w)


def label(masks_dev, level=127, connectivity=8, max_components=1024):
    """masks (n,h,w) or (h,w) uint8 on the device -> Components; 32 bytes per frame and 128 per recorded component of
    the fullest frame are read back."""
    labels, header, records = label_records(masks_dev, level, connectivity, max_components)
    return _to_components(labels, header, records, int(labels.shape[1]), int(labels.shape[2]))


def clean(masks_dev, cfg=CleanConfig()):
    """-> (mask (n,h,w) uint8 on the device: 255 where the pixel's component is kept, else 0; Components; keep
    (n, max_components) uint8 on the device).  The input is left as it is."""
    masks_dev = _masks(masks_dev)
    labels, header, records = label_records(masks_dev, cfg.level, cfg.connectivity, cfg.max_components)
    n, h, w = (int(v) for v in labels.shape)
    cap = int(cfg.max_components)
    dev = labels.device
    keep = torch.empty((n, cap), dtype=torch.uint8, device=dev)
    out = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    _lib.call("unet_keep_components_u8_batch", dev, labels, n, h, w, header, records, cap, int(cfg.min_area),
              int(cfg.min_height), int(cfg.min_width), int(cfg.keep_largest), keep, out)
    return out, _to_components(labels, header, records, h, w), keep


def instances_of(components, keep, y_ref=None, fit_cfg=FitConfig()):
    """Components and the keep table (n, >= recorded) on the host -> per frame the list of LaneInstance of the kept
    components, sorted left to right by x_at(y_ref) (default: the bottom row, height - 1); an instance without
    coefficients sorts by its centroid's x."""
    y_ref = components.height - 1 if y_ref is None else y_ref
    keep = np.asarray(keep)
    out = []
    for i in range(len(components)):
        ids = [c for c in range(1, components.recorded(i) + 1) if keep[i, c - 1]]
        areas = components.area[i]
        boxes, cents = components.bbox[i], components.centroid[i]
        largest = max((int(areas[c - 1]) for c in ids), default=0)
        frame = []
        for c in ids:
            area = int(areas[c - 1])
            frame.append(LaneInstance(i, c, components.fit(i, c, fit_cfg), area, tuple(int(v) for v in boxes[c - 1]),
                                      area / largest, cents[c - 1]))
        frame.sort(key=lambda s: (s.fit.x_at(y_ref) if s.fit.coeffs is not None else s.centroid[0], s.id))
        out.append(frame)
    return out


def lane_instances(masks_dev, cfg=CleanConfig(), y_ref=None, fit_cfg=FitConfig()):
    """masks on the device -> per frame the list of LaneInstance (see instances_of): the roadmap's multi-lane output"""
    _, components, keep = clean(masks_dev, cfg)
    m = max((components.recorded(i) for i in range(len(components))), default=0)
    return instances_of(components, keep[:, :m].cpu().numpy(), y_ref, fit_cfg)
