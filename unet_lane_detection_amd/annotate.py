"""Annotations to training masks: the reference's `labelme_to_mask.py` (README.md:1013-1052), `LaneDataset` with
`A.Resize(image_size, image_size)` (:1996-2055) and the data side of its progressive training (tip 4, :2562-2589).

  LabelMe JSON --load_labelme--> polygons --PolygonBatch--> CSR arrays --.to(device)--> rasterize --> masks (n, h, w)
  TrainingSource(frames, batch).at(size) --> augment.DeviceDataset at that size --> loop.fit_progressive

Frames and polygons stay on the device; the masks are rasterised there (csrc/annotate_kernels.cpp,
`unet_fill_polygons_u8_batch`) at whatever size a stage trains at, and the frames go through `unet_resize_u8_batch`.
A polygon carries one byte, so several labels give a label plane ("lane + drivable area"); the network stays
single-class.

The rule is integer arithmetic, stated in include/unet_hip.h and, as the specification, in tests/annotate_model.py:
even-odd parity at the pixel centre or an 8-connected outline, painter's order, output pixel (X, Y) asking about the
source point ((X * src_w) // out_w, (Y * src_h) // out_h).  numpy batches run through `fill_host`, the same rule on the
host; the kernel and `fill_host` are both tested against the specification with tolerance zero.  Parity with
cv2.fillPoly itself is UNPINNED: cv2 is not installed where this is built and tested and the reference has no fixture;
along boundaries cv2's fixed-point edge walk and its line iterator set other pixels.

Not here: cv2.polylines of the ROI check (README.md:4557), putText, LabelMe shape types other than polygons (every
matching shape is treated as one), PNG / JPEG input and output (writing the masks is the caller's business).
"""
from __future__ import annotations

import json
import os

import numpy as np

COORD_LIMIT = 1 << 20     # |x|, |y| of a vertex: every expression of the rule then fits in 63 bits
MAX_SIDE = 16384          # source and output sizes
_INT32_MAX = (1 << 31) - 1


# ---------------------------------------------------------------------------------------------------------------
# LabelMe
# ---------------------------------------------------------------------------------------------------------------
def load_labelme(path_or_dict, label="lane", values=None):
    """-> (polygons, (imageHeight, imageWidth)); polygons is a list of (points int32 (k, 2), value) in file order.
    The reference's rule: only shapes whose label matches, points through np.array(points, dtype=np.int32), which
    truncates towards zero.  values, a dict from label to byte, selects several labels; the default is {label: 255}."""
    if isinstance(path_or_dict, dict):
        data = path_or_dict
    else:
        with open(path_or_dict, "r") as f:
            data = json.load(f)
    values = {label: 255} if values is None else dict(values)
    for k, v in values.items():
        if not (isinstance(v, (int, np.integer)) and 0 <= int(v) <= 255):
            raise ValueError("the value of label %r must be a byte" % (k,))
    polygons = []
    for shape in data["shapes"]:
        if shape["label"] in values:
            points = np.array(shape["points"], dtype=np.int32).reshape(-1, 2)
            polygons.append((points, int(values[shape["label"]])))
    return polygons, (int(data["imageHeight"]), int(data["imageWidth"]))


# ---------------------------------------------------------------------------------------------------------------
# CSR tables
# ---------------------------------------------------------------------------------------------------------------
def _offsets(name, a, total, what):
    a = np.asarray(a)
    if a.ndim != 1 or a.size < 1 or a.dtype.kind not in "iu":
        raise ValueError("%s must be a 1-d integer array with at least one entry" % name)
    a = a.astype(np.int64)
    if a[0] != 0 or (np.diff(a) < 0).any():
        raise ValueError("%s must start at 0 and never decrease" % name)
    if a[-1] != total:
        raise ValueError("%s must end at the number of %s (%d)" % (name, what, total))
    if total > _INT32_MAX:
        raise ValueError("%s does not fit in int32" % name)
    return a.astype(np.int32)


def _check_sizes(src_size, out_size):
    sizes = tuple(src_size) + tuple(out_size)
    if len(sizes) != 4 or any(not 1 <= int(v) <= MAX_SIDE for v in sizes):
        raise ValueError("src_size and out_size are (height, width) pairs of 1 .. %d" % MAX_SIDE)
    return tuple(int(v) for v in sizes)


class PolygonBatch:
    """The polygons of n frames as CSR arrays: vertices (V, 2) int32, poly_offsets (P + 1) into the vertices,
    poly_values (P) uint8, frame_offsets (n + 1) into the polygons.  frames_of_polygons: one list per frame of
    (points, value) pairs in painter's order; points is an integer array-like of (x, y) rows (no rows: the polygon is
    skipped; one: a dot; two: a line).  Limits and offsets are checked here, ahead of any launch: ValueError.
    `.to(device)` returns the batch with its tables on the device; `rasterize` then runs the kernel."""

    def __init__(self, frames_of_polygons):
        verts, poffs, vals, foffs = [], [0], [], [0]
        for polygons in frames_of_polygons:
            for polygon in polygons:
                if not isinstance(polygon, (tuple, list)) or len(polygon) != 2 or np.ndim(polygon[1]) != 0:
                    raise ValueError("a polygon is a (points, value) pair")
                points, value = polygon
                pts = np.asarray(points)
                if pts.size and pts.dtype.kind not in "iu":
                    raise ValueError("vertices must be integers (load_labelme truncates as the reference does)")
                if pts.size % 2 or (pts.ndim != 2 and pts.size) or (pts.ndim == 2 and pts.shape[1] != 2 and pts.size):
                    raise ValueError("points must be rows of (x, y)")
                verts.append(pts.reshape(-1, 2).astype(np.int64))
                poffs.append(poffs[-1] + verts[-1].shape[0])
                vals.append(value)
            foffs.append(len(vals))
        vertices = np.concatenate(verts) if verts else np.zeros((0, 2), dtype=np.int64)
        self._set(vertices, np.asarray(poffs, dtype=np.int64), np.asarray(vals, dtype=np.int64),
                  np.asarray(foffs, dtype=np.int64))

    @classmethod
    def from_arrays(cls, vertices, poly_offsets, poly_values, frame_offsets):
        """The batch from tables built elsewhere; the same checks."""
        self = cls.__new__(cls)
        self._set(np.asarray(vertices), np.asarray(poly_offsets), np.asarray(poly_values), np.asarray(frame_offsets))
        return self

    def _set(self, vertices, poly_offsets, poly_values, frame_offsets):
        if vertices.ndim != 2 or vertices.shape[1] != 2 or (vertices.size and vertices.dtype.kind not in "iu"):
            raise ValueError("vertices must be an integer array of shape (V, 2)")
        if vertices.size and np.abs(vertices.astype(np.int64)).max() > COORD_LIMIT:
            raise ValueError("coordinates must lie within +-2^20")
        if poly_values.ndim != 1 or (poly_values.size and poly_values.dtype.kind not in "iu"):
            raise ValueError("poly_values must be a 1-d integer array")
        if poly_values.size and (poly_values.min() < 0 or poly_values.max() > 255):
            raise ValueError("a polygon's value must be a byte")
        self.poly_offsets = _offsets("poly_offsets", poly_offsets, vertices.shape[0], "vertices")
        if self.poly_offsets.size != poly_values.size + 1:
            raise ValueError("poly_offsets must hold one entry more than poly_values")
        self.frame_offsets = _offsets("frame_offsets", frame_offsets, poly_values.size, "polygons")
        if self.frame_offsets.size < 2:
            raise ValueError("a batch holds at least one frame")
        self.vertices = np.ascontiguousarray(vertices.astype(np.int32)).reshape(-1, 2)
        self.poly_values = np.ascontiguousarray(poly_values.astype(np.uint8))
        self.device, self._dev = None, None

    @property
    def n(self):
        return int(self.frame_offsets.size - 1)

    def __len__(self):
        return self.n

    def frames(self):
        """back to lists: one list of (points, value) per frame"""
        out = []
        for i in range(self.n):
            out.append([(self.vertices[self.poly_offsets[j]:self.poly_offsets[j + 1]].copy(), int(self.poly_values[j]))
                        for j in range(self.frame_offsets[i], self.frame_offsets[i + 1])])
        return out

    def to(self, device):
        """The same tables with a copy on the device (an ordinal or a torch.device)."""
        import torch
        if isinstance(device, (str, torch.device)):
            dev = torch.device(device)
            dev = torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev
        else:
            dev = torch.device("cuda", int(device))
        if dev.type != "cuda":
            raise ValueError("the tables move to a GPU; a batch that was not moved runs on the host")
        other = PolygonBatch.__new__(PolygonBatch)
        other.vertices, other.poly_offsets = self.vertices, self.poly_offsets
        other.poly_values, other.frame_offsets = self.poly_values, self.frame_offsets
        # an empty table still gets one element, so that its pointer is one the library accepts
        pad = lambda a, shape: a if a.size else np.zeros(shape, dtype=a.dtype)   # noqa: E731
        other.device = dev
        other._dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (
            pad(self.vertices, (1, 2)), self.poly_offsets, pad(self.poly_values, (1,)), self.frame_offsets))
        return other


# ---------------------------------------------------------------------------------------------------------------
# the rule on the host (numpy batches); tests/annotate_model.py is its specification
# ---------------------------------------------------------------------------------------------------------------
def _fill_frame(mask, polygons, sy, sx):
    """mask (h, w) uint8 zeros; sy (h,), sx (w,) int64, both non-decreasing"""
    cols = sx[None, :]
    for pts, value in polygons:
        k = len(pts)
        if k == 0:
            continue
        odd = np.zeros(mask.shape, dtype=bool)
        line = np.zeros(mask.shape, dtype=bool)
        p = pts.astype(np.int64)
        for i in range(k):
            (xa, ya), (xb, yb) = p[i].tolist(), p[(i + 1) % k].tolist()
            if ya > yb or (ya == yb and xa > xb):       # upwards; a horizontal edge left to right
                xa, ya, xb, yb = xb, yb, xa, ya
            r0, r1 = np.searchsorted(sy, ya, "left"), np.searchsorted(sy, yb, "right")
            if r0 == r1:
                continue
            rows = sy[r0:r1, None]
            dxp, dyp = xb - xa, yb - ya
            m = dyp * (cols - xa)
            odd[r0:r1] ^= (rows < yb) & (dxp * (rows - ya) - m > 0)
            if abs(dxp) >= dyp:
                if dxp == 0:
                    t, lim = np.zeros_like(m), 1
                elif dxp > 0:
                    t, lim = 2 * m + dxp - 2 * dxp * (rows - ya), 2 * dxp
                else:
                    t, lim = -2 * m + 2 * dyp * dxp - dxp + 2 * dxp * (rows - yb), -2 * dxp
            else:
                t, lim = 2 * (rows - ya) * dxp + dyp - 2 * m, 2 * dyp
            line[r0:r1] |= (cols >= min(xa, xb)) & (cols <= max(xa, xb)) & (t >= 0) & (t < lim)
        mask[odd | line] = value


def fill_host(batch, src_size, out_size=None):
    """(n, out_h, out_w) uint8 from a batch's host tables"""
    src_h, src_w, out_h, out_w = _check_sizes(src_size, src_size if out_size is None else out_size)
    sy = (np.arange(out_h, dtype=np.int64) * src_h) // out_h
    sx = (np.arange(out_w, dtype=np.int64) * src_w) // out_w
    masks = np.zeros((batch.n, out_h, out_w), dtype=np.uint8)
    for i, polygons in enumerate(batch.frames()):
        _fill_frame(masks[i], polygons, sy, sx)
    return masks


# ---------------------------------------------------------------------------------------------------------------
# the kernel behind torch tensors
# ---------------------------------------------------------------------------------------------------------------
def _fill_device(batch, src_size, out_size, out):
    import torch

    from . import _lib
    src_h, src_w, out_h, out_w = _check_sizes(src_size, src_size if out_size is None else out_size)
    dev, n = batch.device, batch.n
    if out is None:
        out = torch.empty((n, out_h, out_w), dtype=torch.uint8, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.shape != (n, out_h, out_w) or out.dtype != torch.uint8
          or not out.is_contiguous() or out.device != dev):
        raise ValueError("out must be a contiguous (n, out_h, out_w) uint8 tensor on the batch's device")
    vertices, poly_offsets, poly_values, frame_offsets = batch._dev
    _lib.call("unet_fill_polygons_u8_batch", dev, vertices, poly_offsets, poly_values, frame_offsets, n, src_h, src_w, out_h,
              out_w, out)
    return out


def rasterize(batch, src_size, out_size=None, out=None):
    """-> masks (n, out_h, out_w) uint8.  src_size = (height, width) the polygons were drawn in, out_size the size of
    the masks (None: the source size).  A batch moved with `.to(device)` goes through the kernel and gives a tensor on
    that device (out: a tensor to write into); any other batch runs `fill_host` and gives a numpy array."""
    if not isinstance(batch, PolygonBatch):
        raise TypeError("batch must be a PolygonBatch")
    if batch.device is not None:
        return _fill_device(batch, src_size, out_size, out)
    if out is not None:
        raise ValueError("out= is for batches on the device")
    return fill_host(batch, src_size, out_size)


def labelme_to_masks(json_paths, label="lane", values=None, out_size=None, device=None):
    """The reference's batch loop: one mask per LabelMe file, (n, h, w) uint8 - a numpy array, or with `device` a
    tensor rasterised there.  Without out_size every file must declare the same image size, which the masks then
    have; with it every mask is rasterised at out_size from its own image size.  Writing PNGs is the caller's
    business."""
    loaded = [load_labelme(p, label=label, values=values) for p in json_paths]
    if not loaded:
        raise ValueError("no annotation files")
    sizes = [size for _, size in loaded]
    if out_size is None:
        if any(s != sizes[0] for s in sizes):
            raise ValueError("the files declare different image sizes; give out_size")
        out_size = sizes[0]
    result = None
    for size in sorted(set(sizes)):      # one call per source size
        idx = [i for i, s in enumerate(sizes) if s == size]
        batch = PolygonBatch([loaded[i][0] for i in idx])
        masks = rasterize(batch if device is None else batch.to(device), size, out_size)
        if result is None:
            result = masks.new_zeros((len(loaded),) + tuple(masks.shape[1:])) if device is not None else \
                np.zeros((len(loaded),) + masks.shape[1:], dtype=np.uint8)
        result[idx] = masks
    return result


def labelme_files(directory):
    """the .json files of a directory, sorted: the reference walks os.listdir"""
    return [os.path.join(directory, f) for f in sorted(os.listdir(directory)) if f.endswith(".json")]


# ---------------------------------------------------------------------------------------------------------------
# frames and polygons on the device, a data set at any size
# ---------------------------------------------------------------------------------------------------------------
class TrainingSource:
    """Source frames (n, H, W, 3) uint8 and their polygons, both resident on the device.  `.at(size)` gives the
    augment.DeviceDataset of one training stage: the frames through `unet_resize_u8_batch` (with swap_rb when the
    frames are BGR, as cv2.imread delivers them), the masks rasterised at (size, size) from the polygons - not resized
    from a stored mask.  size: an int, a (height, width) pair, or None for the source size."""

    def __init__(self, frames_u8, batch, bgr=False, device=0):
        import torch
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        self.frames = torch.as_tensor(frames_u8).to(self.device).contiguous()
        if self.frames.dtype != torch.uint8 or self.frames.dim() != 4 or self.frames.shape[3] != 3:
            raise ValueError("frames must be (n, H, W, 3) uint8")
        if not isinstance(batch, PolygonBatch) or batch.n != self.frames.shape[0]:
            raise ValueError("batch must be a PolygonBatch with one polygon list per frame")
        self.batch = batch if batch.device == self.device else batch.to(self.device)
        self.bgr = bool(bgr)

    def __len__(self):
        return int(self.frames.shape[0])

    def at(self, size=None):
        import torch

        from . import _lib
        from .augment import DeviceDataset
        n, h, w = (int(v) for v in self.frames.shape[:3])
        out_h, out_w = (h, w) if size is None else ((int(size), int(size)) if np.ndim(size) == 0 else
                                                    (int(size[0]), int(size[1])))
        _check_sizes((h, w), (out_h, out_w))
        images = torch.empty((n, out_h, out_w, 3), dtype=torch.uint8, device=self.device)
        _lib.call("unet_resize_u8_batch", self.device, self.frames, n, h, w, 3, 1 if self.bgr else 0, out_w, out_h, images)
        masks = rasterize(self.batch, (h, w), (out_h, out_w))
        return DeviceDataset(images, masks, device=self.device)
