"""TEST INFRASTRUCTURE ONLY - the numpy statement of lane following's three pieces (include/unet_hip.h:
unet_hsv_lanes_u8_batch, unet_lane_center_u8_batch; unet_lane_detection_amd/follow.py: lane_centers).  The kernels are
checked against it bit for bit.

The extractor is the reference's `extract_white_lanes` (README.md:206-227): cvtColor(BGR2HSV), inRange, morphologyEx
CLOSE and OPEN with a k x k box.  The HSV plane is augment.rgb_to_hsv, the project's stated 8-bit HSV; cv2 is not
importable here, so parity with cv2's own table-driven BGR2HSV is UNPINNED.  Dilate and erode are a box maximum and
minimum over an image padded with the neutral value (0 for the maximum, 255 for the minimum): OpenCV's default border
for both, under which pixels outside the image never take part - at every one of the four steps.

The lane centre is `LineFollower.find_lane_center` (README.md:4115-4126): the mean x of the pixels above 127 on the scan
row at 70 % height, if there are more than 10 of them; int(np.mean(xs)) equals sum // count for every width in use.
"""
import numpy as np

from unet_lane_detection_amd.augment import rgb_to_hsv

DEFAULT_LOWER, DEFAULT_UPPER = (0, 0, 185), (180, 40, 255)


def in_range(frames, lower=DEFAULT_LOWER, upper=DEFAULT_UPPER, bgr=True):
    """(...,3) uint8 -> (...) uint8 of 0 / 255: lower[c] <= HSV[c] <= upper[c] for all three channels."""
    frames = np.asarray(frames)
    return in_range_hsv(rgb_to_hsv(frames[..., ::-1] if bgr else frames), lower, upper)


def in_range_hsv(hsv, lower=DEFAULT_LOWER, upper=DEFAULT_UPPER):
    """cv2.inRange on an HSV plane (...,3) uint8"""
    hsv = np.asarray(hsv).astype(np.int64)
    lo, hi = np.asarray(lower, dtype=np.int64), np.asarray(upper, dtype=np.int64)
    return (((hsv >= lo) & (hsv <= hi)).all(axis=-1) * 255).astype(np.uint8)


def _box(plane, k, fn, neutral):
    """k x k box maximum (fn = np.maximum) or minimum of a (H,W) plane padded with `neutral`."""
    r = int(k) // 2
    h, w = plane.shape
    pad = np.pad(plane, ((r, r), (r, r)), mode="constant", constant_values=neutral)
    rows = pad[:, 0:w]
    for d in range(1, 2 * r + 1):
        rows = fn(rows, pad[:, d:d + w])
    out = rows[0:h]
    for d in range(1, 2 * r + 1):
        out = fn(out, rows[d:d + h])
    return out


def dilate(plane, k):
    return _box(plane, k, np.maximum, 0)


def erode(plane, k, pad=255):
    """pad = 255 is the rule; pad = 0 is the mutant the tests must tell apart"""
    return _box(plane, k, np.minimum, pad)


def close_open(plane, close_ksize=5, open_ksize=5, erode_pad=255):
    """(H,W) uint8 -> (H,W) uint8: dilate kc, erode kc (CLOSE), erode ko, dilate ko (OPEN), each on the whole image."""
    x = dilate(plane, close_ksize)
    x = erode(x, close_ksize, erode_pad)
    x = erode(x, open_ksize, erode_pad)
    return dilate(x, open_ksize)


def hsv_lanes(frames, lower=DEFAULT_LOWER, upper=DEFAULT_UPPER, close_ksize=5, open_ksize=5, bgr=True, erode_pad=255):
    """frames (N,H,W,3) uint8 -> masks (N,H,W) uint8 of 0 / 255"""
    t = in_range(frames, lower, upper, bgr)
    return np.stack([close_open(p, close_ksize, open_ksize, erode_pad) for p in t])


def lane_sums(masks, rows, level=127):
    """masks (N,H,W) uint8, rows: row indices -> (N, len(rows), 2) int64: count and sum of the x with mask > level"""
    masks = np.asarray(masks)
    x = np.arange(masks.shape[2], dtype=np.int64)
    on = masks[:, list(rows), :].astype(np.int64) > int(level)
    return np.stack([on.sum(axis=2), (on * x).sum(axis=2)], axis=2)


def default_row(height):
    return int(height * 0.7)


def lane_centers(masks, scan_rows=None, level=127, min_pixels=10):
    """-> list (N) of lists (rows) of sum // count where count > min_pixels, else None"""
    masks = np.asarray(masks)
    rows = [default_row(masks.shape[1])] if scan_rows is None else list(scan_rows)
    s = lane_sums(masks, rows, level)
    return [[int(c[1] // c[0]) if c[0] > min_pixels else None for c in frame] for frame in s]


def painted_seed(n, h, w):
    """the seed the tests paint a shape's frames with"""
    return 1000 * n + h + w


def painted_frames(seed, n, h, w):
    """Test frames painted from binary fields: random rectangles up to a third of the image with 3 % and 8 % of the
    pixels flipped (per frame alternately); "white" pixels are grey 215..255 plus up to +-4 per channel, the others
    uniformly random colours.  Returns (frames (n,h,w,3) uint8, fields (n,h,w) bool)."""
    rng = np.random.default_rng(seed)
    field = np.zeros((n, h, w), dtype=bool)
    for i in range(n):
        for _ in range(6):
            rh, rw = int(rng.integers(1, max(h // 3, 1) + 1)), int(rng.integers(1, max(w // 3, 1) + 1))
            y0, x0 = int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))
            field[i, y0:y0 + rh, x0:x0 + rw] = True
        field[i] ^= rng.random((h, w)) < (0.03 if i % 2 == 0 else 0.08)
    grey = rng.integers(215, 256, size=(n, h, w, 1)) + rng.integers(-4, 5, size=(n, h, w, 3))
    white = np.clip(grey, 0, 255).astype(np.uint8)
    other = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    return np.where(field[..., None], white, other), field
