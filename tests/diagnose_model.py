"""TEST INFRASTRUCTURE ONLY - the numpy statement of the two diagnostics records (include/unet_hip.h:
unet_frame_stats_u8_batch, unet_prob_stats_f32_batch) and of the host formulas of unet_lane_detection_amd/diagnose.py.
The kernels are checked against it bit for bit.

The frame record is the reference's `diagnose_input_image` (README.md:4476-4496): img.min(), img.max(), img.mean() and
cv2.Laplacian(cv2.cvtColor(img, BGR2GRAY), CV_64F).var().  The gray plane is OpenCV 4's 8-bit formula
(3735 B + 19235 G + 9798 R + 16384) >> 15 and the Laplacian its ksize = 1 kernel with the default border (reflect-101);
cv2 is not importable here and the reference ships no fixture, so parity with cv2 itself is UNPINNED.  The probability
record is the reference's `quick_test` (README.md:4615-4640): output range, mean and share above the threshold.

The `border`, `count_padding`, `swap` and `s2_chunk` arguments produce the look-alikes tests/test_diagnose_cpu.py shows
the test frames to tell apart; the defaults are the rule.
"""
import numpy as np

FRAME_WORDS, PROB_WORDS = 8, 4
MASK64 = (1 << 64) - 1


# ---- frames ------------------------------------------------------------------------------------------------------

def gray(frames, bgr=True):
    """(...,3) uint8 -> (...) int64: OpenCV 4's 8-bit BGR2GRAY (RGB2GRAY with bgr=False)"""
    f = np.asarray(frames).astype(np.int64)
    b, g, r = (f[..., 0], f[..., 1], f[..., 2]) if bgr else (f[..., 2], f[..., 1], f[..., 0])
    return (3735 * b + 19235 * g + 9798 * r + 16384) >> 15


def _neighbours(n, border):
    """indices of i-1 and i+1 for i in [0, n) under reflect-101 (or, the mutant, replicate); i itself where n is 1"""
    i = np.arange(n)
    if n == 1:
        return i, i
    lo, hi = i - 1, i + 1
    if border == "reflect101":
        lo[0], hi[-1] = 1, n - 2
    elif border == "replicate":
        lo[0], hi[-1] = 0, n - 1
    else:
        raise ValueError(border)
    return lo, hi


def laplacian(y, border="reflect101"):
    """(H,W) int64 gray -> (H,W) int64: cv2.Laplacian at ksize = 1"""
    y = np.asarray(y).astype(np.int64)
    up, down = _neighbours(y.shape[0], border)
    left, right = _neighbours(y.shape[1], border)
    return y[up, :] + y[down, :] + y[:, left] + y[:, right] - 4 * y


def frame_records(frames, bgr=True, width=None, border="reflect101", count_padding=False, swap=False, s2_chunk=None):
    """frames (N,H,W,3) uint8, or raw rows (N,H,stride) uint8 with `width` given -> (N,8) uint64 records.
    border, count_padding (padding bytes enter minimum, maximum and sum), swap (R and B exchanged in the gray) and
    s2_chunk (S2 summed in 32-bit words per that many pixels) are the mutants."""
    a = np.asarray(frames)
    if width is None:
        px, counted = a, a.reshape(a.shape[0], -1)
    else:
        px = a[:, :, :3 * width].reshape(a.shape[0], a.shape[1], width, 3)
        counted = a.reshape(a.shape[0], -1) if count_padding else px.reshape(a.shape[0], -1)
    out = np.zeros((a.shape[0], FRAME_WORDS), dtype=np.uint64)
    for i in range(a.shape[0]):
        lap = laplacian(gray(px[i], bgr != swap), border)
        sq = (lap * lap).reshape(-1)
        if s2_chunk is None:
            s2 = int(sq.sum())
        else:
            s2 = sum(int(sq[k:k + s2_chunk].sum()) & 0xFFFFFFFF for k in range(0, sq.size, s2_chunk))
        words = [int(counted[i].min()), int(counted[i].max()), int(counted[i].astype(np.int64).sum()),
                 int(lap.sum()) & MASK64, s2]
        out[i, :5] = np.array(words, dtype=np.uint64)
    return out


def frame_mean(rec, height, width):
    """img.mean() from a record: exact integers, one rounding"""
    return int(rec[2]) / (3 * height * width)


def frame_s1(rec):
    v = int(rec[3])
    return v - (1 << 64) if v >> 63 else v


def frame_sharpness(rec, height, width):
    """Laplacian.var() from a record: (N S2 - S1^2) / N^2 in exact integers, one rounding"""
    n, s1, s2 = height * width, frame_s1(rec), int(rec[4])
    return (n * s2 - s1 * s1) / (n * n)


def frames_seed(n, h, w):
    """the seed the tests make a shape's frames with"""
    return 7000 * n + 3 * h + w


def make_frames(seed, n, h, w):
    """Frames (n,h,w,3) uint8 the mutants cannot pass: a checkerboard of bright (200..255) and dark (0..55) pixels,
    coloured per channel, with a tenth of the pixels replaced by uniformly random colours.  |L| is around 800 at most
    pixels, so 8,192 squares pass 2^32; the channels differ, so R and B matter; the borders are as busy as the rest."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    board = ((yy + xx) & 1).astype(bool)[None, :, :, None]
    bright = rng.integers(200, 256, size=(n, h, w, 3), dtype=np.uint8)
    dark = rng.integers(0, 56, size=(n, h, w, 3), dtype=np.uint8)
    img = np.where(board, bright, dark)
    noise = rng.random((n, h, w, 1)) < 0.1
    return np.where(noise, rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8), img).astype(np.uint8)


# the random frame cases of tests/test_diagnose_gpu.py, (n, h, w): odd sizes, a multiple of the tile, the degenerate
# ones, and one in which several 32-row strips and 254-column tiles meet
FRAME_CASES = [(3, 67, 131), (2, 64, 256), (1, 1, 9), (1, 9, 1), (2, 2, 2), (1, 300, 700)]
PADDED_CASE = ((2, 5, 7), 26)     # (n, h, w), row_stride; the padding is filled with 255


def padded_rows(frames, row_stride, fill=255):
    """(N,H,W,3) -> raw rows (N,H,row_stride) with the padding set to `fill`"""
    n, h, w, _ = frames.shape
    rows = np.full((n, h, row_stride), fill, dtype=np.uint8)
    rows[:, :, :3 * w] = frames.reshape(n, h, 3 * w)
    return rows


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[None, :, :, None], 3, axis=3)


# ---- probability planes ------------------------------------------------------------------------------------------

def float_key(bits):
    """uint32 fp32 bits -> uint32 keys, monotone in the value, -0.0 below +0.0"""
    bits = np.asarray(bits, dtype=np.uint32)
    return np.where(bits >> 31 != 0, ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def prob_records(scores, threshold=0.5):
    """scores (N, ...) float32 -> (N,4) uint64 records"""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    s = s.reshape(s.shape[0], -1)
    thr = np.float32(threshold)
    inf = np.array([np.inf, -np.inf], dtype=np.float32).view(np.uint32)
    out = np.zeros((s.shape[0], PROB_WORDS), dtype=np.uint64)
    for i, row in enumerate(s):
        nan = np.isnan(row)
        v = row[~nan]
        bits = v.view(np.uint32)
        if v.size:
            keys = float_key(bits)
            lo, hi = int(bits[np.argmin(keys)]), int(bits[np.argmax(keys)])
        else:
            lo, hi = int(inf[0]), int(inf[1])
        frac = np.floor(np.clip(v.astype(np.float64), 0.0, 1.0) * 4294967296.0).astype(np.uint64)
        words = [(hi << 32) | lo, int((v > thr).sum()), int(frac.sum(dtype=np.uint64)), int(nan.sum())]
        out[i] = np.array(words, dtype=np.uint64)
    return out


def prob_min_max(rec):
    w = np.array([int(rec[0]) & 0xFFFFFFFF, int(rec[0]) >> 32], dtype=np.uint32).view(np.float32)
    return float(w[0]), float(w[1])


def prob_mean(rec, numel):
    return int(rec[2]) / ((1 << 32) * numel)


SPECIAL_THRESHOLD = 0.5


def special_values(threshold=SPECIAL_THRESHOLD):
    """[NaN, -inf, -0.0, 0.0, subnormal, threshold, nextafter(threshold), 1.0, 1.5, +inf]"""
    t = np.float32(threshold)
    return np.array([np.nan, -np.inf, -0.0, 0.0, 1e-45, t, np.nextafter(t, np.float32(2.0)), 1.0, 1.5, np.inf],
                    dtype=np.float32)
