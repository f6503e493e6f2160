"""TEST INFRASTRUCTURE ONLY - the numpy statement of the frame correction (include/unet_hip.h: unet_correct_u8_batch;
unet_lane_detection_amd/correct.py).  The kernels of csrc/correct_kernels.cpp are checked against it bit for bit: every
region of the work buffer (channel histograms, plan words, channel LUTs, tile histograms, tile LUTs) and the output.

Everything is an integer; `/` of the header is floor division of non-negative integers, written `//` here, and Python
integers are used where 64 bits matter.  The CLAHE is OpenCV's scheme restated in integers (clip, redistribute, residual
with a step, bilinear blend of the four tile tables); cv2 is not importable where this runs and the reference has no
such code, so parity with cv2.createCLAHE or any outside implementation is UNPINNED.

`MISTAKES` names deliberate errors the model can make on request; tests/test_correct_cpu.py shows that the cases the
GPU test runs (`CASES`) tell each of them apart from the right answer.
"""
import numpy as np

PLAN_WORDS = 8
FLAG_CORRECTED, FLAG_STRETCH, FLAG_CLAHE = 1, 2, 4
UNITY = 65536

MISTAKES = ("trunc_floor", "nominal_area", "no_residual", "u16_counters", "gray_before_lut", "tx1_unclamped",
            "stretch_unbalanced", "channels_exchanged", "padding_counted")


def config(white_balance=0, max_gain=4, lo_bp=0, hi_bp=0, tone=None, clahe=0, grid_x=1, grid_y=1, clip_q8=512,
           only_flagged=0, dark_limit=50, bright_limit=200):
    """the fields of unet_correct_config, in its order"""
    tone = np.arange(256, dtype=np.uint8) if tone is None else np.ascontiguousarray(tone, dtype=np.uint8).reshape(256)
    return dict(white_balance=int(white_balance), max_gain=int(max_gain), lo_bp=int(lo_bp), hi_bp=int(hi_bp),
                clahe=int(clahe), grid_x=int(grid_x), grid_y=int(grid_y), clip_q8=int(clip_q8),
                only_flagged=int(only_flagged), dark_limit=int(dark_limit), bright_limit=int(bright_limit), tone=tone)


def gamma_table(gamma):
    """what correct.CorrectConfig(gamma=...) puts into `tone`: rint(255 (v / 255)^gamma)"""
    v = np.arange(256, dtype=np.float64) / 255.0
    return np.clip(np.rint(255.0 * v ** float(gamma)), 0, 255).astype(np.uint8)


def frame_bytes(grid_x, grid_y):
    """the bytes of one frame's part of the work buffer"""
    g = grid_x * grid_y
    return 3 * 256 * 4 + PLAN_WORDS * 4 + 3 * 256 + g * 256 * 4 + g * 256


def work_bytes(n, grid_x, grid_y):
    return n * frame_bytes(grid_x, grid_y)


def gray(px, bgr):
    """(...,3) integers -> (...) : OpenCV 4's 8-bit gray, diagnose's formula"""
    px = np.asarray(px).astype(np.int64)
    b, r = (px[..., 0], px[..., 2]) if bgr else (px[..., 2], px[..., 0])
    return (3735 * b + 19235 * px[..., 1] + 9798 * r + 16384) >> 15


def _plan(hist, n_px, cfg, mistakes):
    """one frame's channel histograms -> (plan words, lut (3,256))"""
    v = np.arange(256, dtype=np.int64)
    sc = [int((v * hist[c]).sum()) for c in range(3)]
    s = sum(sc)
    ident = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    tail = [s & 0xFFFFFFFF, s >> 32]
    if cfg["only_flagged"] and cfg["dark_limit"] * 3 * n_px <= s <= cfg["bright_limit"] * 3 * n_px:
        return [0, UNITY, UNITY, UNITY, 0, 255] + tail, ident
    gains = []
    for c in range(3):
        if not cfg["white_balance"] or sc[c] == 0:
            gains.append(UNITY)
        else:
            g = (s << 16) // (3 * sc[c])
            gains.append(min(max(g, UNITY // cfg["max_gain"]), UNITY * cfg["max_gain"]))
    a = [np.minimum(255, (v * gains[c] + 32768) >> 16) for c in range(3)]
    flags, lo, hi = FLAG_CORRECTED, 0, 255
    s_of = v.copy()
    if cfg["lo_bp"] or cfg["hi_bp"]:
        pool = np.zeros(256, dtype=np.int64)
        for c in range(3):
            np.add.at(pool, v if "stretch_unbalanced" in mistakes else a[c], hist[c].astype(np.int64))
        cum = np.cumsum(pool)
        total = 3 * n_px
        lo = int(np.argmax(cum > cfg["lo_bp"] * total // 10000))
        hi = int(np.argmax(cum >= total - cfg["hi_bp"] * total // 10000))
        if hi > lo:
            flags |= FLAG_STRETCH
            d = hi - lo
            s_of = np.where(v < lo, 0, np.clip(((v - lo) * 255 + d // 2) // d, 0, 255))
    if cfg["clahe"]:
        flags |= FLAG_CLAHE
    lut = np.stack([cfg["tone"][s_of[a[c]]] for c in range(3)]).astype(np.uint8)
    return [flags] + gains + [lo, hi] + tail, lut


def tile_size(h, w, cfg):
    th, tw = -(-h // cfg["grid_y"]), -(-w // cfg["grid_x"])
    return th, tw


def grid_fits(h, w, grid_x, grid_y):
    """False for a grid that would leave a tile empty"""
    th, tw = -(-h // grid_y), -(-w // grid_x)
    return (grid_y - 1) * th < h and (grid_x - 1) * tw < w


def _tile_lut(hist, area, div_area, cfg, mistakes):
    hist = [int(x) for x in hist]
    limit = max(1, cfg["clip_q8"] * area // 65536)
    excess = sum(max(x - limit, 0) for x in hist)
    hist = [min(x, limit) for x in hist]
    hist = [x + excess // 256 for x in hist]
    r = excess % 256
    if r > 0 and "no_residual" not in mistakes:
        step = max(256 // r, 1)
        i = 0
        while i < 256 and r > 0:
            hist[i] += 1
            r -= 1
            i += step
    cdf = np.cumsum(np.array(hist, dtype=np.int64))
    return np.array([(255 * int(c) + div_area // 2) // div_area for c in cdf], dtype=np.int64)


def _clahe(px, bgr, cfg, mistakes, raw):
    """px (h,w,3): the frame after the channel LUTs -> (tile histograms, tile LUTs, output)"""
    h, w = px.shape[:2]
    gy, gx = cfg["grid_y"], cfg["grid_x"]
    th, tw = tile_size(h, w, cfg)
    y_plane = gray(raw if "gray_before_lut" in mistakes else px, bgr)
    thist = np.zeros((gy, gx, 256), dtype=np.int64)
    tlut = np.zeros((gy, gx, 256), dtype=np.int64)
    for ty in range(gy):
        for tx in range(gx):
            t = y_plane[ty * th:min((ty + 1) * th, h), tx * tw:min((tx + 1) * tw, w)]
            cnt = np.bincount(t.ravel(), minlength=256).astype(np.int64)
            if "u16_counters" in mistakes:
                cnt &= 0xFFFF
            thist[ty, tx] = cnt
            tlut[ty, tx] = _tile_lut(cnt, t.size, th * tw if "nominal_area" in mistakes else t.size, cfg, mistakes)

    def axis(size, t, g):
        x = 2 * np.arange(size, dtype=np.int64) + 1 - t
        t0 = (np.trunc(x / (2.0 * t)).astype(np.int64)) if "trunc_floor" in mistakes else x // (2 * t)
        wgt = x - t0 * 2 * t
        return np.clip(t0, 0, g - 1), t0 + 1, wgt

    ty0, ty1, wy = axis(h, th, gy)
    tx0, tx1, wx = axis(w, tw, gx)
    ty1 = np.clip(ty1, 0, gy - 1)
    flat = tlut.reshape(gy * gx, 256)
    if "tx1_unclamped" in mistakes:     # the next table in memory, whatever it is
        col1 = lambda ty: np.clip(ty[:, None] * gx + tx1[None, :], 0, gy * gx - 1)
    else:
        tx1 = np.clip(tx1, 0, gx - 1)
        col1 = lambda ty: ty[:, None] * gx + tx1[None, :]
    col0 = lambda ty: ty[:, None] * gx + tx0[None, :]
    wy, wx = wy[:, None], wx[None, :]
    top = (2 * tw - wx) * flat[col0(ty0), y_plane] + wx * flat[col1(ty0), y_plane]
    bot = (2 * tw - wx) * flat[col0(ty1), y_plane] + wx * flat[col1(ty1), y_plane]
    y2 = ((2 * th - wy) * top + wy * bot + 2 * tw * th) // (4 * tw * th)
    safe = np.maximum(y_plane, 1)
    scaled = np.minimum(255, (px.astype(np.int64) * y2[..., None] + (y_plane // 2)[..., None]) // safe[..., None])
    out = np.where((y_plane == 0)[..., None], y2[..., None], scaled)
    return thist, tlut, out.astype(np.uint8)


def correct(frames, cfg, bgr=True, mistakes=(), padded=None):
    """frames (n,h,w,3) uint8 -> dict of every intermediate and the output:
        hist (n,3,256) uint32, plan (n,8) uint32, lut (n,3,256) uint8, tile_hist (n,gy,gx,256) uint32,
        tile_lut (n,gy,gx,256) uint8, out (n,h,w,3) uint8
    padded: the same frames as raw rows (n,h,stride), which only the mistake "padding_counted" looks at."""
    frames = np.asarray(frames)
    n, h, w, _ = frames.shape
    gy, gx = cfg["grid_y"], cfg["grid_x"]
    if "channels_exchanged" in mistakes and not bgr:
        bgr = True
    res = dict(hist=np.zeros((n, 3, 256), np.uint32), plan=np.zeros((n, PLAN_WORDS), np.uint32),
               lut=np.zeros((n, 3, 256), np.uint8), tile_hist=np.zeros((n, gy, gx, 256), np.uint32),
               tile_lut=np.tile(np.arange(256, dtype=np.uint8), (n, gy, gx, 1)), out=np.zeros_like(frames))
    for i in range(n):
        f = frames[i]
        if "padding_counted" in mistakes and padded is not None:
            row = padded[i]
            hist = np.stack([np.bincount(row[:, c::3].ravel(), minlength=256) for c in range(3)])
        else:
            hist = np.stack([np.bincount(f[..., c].ravel(), minlength=256) for c in range(3)])
        plan, lut = _plan(hist, h * w, cfg, mistakes)
        res["hist"][i], res["plan"][i], res["lut"][i] = hist, plan, lut
        px = np.stack([lut[c][f[..., c]] for c in range(3)], axis=-1)
        if plan[0] & FLAG_CLAHE:
            th_, tl_, px = _clahe(px, bgr, cfg, mistakes, f)
            res["tile_hist"][i], res["tile_lut"][i] = th_, tl_
        res["out"][i] = px
    return res


def pack_work(res):
    """the work buffer the call leaves behind, byte for byte: per frame histograms, plan, LUTs, tile histograms, tile
    LUTs"""
    parts = []
    for i in range(res["hist"].shape[0]):
        for key in ("hist", "plan", "lut", "tile_hist", "tile_lut"):
            parts.append(np.ascontiguousarray(res[key][i]).reshape(-1).view(np.uint8))
    return np.concatenate(parts)


def padded_rows(frames, stride, fill=255):
    """(n,h,w,3) -> (n,h,stride) raw rows, the padding set to `fill`"""
    n, h, w, _ = frames.shape
    rows = np.full((n, h, stride), fill, dtype=np.uint8)
    rows[:, :, :3 * w] = frames.reshape(n, h, 3 * w)
    return rows


# ---- the frames and cases of the GPU test ----------------------------------------------------------------------------

def scene(seed, n, h, w, base=(60, 110, 150), spread=70):
    """n different frames with a colour cast, a brightness ramp, blocks of other levels and noise: uneven histograms,
    tiles that differ from each other, all three channels different"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w, 3), dtype=np.int64)
    for i in range(n):
        ramp = (xx * spread) // max(w - 1, 1) + (yy * spread // 2) // max(h - 1, 1)
        for c in range(3):
            out[i, ..., c] = base[(c + i) % 3] + ramp * (c + 1) // 2 + rng.integers(-12, 13, (h, w))
        for _ in range(4):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            out[i, y0:y0 + max(h // 3, 1), x0:x0 + max(w // 3, 1)] += int(rng.integers(-60, 90))
        dots = rng.random((h, w)) < 0.02
        out[i][dots] = rng.integers(0, 256, (int(dots.sum()), 3))
    return np.clip(out, 0, 255).astype(np.uint8)


TONE = gamma_table(0.8)
ALL = dict(white_balance=1, lo_bp=100, hi_bp=100, tone=TONE, clahe=1)


def _flagged_batch():
    f = scene(31, 3, 20, 24)
    f[0] = f[0] // 6             # mean below 50
    f[2] = 215 + f[2] // 8       # mean above 200
    return f


def _gain_frames():
    f = scene(32, 3, 12, 20)
    f[0, ..., 1] = 0             # S_c = 0: the gain stays at unity
    f[1, ..., 0] = 0
    f[1, 3, 4:7, 0] = 1          # nearly zero: the gain is cut off at max_gain
    f[2, ..., 2] = 250
    f[2, ..., :2] //= 16         # one channel carries the frame: its gain is cut off at 1 / max_gain
    return f


# name -> (frames, cfg keywords, extras); extras: stride (bytes beyond 3 w), lead (offset of the input from a 64-byte
# boundary), inplace.  Every case runs with is_bgr 1 and 0.
CASES = {
    "odd_37x53_grid4x3": (scene(1, 3, 37, 53), dict(ALL, grid_x=4, grid_y=3), {}),
    "aligned_16x64": (scene(2, 2, 16, 64), dict(ALL, grid_x=4, grid_y=2), {}),
    "offset65_16x64": (scene(2, 2, 16, 64), dict(ALL, grid_x=4, grid_y=2), dict(stride=5, lead=1)),
    "grid1x1_16x16": (scene(3, 1, 16, 16), dict(ALL, grid_x=1, grid_y=1), {}),
    "grid16x16_16x16": (scene(3, 1, 16, 16), dict(ALL, grid_x=16, grid_y=16), {}),
    "flat_300x300": (np.full((1, 300, 300, 3), 93, np.uint8), dict(ALL, grid_x=1, grid_y=1), {}),
    "zeros": (np.zeros((1, 9, 11, 3), np.uint8), dict(ALL, grid_x=2, grid_y=2), {}),
    "gain_clamp": (_gain_frames(), dict(ALL, max_gain=2, grid_x=2, grid_y=2), {}),
    "only_flagged": (_flagged_batch(), dict(ALL, only_flagged=1, grid_x=3, grid_y=2), dict(stride=7)),
    "in_place": (scene(4, 2, 21, 35), dict(ALL, grid_x=3, grid_y=3), dict(inplace=True, stride=3)),
    "white_balance_alone": (scene(5, 2, 19, 33), dict(white_balance=1), {}),
    "stretch_alone": (scene(6, 2, 19, 33), dict(lo_bp=200, hi_bp=50), {}),
    "tone_alone": (scene(7, 2, 19, 33), dict(tone=TONE), {}),
    "clahe_alone": (scene(8, 2, 19, 33), dict(clahe=1, grid_x=3, grid_y=2, clip_q8=768), {}),
    "nothing": (scene(9, 1, 7, 5), dict(), {}),
    "wide_640x24_grid8x2": (scene(10, 1, 24, 640), dict(ALL, grid_x=8, grid_y=2), {}),
}


def case(name):
    frames, kw, extras = CASES[name]
    return frames, config(**kw), dict(extras)


# ---- the reference's failure case 1: a blue-deficient cast on a gray track with white markings ----------------------

TRACK_SURFACE, TRACK_WHITE, CAST_BLUE = 100, 240, 0.7


def track(h=480, w=640):
    """(h,w,3) uint8 BGR: a gray surface with two white markings that converge towards the top.  Both levels are at
    least 16 away from every threshold of the extractor (V 185, S 40) - before the cast, under it (the markings then
    have S = 76) and after the gray-world correction (V = 216)."""
    img = np.full((h, w, 3), TRACK_SURFACE, dtype=np.uint8)
    for y in range(h):
        half = w // 10 + (w // 4) * y // h
        for centre in (w // 2 - half, w // 2 + half):
            img[y, max(centre - 12, 0):centre + 12] = TRACK_WHITE
    return img


def cast(img, blue=CAST_BLUE, bgr=True):
    """the blue channel scaled by `blue`"""
    out = img.copy()
    c = 0 if bgr else 2
    out[..., c] = np.floor(img[..., c].astype(np.float64) * blue + 0.5).astype(np.uint8)
    return out
