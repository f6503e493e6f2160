"""The lane view's host side: the entry point is exported, prototyped and refuses everything outside its domain before
a device is touched; the 63-bit bound of the curve evaluation in Python ints; `laneview.quantise` and `curve_table`;
tests/laneview_model.py against closed forms of the area between two curves; and the inputs of
tests/test_laneview_gpu.py are a test of the definition - each of the model's mutants changes an output on them."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import laneview_cases as LC
import laneview_model as M
from unet_lane_detection_amd import _lib
from unet_lane_detection_amd import lanefit as LF
from unet_lane_detection_amd import laneview as LV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the entry point -------------------------------------------------------------------------------------------

def test_symbols_exported_and_prototyped(lib):
    for name in ("unet_lane_view_u8_batch", "unet_lane_view_style_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "unet_hip.h")) as f:
        header = f.read()
    assert "int unet_lane_view_u8_batch(int device, const uint8_t* frames_dev, int n, int height, int width, int step," in header
    assert "#define UNET_LANE_VIEW_WORDS 8" in header and "#define UNET_LANE_VIEW_MAX 8" in header
    section = header[header.index("lane view on the device"):header.index("unet_lane_view_u8_batch(int device")]
    assert "unpinned" in section and "2^62 + 2^61 + 2^57 < 2^63" in section
    assert header.index("unet_keep_components_u8_batch(int device") < header.index("unet_lane_view_u8_batch(int device")
    assert (LV.VIEW_WORDS, LV.VIEW_MAX) == (8, 8) == (M.WORDS, M.MAX)
    assert lib.unet_lane_view_style_bytes() == C.sizeof(_lib.LaneViewStyle) == 28
    from unet_lane_detection_amd.build import SOURCES
    assert "laneview_kernels.cpp" in SOURCES


def test_lane_view_refuses_bad_arguments(lib):
    """null DEVICE pointers throughout: a call that got past the checks would have to touch a device to go wrong, and
    the host bytes behind the outputs stay clear"""
    call = lib.unet_lane_view_u8_batch
    name = b"unet_lane_view_u8_batch"
    frames = C.cast((C.c_uint8 * 64)(), C.c_void_p)
    masks = C.cast((C.c_uint8 * 64)(), C.c_void_p)
    words = (C.c_int64 * 72)()
    curves = C.cast(words, C.c_void_p)
    view_bytes, layer_bytes = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    view, layers = C.cast(view_bytes, C.c_void_p), C.cast(layer_bytes, C.c_void_p)
    eye = np.eye(3).reshape(9)

    def refused(rc, word):
        msg = lib.unet_op_last_error()
        return rc == 1 and msg.startswith(b"invalid argument") and name in msg and word in msg

    def go(frames=frames, n=1, h=2, w=4, step=12, m=eye, ww=4, wh=2, masks=masks, level=127, curves=curves, k=1,
           style=None, view=view, layers=layers, device=0):
        mp = None if m is None else np.ascontiguousarray(m, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
        sp = None if style is None else C.byref(style)
        return call(device, frames, n, h, w, step, mp, ww, wh, masks, level, curves, k, sp, view, layers, None)

    def style(**kw):
        s = LV.ViewConfig().style()
        for key, value in kw.items():
            setattr(s, key, value)
        return s
    assert refused(go(frames=None), b"null")
    assert refused(go(m=None), b"null")
    assert refused(go(view=None, layers=None), b"both")
    for n in (0, -1):
        assert refused(go(n=n), b"n must")
    for h in (0, -2, 4097):
        assert refused(go(h=h), b"height")
    for w in (0, -4, 4097):
        assert refused(go(w=w, step=3 * 4097), b"width")
    for step in (11, 0, -12):
        assert refused(go(step=step), b"step")
    assert refused(go(n=128, h=4096, w=1, step=4096), b"2^31")              # exactly 2^31 bytes
    assert refused(go(n=1 << 20, h=4096, w=4096, step=3 * 4096), b"2^31")   # a product that overflows 32 bits
    for ww in (0, -1, 8193):
        assert refused(go(ww=ww), b"warp_w")
    for wh in (0, -1, 2049):
        assert refused(go(wh=wh), b"warp_h")
    for level in (-1, 256):
        assert refused(go(level=level), b"level")
    for k in (-1, 9):
        assert refused(go(k=k), b"k must lie")
    assert refused(go(k=0), b"exactly when")
    assert refused(go(curves=None, k=1), b"exactly when")
    assert refused(go(curves=C.c_void_p(curves.value + 4)), b"8-byte")
    for i in range(9):
        for bad in (math.nan, math.inf, -math.inf):
            m = eye.copy()
            m[i] = bad
            assert refused(go(m=m), b"finite")
    for field in ("alpha", "beta", "gamma"):
        for bad in (math.nan, math.inf):
            assert refused(go(style=style(**{field: bad})), b"alpha, beta and gamma")
    for t in (0, -1, 65):
        assert refused(go(style=style(thickness=t)), b"thickness")
    assert refused(go(style=style(layers=4)), b"layers")
    assert not any(view_bytes) and not any(layer_bytes)
    # what passes the checks goes on to the device: an ordinal the runtime refuses shows it got that far
    bad = 1 << 20
    for kw in (dict(), dict(masks=None), dict(curves=None, k=0), dict(view=None), dict(layers=None), dict(k=8),
               dict(style=style(thickness=64, layers=0)), dict(style=style(thickness=1, layers=3)),
               dict(n=127, h=4096, w=1, step=4096), dict(h=4096, w=4096, step=3 * 4096, ww=8192, wh=2048, level=255),
               dict(h=1, w=1, step=3, ww=1, wh=1, level=0)):
        assert go(device=bad, **kw) == _lib.UNET_ERR_HIP, kw
        assert b"hipSetDevice" in lib.unet_op_last_error()
    assert not any(view_bytes) and not any(layer_bytes)


# ---- the integers ----------------------------------------------------------------------------------------------

def test_largest_sum_fits_63_bits():
    """the header's derivation at the extreme record: every clamped coefficient at its bound, Y at its largest"""
    a, b, c, y = M.A_BOUND, M.B_BOUND, M.C_BOUND, M.Y_LIMIT - 1
    assert (a, b, c) == ((1 << 30) - 1, (1 << 45) - 1, (1 << 57) - 1) and y == 32 * 2048 - 1
    assert (LV.A_LIMIT, LV.B_LIMIT, LV.C_LIMIT) == (a + 1, b + 1, c + 1)
    largest = a * y * y + b * y + c
    assert largest < (1 << 62) + (1 << 61) + (1 << 57) < 1 << 63
    assert largest / 2 ** 63 > 0.75                                    # the bound is not a loose one
    with open(os.path.join(ROOT, "include", "unet_hip.h")) as f:
        assert f"{largest:,}".replace(",", " ") in f.read()
    # every partial sum of every sign pattern, as the kernel forms them
    for sa in (1, -1):
        for sb in (1, -1):
            for sc in (1, -1):
                for term in (sa * a * y, sa * a * y * y, sa * a * y * y + sb * b * y, sa * a * y * y + sb * b * y + sc * c):
                    assert -(1 << 63) <= term < 1 << 63
    # and the model's int64 arithmetic agrees with Python's ints there, the floor below zero included
    t = LC.extreme_records()[0]
    _, _, _, A, B, C_, _ = M.clamp_records(t, 2048)
    for i in range(4):
        want = (int(A[i]) * y * y + int(B[i]) * y + int(C_[i])) >> 32
        assert int(M.x32(A[i], B[i], C_[i], np.int64(y))) == want
    # a record of random words is clamped into that domain
    rng = np.random.default_rng(5)
    wild = rng.integers(-(1 << 63), (1 << 63) - 1, (64, M.WORDS), dtype=np.int64, endpoint=True)
    flags, lo, hi, A, B, C_, col = M.clamp_records(wild, 2048)
    assert (np.abs(A) <= a).all() and (np.abs(B) <= b).all() and (np.abs(C_) <= c).all()
    assert (lo >= 0).all() and (hi <= 32 * 2047 + 31).all() and (flags < 8).all() and (col < 1 << 24).all()


def test_quantise_round_trip_and_refusal():
    rng = np.random.default_rng(11)
    for _ in range(200):
        co = (float(rng.uniform(-7.9, 7.9)), float(rng.uniform(-8000, 8000)), float(rng.uniform(-1e6, 1e6)))
        A, B, C_ = LV.quantise(co)
        for q, v, bits in ((A, co[0], 27), (B, co[1], 32), (C_, co[2], 37)):
            exact = Fraction(v) * (1 << bits)
            assert isinstance(q, int) and abs(q - exact) <= Fraction(1, 2)
            if abs(q - exact) == Fraction(1, 2):
                assert q % 2 == 0                                      # half to even
    assert LV.quantise((2.0 ** -28, -(2.0 ** -33), 1.5 * 2.0 ** -37)) == (0, 0, 2)      # ties go to the even integer
    assert LV.quantise((3 * 2.0 ** -28, 0.0, 2.5 * 2.0 ** -37)) == (2, 0, 2)
    assert LV.quantise((1.0, -1.0, 0.03125)) == (1 << 27, -(1 << 32), 1 << 32)
    # the domain: |A| < 2^30, |B| < 2^45, |C| < 2^57
    edge = (8.0 - 2.0 ** -27, 8192.0 - 2.0 ** -32, math.nextafter(2.0 ** 20, 0.0))     # the last: 2^20 - 2^-33
    assert LV.quantise(edge) == ((1 << 30) - 1, (1 << 45) - 1, (1 << 57) - 16)
    assert LV.quantise(tuple(-v for v in edge)) == (-(1 << 30) + 1, -(1 << 45) + 1, -(1 << 57) + 16)
    for bad in ((8.0, 0, 0), (-8.0, 0, 0), (0, 8192.0, 0), (0, -8192.0, 0), (0, 0, 2.0 ** 20), (0, 0, -2.0 ** 20),
                (math.nan, 0, 0), (0, math.inf, 0), (0, 0, -math.inf), (1e308, 0, 0), (0, 0, 1e308)):
        assert LV.quantise(bad) is None, bad
    assert LV.quantise(None) is None


def _fits(words_by_frame, height, width):
    return LF.LaneFits.from_records(np.array(words_by_frame, dtype=np.uint64), height, width)


def _lane_words(points):
    """a lane-fit record whose sums are those of the pixels (x, y)"""
    if not points:
        return [0] * 5 + [0] * 8 + [100, 0, 0]
    S = [sum(y ** k for _, y in points) for k in range(5)]
    T = [sum(x * y ** k for x, y in points) for k in range(3)]
    ys = [y for _, y in points]
    return [1, 0, 1, 1, 0] + S + T + [min(ys), max(ys), 0]


def test_curve_table_from_fits_and_instances():
    h, w = 100, 160
    left = [(30 + y // 10, y) for y in range(20, 90)]
    right = [(120 - y // 20, y) for y in range(10, 95)]
    fits = _fits([[_lane_words(left), _lane_words(right)], [_lane_words(left), _lane_words([])]], h, w)
    t = LV.curve_table(fits, (w, h))
    assert t.shape == (2, 2, 8) and t.dtype == np.int64
    assert [int(v) for v in t[0, :, 0]] == [7, 5] and [int(v) for v in t[1, :, 0]] == [7, 0]      # fill on the left only
    assert [tuple(r[1:3]) for r in t[0]] == [(0, h - 1), (0, h - 1)]
    for lane, rec in zip(fits[0].lanes, t[0]):
        assert tuple(int(v) for v in rec[3:6]) == LV.quantise(lane.coeffs) and rec[7] == 0
    assert int(t[0, 0, 6]) == 255 and int(t[0, 1, 6]) == 255 << 16                                 # the default colours
    assert not t[1, 1].any()                                                                        # an absent lane
    pix = LV.curve_table(fits, (w, h), LV.ViewConfig(extent="pixels", draw_curves=False, fill=False))
    assert [tuple(int(v) for v in r[:3]) for r in pix[0]] == [(1, 20, 89), (1, 10, 94)]
    # instances: left to right, capped, fill between neighbours
    from unet_lane_detection_amd.instances import LaneInstance

    def inst(i, x):
        pts = [(x, y) for y in range(5 + i, 60 + i)]
        fit = LF.LaneFit(np.array(_lane_words(pts), dtype=np.uint64), h, LF.FitConfig())
        return LaneInstance(0, i + 1, fit, len(pts), (x, x, 5 + i, 59 + i), 1.0, (float(x), 30.0))
    many = [[inst(i, 10 + 12 * i) for i in range(10)], [inst(0, 50)], []]
    t = LV.curve_table(many, (w, h), LV.ViewConfig(extent="pixels"))
    assert t.shape == (3, 8, 8)
    assert [int(v) for v in t[0, :, 0]] == [7] * 7 + [5] and [int(v) for v in t[1, :, 0]] == [5] + [0] * 7
    assert not t[2].any() and tuple(int(v) for v in t[0, 3, 1:3]) == (8, 62)
    assert LV.curve_table([[], []], (w, h)).shape == (2, 0, 8)
    with pytest.raises(ValueError):
        LV.ViewConfig(extent="rows")


def test_orient_puts_the_road_below_the_horizon():
    """cv2.getPerspectiveTransform scales the reference's matrix so that w is negative on the whole road: as it
    stands the definition's `w > 0` would draw nothing there"""
    from unet_lane_detection_amd import ros_bridge as RB
    m = RB.get_perspective_transform(RB.REF_SRC_POINTS, RB.REF_DST_POINTS)
    o = LV.orient(m, RB.REF_WARP_SIZE)
    assert np.array_equal(o, -m) and o is not m
    for x, y in RB.REF_SRC_POINTS:
        assert o[2, 0] * x + o[2, 1] * y + o[2, 2] > 0 > m[2, 0] * x + m[2, 1] * y + m[2, 2]
    assert np.array_equal(LV.orient(o, RB.REF_WARP_SIZE), o)
    assert np.array_equal(LV.orient(np.eye(3), (64, 32)), np.eye(3))
    assert np.array_equal(LV.orient(-np.eye(3), (64, 32)), np.eye(3))
    frames, masks = LC.frames_of(1, 1, 480, 640), np.full((1, 685, 1055), 255, dtype=np.uint8)
    assert not M.lane_view(frames, m, 1055, 685, masks)[1].any()
    lit = M.lane_view(frames, o, 1055, 685, masks)[1]
    assert (lit == 2).any() and not lit[0, 0].any()          # the top row is sky


# ---- the model against closed forms ----------------------------------------------------------------------------

def _exact_x32(coeffs, y):
    """floor(32 x(y)) of the float coefficients, exactly"""
    a, b, c = (Fraction(v) for v in coeffs)
    return math.floor(32 * (a * y * y + b * y + c))


def test_area_is_ceil_to_floor_of_the_curves_on_integer_rows():
    """identity matrix: camera pixel (x, y) is the bird's-eye position (32 x, 32 y), so on row y layer 1 is the columns
    ceil(xl) .. floor(xr) of the float curves, to within the one 1/32-pixel step the Q32 rounding allows: its error
    (Y^2 + Y + 1) / 2^33 stays below one step for Y < 2^16"""
    h, w = 60, 90
    left, right = (0.004, -0.31, 24.3), (-0.002, 0.2, 61.77)
    t = np.zeros((1, 2, 8), dtype=np.int64)
    t[0, 0] = M.record(True, True, False, 5, 50, *LV.quantise(left))
    t[0, 1] = M.record(True, False, False, 0, 54, *LV.quantise(right))
    frames = LC.frames_of(1, 1, h, w)
    _, layers = M.lane_view(frames, np.eye(3), w, h, None, 127, t)
    assert set(np.unique(layers)) == {0, 1}
    assert not layers[0, :5].any() and not layers[0, 51:].any()                       # the rows both curves cover
    for y in range(5, 51):
        cols = np.flatnonzero(layers[0, y])
        fl, fr = _exact_x32(left, y), _exact_x32(right, y)
        assert -((-(fl - 1)) // 32) <= cols[0] <= -((-(fl + 1)) // 32), y            # ceil((fl -+ 1) / 32)
        assert (fr - 1) // 32 <= cols[-1] <= (fr + 1) // 32, y
        assert np.array_equal(cols, np.arange(cols[0], cols[-1] + 1))
        # and exactly the integers' own answer
        A, B, C_ = LV.quantise(left)
        xl = (A * (32 * y) ** 2 + B * 32 * y + C_) >> 32
        assert abs(xl - fl) <= 1 and cols[0] == -((-xl) // 32)


def test_crossing_curves_leave_the_crossed_rows_empty():
    h, w = 40, 64
    t = np.zeros((1, 2, 8), dtype=np.int64)
    t[0, 0] = M.record(True, True, False, 0, h - 1, *LV.quantise((0.0, 1.0, 10.0)))      # x = 10 + y
    t[0, 1] = M.record(True, False, False, 0, h - 1, *LV.quantise((0.0, -1.0, 50.5)))    # x = 50.5 - y: they cross at 20.25
    _, layers = M.lane_view(LC.frames_of(2, 1, h, w), np.eye(3), w, h, None, 127, t)
    for y in range(h):
        cols = np.flatnonzero(layers[0, y] == 1)
        if y <= 20:
            assert cols[0] == 10 + y and cols[-1] == 50 - y, y
        else:
            assert cols.size == 0, y
    assert set(np.unique(layers)) == {0, 1}


def test_default_blend_is_the_reference_overlay():
    """visualize_output: overlay[binary > 0] = [0, 255, 0]; addWeighted(img, 0.7, overlay, 0.3, 0), where overlay is
    the image itself elsewhere"""
    h, w = 16, 24
    frames = LC.frames_of(3, 1, h, w)
    masks = LC.masks_of(4, 1, w, h)
    view, layers = M.lane_view(frames, np.eye(3), w, h, masks, 127, None)
    assert np.array_equal(layers[0] == 2, masks[0] > 127) and set(np.unique(layers)) == {0, 2}
    overlay = frames[0].copy()
    overlay[masks[0] > 127] = (0, 255, 0)
    want = np.float32(0.7) * frames[0].astype(np.float32) + np.float32(0.3) * overlay.astype(np.float32)
    assert np.array_equal(view[0], np.clip(np.rint(want + np.float32(0.0)), 0, 255).astype(np.uint8))


# ---- the GPU test's inputs are a test of the definition ---------------------------------------------------------

MUTANTS = [dict(shift="trunc"), dict(priority="mask"), dict(horizon="ne"), dict(blend_all=False)]


def test_small_cases_reach_what_they_claim():
    for kind, matrix in LC.SMALL:
        case = LC.small(kind, matrix)
        h, w = case["frames"].shape[1:3]
        assert (case["step"] % 16 != 0) == (kind == "scalar") and (w % 16 != 0) == (kind == "scalar")
        _, layers = M.lane_view(case["frames"], case["m"], *case["warp"], case["masks"], 127, case["curves"], LC.LOUD)
        assert set(np.unique(layers[0])) == {0, 2}                                     # no curve
        assert set(np.unique(layers[1])) == {0, 2, 3}                                  # one curve
        assert {0, 1, 2, 3, 4} <= set(np.unique(layers[2])) and layers[2].max() == 4   # the outside curve is never seen
        valid, X, Y = M.positions(case["m"], w, h)
        if matrix == "horizon":
            assert (~valid).any() and valid.any() and not layers[:, ~valid].any()
            wrong, X2, Y2 = M.positions(case["m"], w, h, horizon="ne")
            above = wrong & ~valid
            assert (above & (X2 >= 0) & (X2 < 32 * 48) & (Y2 >= 0) & (Y2 < 32 * 40)).any()
        # rows that start and end inside the image: the curves of frame 2 stop short of both borders
        y0, y1 = (int(v) for v in case["curves"][2, 0, 1:3])
        assert 0 < y0 < y1 < case["warp"][1] - 1
        inside = valid & (X >= 0) & (Y >= 0) & (X < 32 * case["warp"][0]) & (Y < 32 * case["warp"][1])
        outside_rows = inside & ((Y < 32 * y0) | (Y > 32 * y1 + 31))
        assert outside_rows.any() and not np.isin(layers[2][outside_rows], (1, 3, 4)).any()


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: "-".join(f"{k}={v}" for k, v in m.items()))
def test_model_tells_mutants_apart(mutant):
    """`>> 32` replaced by a truncating division, the layer priority swapped, w > 0 replaced by w != 0, the blend
    skipped on layer-0 pixels: each changes a view or a layer plane of the small cases"""
    changed = []
    for kind, matrix in LC.SMALL:
        case = LC.small(kind, matrix)
        args = (case["frames"], case["m"], *case["warp"], case["masks"], 127, case["curves"], LC.LOUD)
        good, bad = M.lane_view(*args), M.lane_view(*args, **mutant)
        if not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])):
            changed.append((kind, matrix))
    assert changed, mutant
    if "horizon" in mutant:
        assert {m for _, m in changed} == {"horizon"}
    else:
        assert len(changed) >= 2
