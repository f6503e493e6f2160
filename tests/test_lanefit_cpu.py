"""The lane fit's host side: the entry point is exported, prototyped and refuses everything outside its domain before
a device is touched; `lanefit.solve`, `prior_table`, the curvature and heading formulas and `LaneTracker` against
tests/lanefit_model.py and closed forms; and the inputs of tests/test_lanefit_gpu.py are a test of the definition -
each of the model's two mutants changes a record on them."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import follow_model as FM
import lanefit_model as LM
from unet_lane_detection_amd import _lib
from unet_lane_detection_amd import lanefit as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = (1 << 31) - 1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the entry point -------------------------------------------------------------------------------------------

def test_symbol_exported_and_prototyped(lib):
    assert hasattr(lib, "unet_lane_fit_u8_batch") and "unet_lane_fit_u8_batch" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "unet_hip.h")) as f:
        header = f.read()
    assert "int unet_lane_fit_u8_batch(int device, const uint8_t* masks_dev, int n, int height, int width, int level," in header
    assert "#define UNET_LANE_FIT_WORDS 16" in header and "#define UNET_LANE_FIT_WINDOWS_MAX 64" in header
    assert "unpinned" in header[header.index("lane fit on the device"):header.index("unet_lane_fit_u8_batch(int device")]
    assert header.index("unet_lane_center_u8_batch(int device") < header.index("unet_lane_fit_u8_batch(int device")
    assert LF.FIT_WORDS == 16 and LF.FIT_WINDOWS_MAX == 64
    from unet_lane_detection_amd.build import SOURCES
    assert "lanefit_kernels.cpp" in SOURCES


def test_lane_fit_refuses_bad_arguments(lib):
    """null DEVICE pointers throughout: a call that got past the checks would have to touch a device to go wrong, and
    the host words behind `out` stay clear"""
    call = lib.unet_lane_fit_u8_batch
    name = b"unet_lane_fit_u8_batch"
    masks = C.cast((C.c_uint8 * 64)(), C.c_void_p)
    out_words = (C.c_uint64 * 64)()
    out = C.cast(out_words, C.c_void_p)
    prior = C.cast((C.c_int32 * 64)(), C.c_void_p)

    def refused(rc, word):
        msg = lib.unet_op_last_error()
        return rc == 1 and msg.startswith(b"invalid argument") and name in msg and word in msg

    def go(masks=masks, n=2, h=4, w=8, level=127, nw=2, margin=3, minpix=0, prior=None, out=out, device=0):
        return call(device, masks, n, h, w, level, nw, margin, minpix, prior, out, None)
    assert refused(go(masks=None), b"null")
    assert refused(go(out=None), b"null")
    assert refused(go(masks=None, prior=prior), b"null")
    for n in (0, -1):
        assert refused(go(n=n), b"n must")
    for h in (0, -4, 2049):
        assert refused(go(h=h, nw=1), b"height")
    for w in (0, -8, 8193):
        assert refused(go(w=w), b"width")
    assert refused(go(n=128, h=2048, w=8192, nw=1), b"2^31")                 # exactly 2^31 pixels
    assert refused(go(n=1 << 20, h=2048, w=8192, nw=1), b"2^31")             # a product that overflows 32 bits
    for level in (-1, 256):
        assert refused(go(level=level), b"level")
    for nw in (0, -1, 5, 65):                                                 # 5 > height = 4
        assert refused(go(nw=nw), b"n_windows")
    assert refused(go(h=100, nw=65), b"n_windows")
    for margin in (0, -1, 513):
        assert refused(go(margin=margin), b"margin")
    assert refused(go(minpix=-1), b"min_pixels")
    assert not any(out_words)
    # what passes the checks goes on to the device: an ordinal the runtime refuses shows it got that far
    bad = 1 << 20
    for kw in (dict(), dict(prior=prior), dict(n=1, h=2048, w=8192, nw=64, margin=512, level=255, minpix=INT_MAX),
               dict(n=1, h=1, w=1, nw=1, margin=1, level=0), dict(n=127, h=2048, w=8192, nw=1), dict(h=4, nw=4)):
        assert go(device=bad, **kw) == _lib.UNET_ERR_HIP, kw
        assert b"hipSetDevice" in lib.unet_op_last_error()
    assert not any(out_words)


# ---- the solve -------------------------------------------------------------------------------------------------

def _sums(points):
    S = [sum(y ** k for _, y in points) for k in range(5)]
    T = [sum(x * y ** k for x, y in points) for k in range(3)]
    return S, T


def test_solve_is_exact_on_a_parabola():
    S, T = _sums([(3 + 2 * y + y * y, y) for y in range(12)])
    assert LF.solve(S, T) == (1.0, 2.0, 3.0)
    assert LM.solve(S, T) == (1.0, 2.0, 3.0)
    assert LM.solve_exact(S, T) == (Fraction(1), Fraction(2), Fraction(3))


def test_exact_solution_satisfies_the_normal_equations_and_solve_rounds_it_once():
    rng = np.random.default_rng(3)
    for trial in range(20):
        h = int(rng.integers(3, 2048))
        pts = [(int(rng.integers(0, 8192)), int(y)) for y in rng.integers(0, h, int(rng.integers(3, 400)))]
        if len({y for _, y in pts}) < 3:
            continue
        S, T = _sums(pts)
        a, b, c = LM.solve_exact(S, T)
        assert S[4] * a + S[3] * b + S[2] * c == T[2]
        assert S[3] * a + S[2] * b + S[1] * c == T[1]
        assert S[2] * a + S[1] * b + S[0] * c == T[0]
        assert LF.solve(S, T) == (float(a), float(b), float(c)) == LM.solve(S, T)
    # the largest sums the device can deliver: every pixel of a 2048-row, 1024-column band
    S = [1024 * sum(y ** k for y in range(2048)) for k in range(5)]
    T = [sum(range(7168, 8192)) * sum(y ** k for y in range(2048)) for k in range(3)]
    assert S[4] < 1 << 64 and T[2] < 1 << 64 and S[4] / 2 ** 64 > 0.39
    assert LF.solve(S, T) == LM.solve(S, T) == (0.0, 0.0, 7679.5)


def test_fallbacks_and_min_fit_pixels():
    two_rows = [(10, 5), (12, 5), (20, 9), (22, 9), (24, 9)]            # two distinct rows: the exact line
    S, T = _sums(two_rows)
    got = LF.solve(S, T)
    assert got == LM.solve(S, T) and got[0] == 0.0
    q = LM.solve_exact(S, T)
    assert q[0] == 0 and q[1] * 5 + q[2] == 11 and q[1] * 9 + q[2] == 22
    one_row = [(10, 7), (13, 7), (19, 7)]                               # one row: the constant mean
    S, T = _sums(one_row)
    assert LF.solve(S, T) == LM.solve(S, T) == (0.0, 0.0, 14.0)
    assert LF.solve(*_sums([(1, 0), (2, 0), (4, 0)])) == (0.0, 0.0, 7 / 3)      # y = 0 only
    S, T = _sums([(5, 1), (6, 2)])
    assert LF.solve(S, T) is None and LM.solve(S, T) is None            # 2 < min_fit_pixels = 3
    assert LF.solve(S, T, min_fit_pixels=2) == LM.solve(S, T, 2) == (0.0, 1.0, 4.0)
    assert LF.solve([0] * 5, [0] * 3, min_fit_pixels=0) is None         # no pixels, whatever the limit
    S, T = _sums([(3 + y * y, y) for y in range(3)])
    assert LF.solve(S, T, min_fit_pixels=3) == (1.0, 0.0, 3.0) and LF.solve(S, T, min_fit_pixels=4) is None


# ---- what is read off a fit ------------------------------------------------------------------------------------

def _lane_words(points, height, hit=3, tried=4, flags=1):
    S, T = _sums(points)
    ys = [y for _, y in points]
    return [flags, 0, hit, tried, 0] + S + T + [min(ys) if ys else height, max(ys) if ys else 0, 0]


def test_formulas_against_closed_forms():
    left = _lane_words([(3 + 2 * y + y * y, y) for y in range(12)], 50)
    right = _lane_words([(40 + y, y) for y in range(0, 12, 2)], 50, hit=1, tried=2)
    fits = LF.LaneFits.from_records(np.array([[left, right]], dtype=np.uint64), 50, 101, LF.FitConfig())
    assert len(fits) == 1
    f = fits[0]
    assert f.left.coeffs == (1.0, 2.0, 3.0) and f.right.coeffs == (0.0, 1.0, 40.0)
    assert f.left.present and f.left.pixels == 12 and f.left.y_range == (0, 11) and f.left.confidence == 0.75
    assert f.right.confidence == 0.5 and f.right.pixels == 6 and f.right.y_range == (0, 10)
    for y in (0, 3, 10.5, 49):
        assert f.left.x_at(y) == y * y + 2 * y + 3 == LM.x_at(f.left.coeffs, y)
        assert math.isclose(f.left.heading(y), math.atan(2 * y + 2), rel_tol=1e-12)
        assert f.right.heading(y) == math.atan(1.0)
        assert math.isclose(f.left.curvature_radius(y), (1 + (2 * y + 2) ** 2) ** 1.5 / 2, rel_tol=1e-12)
        assert f.left.curvature_radius(y) == LM.radius(f.left.coeffs, y)
        assert f.right.curvature_radius(y) == math.inf
        assert f.center_at(y) == (f.left.x_at(y) + f.right.x_at(y)) / 2
        assert f.center_px(y) == int(math.floor(f.center_at(y)))
        assert f.lane_width(y) == f.right.x_at(y) - f.left.x_at(y)
        assert f.offset(y) == f.center_at(y) - 50
    # a circle of radius 500 around (x, y) = (600, 40): x = 600 - sqrt(500^2 - (y - 40)^2); its osculating parabola at
    # y = 40 is x = 100 + (y - 40)^2 / 1000, whose radius of curvature there is the circle's
    a, b, c = 1 / 1000, -80 / 1000, 100 + 1600 / 1000
    assert math.isclose(LM.radius((a, b, c), 40), 500.0, rel_tol=1e-12)
    lane = fits[0].left
    lane.coeffs = (a, b, c)
    assert math.isclose(lane.curvature_radius(40), 500.0, rel_tol=1e-12)
    assert math.isclose(lane.heading(40), 0.0, abs_tol=1e-15)
    # metres: A = a xm / ym^2, B = b xm / ym at y ym
    cfg = LF.FitConfig(xm_per_pix=3.7 / 700, ym_per_pix=30 / 720)
    m = LF.LaneFits.from_records(np.array([[left, right]], dtype=np.uint64), 50, 101, cfg)[0].left
    xm, ym = cfg.xm_per_pix, cfg.ym_per_pix
    A, B = 1.0 * xm / ym ** 2, 2.0 * xm / ym
    for y in (0, 7, 49):
        want = (1 + (2 * A * y * ym + B) ** 2) ** 1.5 / abs(2 * A)
        assert math.isclose(m.curvature_radius(y), want, rel_tol=1e-12)
        assert m.curvature_radius(y) == LM.radius(m.coeffs, y, xm, ym)
    # a lane without coefficients: nothing is made up
    empty = _lane_words([], 50, hit=0, tried=0, flags=0)
    f = LF.LaneFits.from_records(np.array([[left, empty]], dtype=np.uint64), 50, 101)[0]
    assert f.right.coeffs is None and not f.right.present and f.right.confidence == 0.0 and f.right.y_range is None
    assert f.right.x_at(3) is None and f.right.heading(3) is None and f.right.curvature_radius(3) is None
    assert f.center_at(3) is None and f.center_px(3) is None and f.lane_width(3) is None and f.offset(3) is None


def test_prior_table_rounding():
    h = 16
    half = _lane_words([(2 * y + 1, 2 * y) for y in range(8)] + [(2 * y + 2, 2 * y) for y in range(8)], h)   # x = y + 1.5
    far = _lane_words([(8000, y) for y in range(4)], h)
    rec = np.array([[half, far], [_lane_words([], h, 0, 0, 0), half]], dtype=np.uint64)
    fits = LF.LaneFits.from_records(rec, h, 8192)
    assert fits[0].left.coeffs == (0.0, 1.0, 1.5)
    table = LF.prior_table(fits, h)
    assert table.dtype == np.int32 and table.shape == (2, 2, h)
    assert table[0, 0].tolist() == [y + 2 for y in range(h)]             # floor(y + 1.5 + 0.5): halves round up
    assert (table[0, 1] == 8000).all() and (table[1, 0] == -1).all()
    assert np.array_equal(table, LM.prior_table(rec, h))
    # negative halves: floor(-2.5 + 0.5) = -2; and the clip to int32 on both sides
    lane = fits[0].left
    lane.coeffs = (0.0, -1.0, 0.5)
    assert LF.prior_table(fits, h)[0, 0, :4].tolist() == [1, 0, -1, -2]
    lane.coeffs = (1e12, 0.0, -1e12)
    got = LF.prior_table(fits, h)[0, 0]
    assert got[0] == -(1 << 31) and got[1] == 0 and got[2] == INT_MAX and got[-1] == INT_MAX


# ---- the inputs of the GPU test are a test of the definition ---------------------------------------------------

def test_crafted_windows_tell_both_mutants_apart():
    mask, kw = LM.crafted()
    ref = LM.records(mask, **kw)
    left, right = ref[0]
    # window 0 holds exactly min_pixels pixels and does not recentre; window 4 holds min_pixels + 1 and does
    assert int(left[1]) == 3 and int(left[2]) == 1 and int(left[4]) == 5 and int(left[3]) == 8
    assert int(left[5]) == 5 + 6 + 2                                      # the pixel at x == c + margin = 11 is outside
    assert int(right[1]) == 62 and int(right[2]) == 0 and int(right[5]) == 4
    on = mask[0] > kw["level"]
    assert int(on[35:40].sum() - on[35:40, 32:].sum()) == kw["min_pixels"]
    assert int(on[15:20, :32].sum()) == kw["min_pixels"] + 1
    assert on[12, 5 + kw["margin"]]
    # the windows are clipped at both borders: base - margin < 0 on the left, base + margin > width on the right
    assert int(left[1]) - kw["margin"] < 0 and int(right[1]) + kw["margin"] > mask.shape[2]
    closed = LM.records(mask, closed_upper=True, **kw)
    assert int(closed[0, 0, 5]) == int(left[5]) + 1 and not np.array_equal(closed, ref)
    ge = LM.records(mask, recentre_ge=True, **kw)
    assert int(ge[0, 0, 2]) == 2 and not np.array_equal(ge, ref)
    # ... and in prior mode the closed bound shows on a table through the same pixel
    table = np.full((1, 2, 40), -1, dtype=np.int32)
    table[0, 0, 12] = 5
    a, b = LM.records(mask, prior=table, **kw), LM.records(mask, prior=table, closed_upper=True, **kw)
    assert int(a[0, 0, 5]) == 0 and int(b[0, 0, 5]) == 1 and int(a[0, 0, 3]) == 1 and int(a[0, 0, 2]) == 0


@pytest.mark.parametrize("n,h,w,margin", [(2, 90, 131, 6), (2, 685, 1055, 100)])
def test_painted_frames_find_both_lanes_and_an_absent_one(n, h, w, margin):
    """The frames of tests/test_lanefit_gpu.py (same generator, same seeds).  On the 90 x 131 frame a scan row in a gap
    of the dashed left marking has no centre (`lane_centers` gives None) while `center_px` is an integer there.  On
    the 685 x 1055 frame the right marking alone is 21 pixels wide, more than LineFollower's 10, so such a row does
    get a centre - a wrong one, pulled to the right marking; that is what is asserted there."""
    masks = LM.painted_lanes(LM.painted_seed(n, h, w), n, h, w)
    values = set(np.unique(masks).tolist())
    assert {127, 128} <= values and {0, 255} <= values                   # both sides of the level, and the level itself
    flipped = float((masks[0] > 127).mean())
    assert 0.01 < flipped < 0.08
    cfg = LF.FitConfig(margin=margin, min_pixels=max(2, margin // 2))
    rec = LM.records(masks, cfg.level, cfg.n_windows, cfg.margin, cfg.min_pixels)
    fits = LF.LaneFits.from_records(rec, h, w, cfg)
    f = fits[0]
    assert f.left.present and f.right.present and f.left.coeffs is not None and f.right.coeffs is not None
    for lane in f.lanes:
        assert lane.coeffs == LM.coeffs_of(lane.words)
        assert lane.confidence == LM.confidence(lane.words)
    # the fit follows the painted markings: at the bottom row the lanes are near 0.22 w and 0.70 w
    assert abs(f.left.x_at(h - 1) - 0.22 * w) < 0.06 * w and abs(f.right.x_at(h - 1) - 0.70 * w) < 0.06 * w
    assert 0.35 * w < f.lane_width(h - 1) < 0.6 * w
    # the last frame has an empty half: that lane is absent, with the record of an absent lane
    last = fits[n - 1]
    gone = last.right if LM.painted_seed(n, h, w) % 2 == 0 else last.left
    assert not gone.present and gone.coeffs is None
    assert gone.words == [0] * 13 + [h, 0, 0]
    assert last.center_px(h // 2) is None
    # the closed upper bound changes a record on these very frames
    assert not np.array_equal(LM.records(masks, cfg.level, cfg.n_windows, cfg.margin, cfg.min_pixels, closed_upper=True), rec)
    # a dashed marking: some scan row falls into a gap and has no centre, while the fit still has one there
    rows = list(range(h // 2, h))
    centres = FM.lane_centers(masks[:1], rows)[0]
    holes = [r for r, c in zip(rows, centres) if c is None]
    assert all(isinstance(f.center_px(r), int) for r in rows)
    if w < 500:
        assert holes         # fewer than 11 pixels on a gap's row: LineFollower.update does nothing for that frame
    else:
        # the wide frame's right marking alone passes the "more than 10 pixels" rule, so a gap's row does get a centre:
        # one pulled towards the right marking, while the fit's centre stays between the lanes
        pulled = [r for r, c in zip(rows, centres) if c is not None and c - f.center_at(r) > 0.05 * w]
        print(f"({h},{w}): {len(holes)} rows without a centre, {len(pulled)} rows pulled to the right by more than {0.05 * w:.0f} px")
        assert any((r // max(2, h // 12)) % 2 == 1 for r in pulled)      # rows of a gap among them


def test_tracker_mode_sequence_on_a_fake_source():
    h, w = 50, 101
    good = [_lane_words([(3 + 2 * y + y * y, y) for y in range(12)], h, hit=4, tried=4),
            _lane_words([(40 + y, y) for y in range(12)], h, hit=2, tried=4)]
    weak = [good[0], _lane_words([(40 + y, y) for y in range(12)], h, hit=1, tried=4)]       # confidence 0.25
    lost = [good[0], _lane_words([], h, hit=0, tried=0, flags=0)]
    few = [good[0], _lane_words([(40, 3), (41, 4)], h, hit=4, tried=4)]                       # 2 pixels: no coefficients
    script = [good, good, weak, good, lost, good, few, good, good]
    calls = []

    def source(mask, cfg, prior):
        calls.append(None if prior is None else np.array(prior))
        return np.array([script[len(calls) - 1]], dtype=np.uint64)
    tracker = LF.LaneTracker(LF.FitConfig(), min_confidence=0.5, source=source)
    mask = np.zeros((h, w), dtype=np.uint8)
    for _ in script:
        fits = tracker.update(mask)
        assert len(fits) == 1
    assert tracker.modes == ["window", "prior", "prior", "window", "prior", "window", "prior", "window", "prior"]
    assert tracker.mode == "prior"
    for mode, prior in zip(tracker.modes, calls):
        assert (prior is None) == (mode == "window")
    # the table handed to prior mode is the model's table of the last records
    want = LM.prior_table(np.array([good], dtype=np.uint64), h)
    assert calls[1].dtype == np.int32 and np.array_equal(calls[1], want)
    assert calls[1][0, 0, :3].tolist() == [3, 6, 11] and calls[1][0, 1, :3].tolist() == [40, 41, 42]
    tracker.reset()
    script.append(good)
    tracker.update(mask)
    assert tracker.mode == "window"
