"""Lane instances, host side: tests/label_model.py is held to scipy.ndimage (labels, count, areas, boxes, coordinate
sums) on every content and shape of tests/test_label_gpu.py; those contents tell the model's mutants apart; both entry
points are exported, prototyped and refuse everything outside their domain before a device is touched; and
`instances.Components`, `.fit`, `instances_of` and the confidence against the model's records and closed forms."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import ndimage

import label_model as M
import lanefit_model as LM
from unet_lane_detection_amd import _lib
from unet_lane_detection_amd import instances as I
from unet_lane_detection_amd import lanefit as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTURE = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the model against scipy -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w", M.SHAPES)
def test_model_against_scipy(n, h, w):
    """every case the GPU test runs for this shape (content, level, connectivity, cap), frame by frame"""
    yy, xx = np.mgrid[0:h, 0:w]
    for name, level, conn, cap in M.cases(n, h, w):
        masks = M.content(name, n, h, w)
        labels, header, records = M.reference(name, n, h, w, level, conn, cap)
        for i in range(n):
            on = masks[i].astype(np.int64) > level
            want, k = ndimage.label(on, structure=STRUCTURE[conn])
            what = (name, level, conn, cap, i)
            assert int(header[i, 0]) == k and int(header[i, 1]) == int(on.sum()) and int(header[i, 2]) == min(k, cap), what
            assert int(header[i, 3]) == 0
            assert np.array_equal(labels[i], want), what
            m = min(k, cap)
            assert not records[i, m:].any(), what
            if m == 0:
                continue
            idx = np.arange(1, m + 1)
            rec = records[i, :m].astype(np.int64)
            assert np.array_equal(rec[:, 0], ndimage.sum(on, want, idx).astype(np.int64)), what
            boxes = ndimage.find_objects(want)[:m]
            assert np.array_equal(rec[:, 1:5], np.array([[b[1].start, b[1].stop - 1, b[0].start, b[0].stop - 1] for b in boxes])), what
            assert np.array_equal(rec[:, 5], np.rint(ndimage.sum(xx, want, idx)).astype(np.int64)), what
            assert np.array_equal(rec[:, 6], np.rint(ndimage.sum(yy, want, idx)).astype(np.int64)), what
            # the words scipy has no function for, from the map itself
            assert np.array_equal(rec[:, 12], ndimage.minimum(yy * w + xx, want, idx).astype(np.int64)), what
            for c in (1, m, (m + 1) // 2):
                py, px = np.nonzero(want == c)
                py, px = py.astype(np.int64), px.astype(np.int64)        # 685^4 * 685 * 1055 < 2^58: int64 holds these
                sums = [int((py ** 2).sum()), int((py ** 3).sum()), int((py ** 4).sum()), int((px * py).sum()), int((px * py ** 2).sum())]
                assert [int(v) for v in records[i, c - 1, 7:12]] == sums, what
                flags = (py.min() == 0) * 1 + (py.max() == h - 1) * 2 + (px.min() == 0) * 4 + (px.max() == w - 1) * 8
                assert int(records[i, c - 1, 13]) == flags and not records[i, c - 1, 14:].any(), what


def test_counts_the_contents_are_there_for():
    n, h, w = 3, 37, 53
    hw = h * w

    def k(name, conn, level=127, i=0):
        return int(M.reference(name, n, h, w, level, conn, 1024)[1][i, 0])
    assert k("zeros", 8) == 0 and k("full", 4) == 1 and k("full", 8, 255) == 0
    assert k("checker", 4) == (hw + 1) // 2 > 7 and k("checker", 8) == 1
    assert k("serpentine", 4) == 1 and k("spiral", 4) == 1 and k("uw", 4) == 1
    assert k("diagonal", 8) == 1 and k("diagonal", 4) == min(h, w) and k("diagonal", 8, i=1) == 1
    assert k("rings", 4) == k("rings", 8) == (min(h, w) + 3) // 4
    # the records of a truncated frame: the map is complete, the header says K
    labels, header, records = M.reference("checker", n, h, w, 127, 4, 7)
    assert int(header[0, 0]) == (hw + 1) // 2 and int(header[0, 2]) == 7 and int(labels[0].max()) == (hw + 1) // 2
    # straddle: 127 is OFF and 128 ON at level 127
    s = M.content("straddle", n, h, w)
    assert set(np.unique(s).tolist()) == {126, 127, 128, 129}
    assert int(M.reference("straddle", n, h, w, 127, 8, 1024)[1][0, 1]) == int((s[0] >= 128).sum())


# ---- the contents discriminate ---------------------------------------------------------------------------------

def test_contents_tell_the_mutants_apart():
    """each mutant of the model differs from the model on at least one content of the GPU list, at a small shape"""
    n, h, w = 3, 37, 53

    def differs(names, conn, level=127, **mutant):
        hit = []
        for name in names:
            ref = M.reference(name, n, h, w, level, conn, 1024)
            got = M.label(M.content(name, n, h, w), level, conn, 1024, **mutant)
            if not all(np.array_equal(a, b) for a, b in zip(ref, got)):
                hit.append(name)
        return hit
    # 4-connectivity used for 8
    four = [name for name in M.CONTENTS
            if not np.array_equal(M.reference(name, n, h, w, 127, 8, 1024)[0], M.reference(name, n, h, w, 127, 4, 1024)[0])]
    assert {"checker", "diagonal", "random41"} <= set(four)
    assert {"random05", "random41", "painted"} <= set(differs(M.CONTENTS, 8, column_major=True))
    assert {"diagonal", "random41"} <= set(differs(M.CONTENTS, 8, drop_corner=True))
    assert differs(M.CONTENTS, 4, drop_corner=True) == []          # no diagonal links to drop
    assert "straddle" in differs(M.CONTENTS, 8, ge=True) and "painted" in differs(M.CONTENTS, 8, ge=True)
    # keep_largest: equal areas won by the higher id - the rings of `checker` with 4 are all of area 1
    labels, header, records = M.reference("checker", n, h, w, 127, 4, 1024)
    a = M.keep(labels, header, records, 1024, keep_largest=2)
    b = M.keep(labels, header, records, 1024, keep_largest=2, tie_high=True)
    assert a[0][0, :2].tolist() == [1, 1] and int(a[0][0].sum()) == 2 and not np.array_equal(a[0], b[0])
    assert not np.array_equal(a[1], b[1])


def test_keep_rule_of_the_model():
    mask = np.zeros((1, 12, 20), np.uint8)
    mask[0, 0, 0:3] = 255            # 1: area 3, 1 x 3
    mask[0, 2:8, 5] = 255            # 2: area 6, 6 x 1
    mask[0, 2:4, 8:11] = 255         # 3: area 6, 2 x 3
    mask[0, 10, 19] = 255            # 4: area 1
    labels, header, records = M.label(mask, 127, 8, 8)
    assert int(header[0, 0]) == 4 and [int(v) for v in records[0, :4, 0]] == [3, 6, 6, 1]

    def table(**kw):
        return M.keep(labels, header, records, 8, **kw)[0][0, :4].tolist()
    assert table() == [1, 1, 1, 1] and table(min_area=3) == [1, 1, 1, 0] and table(min_area=7) == [0, 0, 0, 0]
    assert table(min_height=2) == [0, 1, 1, 0] and table(min_width=3) == [1, 0, 1, 0]
    assert table(keep_largest=1) == [0, 1, 0, 0] and table(keep_largest=1, tie_high=True) == [0, 0, 1, 0]
    assert table(keep_largest=3) == [1, 1, 1, 0] and table(keep_largest=9) == [1, 1, 1, 1]
    assert table(keep_largest=1, min_width=2) == [0, 0, 1, 0]       # the order is among the components that pass
    t, m = M.keep(labels, header, records, 8, min_area=6)
    assert np.array_equal(m[0] == 255, (labels[0] == 2) | (labels[0] == 3)) and set(np.unique(m).tolist()) == {0, 255}
    # a component beyond the cap has no record and is never kept
    l1, h1, r1 = M.label(mask, 127, 8, 2)
    t, m = M.keep(l1, h1, r1, 2)
    assert t[0].tolist() == [1, 1] and np.array_equal(m[0] == 255, (l1[0] == 1) | (l1[0] == 2))


# ---- the entry points ------------------------------------------------------------------------------------------

def test_symbols_exported_and_prototyped(lib):
    for name in ("unet_label_work_bytes", "unet_label_u8_batch", "unet_keep_components_u8_batch"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "unet_hip.h")) as f:
        header = f.read()
    assert "#define UNET_LABEL_WORDS 16" in header and I.LABEL_WORDS == 16
    assert header.index("unet_lane_fit_u8_batch(int device") < header.index("unet_label_u8_batch(int device")
    section = header[header.index("lane instances on the device"):header.index("unet_label_u8_batch(int device")]
    assert "unpinned" in section and "14 739 386 724 520 034 304" in section and "never kept" in section
    from unet_lane_detection_amd.build import SOURCES
    assert "label_kernels.cpp" in SOURCES


def test_work_bytes(lib):
    f = lib.unet_label_work_bytes
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, 2049, 4), (1, 4, 2049), (512, 2048, 2048), (1 << 20, 2048, 2048)):
        assert f(*bad) == 0, bad
    assert f(1, 1, 1) > 0 and f(1, 2048, 2048) > 0 and f(511, 2048, 2048) > 0
    for n, h, w in ((1, 1, 1), (3, 37, 53), (2, 150, 200), (1, 685, 1055)):
        base = f(n, h, w)
        assert base > 0 and f(n + 1, h, w) >= base and f(n, h + 1, w) >= base and f(n, h, w + 1) >= base
    assert f(64, 685, 1055) >= f(1, 685, 1055)


def test_label_refuses_bad_arguments(lib):
    """null DEVICE pointers never get as far as a device; the host words behind the outputs stay clear"""
    name = b"unet_label_u8_batch"
    masks = C.cast((C.c_uint8 * 64)(), C.c_void_p)
    words = (C.c_uint64 * 256)()
    out = C.cast(words, C.c_void_p)

    def refused(rc, word):
        msg = lib.unet_op_last_error()
        return rc == 1 and msg.startswith(b"invalid argument") and name in msg and word in msg

    def go(masks=masks, n=2, h=4, w=8, level=127, conn=8, labels=out, cap=4, header=out, records=out, work=out,
           work_bytes=None, device=0):
        if work_bytes is None:
            work_bytes = max(lib.unet_label_work_bytes(n, h, w), 1)
        return lib.unet_label_u8_batch(device, masks, n, h, w, level, conn, labels, cap, header, records, work, work_bytes, None)
    for kw in (dict(masks=None), dict(labels=None), dict(header=None), dict(records=None), dict(work=None)):
        assert refused(go(**kw), b"null"), kw
    for n in (0, -1):
        assert refused(go(n=n), b"n must")
    for h in (0, -4, 2049):
        assert refused(go(h=h), b"height")
    for w in (0, -8, 2049):
        assert refused(go(w=w), b"width")
    assert refused(go(n=512, h=2048, w=2048), b"2^31")
    assert refused(go(n=1 << 20, h=2048, w=2048), b"2^31")
    for level in (-1, 256):
        assert refused(go(level=level), b"level")
    for conn in (6, 0, 5, -8):
        assert refused(go(conn=conn), b"connectivity")
    for cap in (0, -1, 65537):
        assert refused(go(cap=cap), b"max_components")
    assert refused(go(work_bytes=lib.unet_label_work_bytes(2, 4, 8) - 1), b"work_bytes")
    assert refused(go(work_bytes=0), b"work_bytes")
    odd = C.c_void_p(out.value + 2)
    assert refused(go(labels=odd), b"aligned") and refused(go(records=C.c_void_p(out.value + 4)), b"aligned")
    assert not any(words)
    bad = 1 << 20        # what passes the checks goes on to the device: an ordinal the runtime refuses shows it got there
    for kw in (dict(), dict(conn=4), dict(n=1, h=2048, w=2048, cap=65536, level=255), dict(n=1, h=1, w=1, cap=1, level=0),
               dict(n=511, h=2048, w=2048), dict(masks=C.c_void_p(masks.value + 1))):
        assert go(device=bad, **kw) == _lib.UNET_ERR_HIP, kw
        assert b"hipSetDevice" in lib.unet_op_last_error()
    assert not any(words)


def test_keep_refuses_bad_arguments(lib):
    name = b"unet_keep_components_u8_batch"
    words = (C.c_uint64 * 256)()
    buf = C.cast(words, C.c_void_p)

    def refused(rc, word):
        msg = lib.unet_op_last_error()
        return rc == 1 and msg.startswith(b"invalid argument") and name in msg and word in msg

    def go(labels=buf, n=2, h=4, w=8, header=buf, records=buf, cap=4, min_area=0, min_height=0, min_width=0,
           keep_largest=0, keep=buf, mask=buf, device=0):
        return lib.unet_keep_components_u8_batch(device, labels, n, h, w, header, records, cap, min_area, min_height,
                                                 min_width, keep_largest, keep, mask, None)
    for kw in (dict(labels=None), dict(header=None), dict(records=None), dict(keep=None), dict(mask=None)):
        assert refused(go(**kw), b"null"), kw
    assert refused(go(n=0), b"n must") and refused(go(h=2049), b"height") and refused(go(w=2049), b"width")
    assert refused(go(h=0), b"height") and refused(go(w=0), b"width")
    assert refused(go(n=512, h=2048, w=2048), b"2^31")
    for cap in (0, 65537):
        assert refused(go(cap=cap), b"max_components")
    assert refused(go(min_area=-1), b"min_area") and refused(go(min_height=-1), b"min_height")
    assert refused(go(min_width=-1), b"min_width") and refused(go(keep_largest=-1), b"keep_largest")
    assert not any(words)
    for kw in (dict(), dict(min_area=1 << 30, keep_largest=(1 << 31) - 1), dict(n=1, h=2048, w=2048, cap=65536)):
        assert go(device=1 << 20, **kw) == _lib.UNET_ERR_HIP, kw
        assert b"hipSetDevice" in lib.unet_op_last_error()
    assert not any(words)


# ---- the host layer --------------------------------------------------------------------------------------------

def test_largest_sum_fits_64_bits():
    rec = M.full_frame_record(2048, 2048)
    assert rec[9] == 2048 * sum(y ** 4 for y in range(2048)) == 14739386724520034304 < 1 << 64
    assert rec[9] == 2 * 7369693362260017152                      # twice the lane fit's bound
    assert rec[11] < 1 << 54 and max(rec) == rec[9]
    # the closed form is the model's record on a frame the model can run
    labels, header, records = M.label(np.full((1, 9, 14), 255, np.uint8), 127, 4, 3)
    assert [int(v) for v in records[0, 0]] == M.full_frame_record(9, 14) and int(header[0, 0]) == 1


def test_components_and_fit_from_the_models_records():
    n, h, w = 3, 37, 53
    masks = M.content("painted", n, h, w)
    labels, header, records = M.reference("painted", n, h, w, 127, 8, 1024)
    comp = I.Components(None, header, records, h, w)
    assert len(comp) == n and comp.count == [int(v) for v in header[:, 0]]
    assert comp.on_pixels == [int((m > 127).sum()) for m in masks] and comp.truncated == [False] * n
    for i in range(n):
        k = comp.count[i]
        assert comp.recorded(i) == k and comp.area[i].shape == (k,) and comp.bbox[i].shape == (k, 4)
        for c in (1, k, (k + 1) // 2):
            py, px = np.nonzero(labels[i] == c)
            assert comp.area[i][c - 1] == len(py)
            assert comp.bbox[i][c - 1].tolist() == [px.min(), px.max(), py.min(), py.max()]
            assert comp.centroid[i][c - 1] == (int(px.sum()) / len(px), int(py.sum()) / len(py))
            assert comp.first_pixel[i][c - 1].tolist() == [py[0], px[0]]
            flags = (py.min() == 0) * 1 + (py.max() == h - 1) * 2 + (px.min() == 0) * 4 + (px.max() == w - 1) * 8
            assert comp.touches[i][c - 1] == flags
            fit = comp.fit(i, c)
            S = [int(sum(int(y) ** p for y in py)) for p in range(5)]
            T = [int(sum(int(x) * int(y) ** p for x, y in zip(px, py))) for p in range(3)]
            assert fit.S == tuple(S) and fit.T == tuple(T) and fit.pixels == len(py)
            assert fit.coeffs == LM.solve(S, T) == LF.solve(S, T)
            assert fit.y_range == (py.min(), py.max()) and fit.present
    with pytest.raises(IndexError):
        comp.fit(0, comp.count[0] + 1)
    with pytest.raises(IndexError):
        comp.fit(0, 0)
    # min_fit_pixels: a one-pixel component has no coefficients with the default 3, a constant with 1
    one = int(np.flatnonzero(comp.area[0] == 1)[0]) + 1
    assert comp.fit(0, one).coeffs is None
    assert comp.fit(0, one, LF.FitConfig(min_fit_pixels=1)).coeffs == (0.0, 0.0, float(comp.bbox[0][one - 1][0]))
    # truncated: K > cap
    t = I.Components(None, *M.reference("checker", n, h, w, 127, 4, 7)[1:], h, w)
    assert t.truncated == [True] * n and t.recorded(0) == 7 and t.count[0] == (h * w + 1) // 2


def test_lane_instances_sorting_and_confidence():
    n, h, w = 2, 150, 200
    labels, header, records = M.reference("painted", n, h, w, 127, 8, 1024)
    comp = I.Components(None, header, records, h, w)
    keep, mask = M.keep(labels, header, records, 1024, min_area=64)
    frames = I.instances_of(comp, keep)
    assert len(frames) == n
    for i, frame in enumerate(frames):
        assert len(frame) == 3 == int(keep[i].sum())                  # three markings; the speckle is gone
        xs = [s.x_at(h - 1) for s in frame]
        assert xs == sorted(xs) and all(s.fit.coeffs is not None for s in frame)
        for s, base in zip(frame, (0.15, 0.45, 0.75)):
            assert abs(s.x_at(h - 1) - base * w) < 0.04 * w
            assert s.area == int(records[i, s.id - 1, 0]) and s.frame == i and keep[i, s.id - 1] == 1
            assert s.bbox == tuple(int(v) for v in records[i, s.id - 1, 1:5])
        largest = max(s.area for s in frame)
        assert [s.confidence for s in frame] == [s.area / largest for s in frame] and max(s.confidence for s in frame) == 1.0
        # another reference row, another order is possible; the key is x_at(y_ref)
        top = I.instances_of(comp, keep, y_ref=0)[i]
        assert [s.x_at(0) for s in top] == sorted(s.x_at(0) for s in top)
    # without the filter the speckle is there, and the model's mask shows what the filter removes
    assert all(len(f) > 3 for f in I.instances_of(comp, np.ones_like(keep)))
    assert int((mask[0] == 255).sum()) == sum(s.area for s in frames[0]) < int(header[0, 1])
    assert I.CleanConfig() == I.CleanConfig(64, 0, 0, 0, 127, 8, 1024)
