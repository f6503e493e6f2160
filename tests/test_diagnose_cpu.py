"""The diagnostics' host side: the two entry points are exported and refuse bad arguments before a device is touched,
tests/diagnose_model.py and the host formulas of unet_lane_detection_amd/diagnose.py agree with numpy's own mean and
variance, hand-made frames and probabilities give the records worked out by hand, and the frames of
tests/test_diagnose_gpu.py are a test of the rule: a look-alike with another border, with the padding counted, with R
and B exchanged or with a 32-bit sum of squares gives another record on them."""
import ctypes as C

import numpy as np
import pytest

import diagnose_model as DM
from unet_lane_detection_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the entry points ------------------------------------------------------------------------------------------

NAMES = ("unet_frame_stats_u8_batch", "unet_prob_stats_f32_batch")


def test_symbols_exported(lib):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", open(os.path.join(root, "include", "unet_hip.h")).read()))
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in declared     # tests/test_abi_cpu.py's parse


def _refused(lib, rc, call):
    msg = lib.unet_op_last_error()
    return rc == 1 and msg.startswith(b"invalid argument") and call in msg


def test_frame_stats_refuses_bad_arguments(lib):
    call = lib.unet_frame_stats_u8_batch
    name = b"unet_frame_stats_u8_batch"
    frames = C.cast((C.c_uint8 * (2 * 4 * 16))(), C.c_void_p)
    out_words = (C.c_uint64 * (2 * 8 + 1))()
    out = C.cast(out_words, C.c_void_p)
    assert _refused(lib, call(0, None, 2, 4, 4, 0, 1, out, None), name)                  # null pointers
    assert _refused(lib, call(0, frames, 2, 4, 4, 0, 1, None, None), name)
    for n, h, w in ((0, 4, 4), (-1, 4, 4), (2, 0, 4), (2, -4, 4), (2, 4, 0), (2, 4, -1)):   # non-positive sizes
        assert _refused(lib, call(0, frames, n, h, w, 0, 1, out, None), name), (n, h, w)
    for stride in (11, 1, -12):                                                          # row_stride < 3 * width
        assert _refused(lib, call(0, frames, 2, 4, 4, stride, 1, out, None), name), stride
        assert b"row_stride" in lib.unet_op_last_error()
    assert _refused(lib, call(0, frames, 2, 1 << 15, 1 << 15, 0, 1, out, None), name)    # 2^31 pixels
    assert b"2^31" in lib.unet_op_last_error()
    assert _refused(lib, call(0, frames, 1 << 11, 1 << 10, 1 << 10, 0, 1, out, None), name)
    assert _refused(lib, call(0, frames, 2, 4, 4, 0, 1, C.c_void_p(C.addressof(out_words) + 4), None), name)
    assert b"aligned" in lib.unet_op_last_error()
    assert not any(out_words)
    # what passes the checks goes on to the device: an ordinal the runtime refuses shows it got that far
    for stride, bgr in ((0, 1), (12, 0), (16, 1)):
        assert call(1 << 20, frames, 2, 4, 4, stride, bgr, out, None) == _lib.UNET_ERR_HIP
        assert b"hipSetDevice" in lib.unet_op_last_error()
    assert not any(out_words)


def test_prob_stats_refuses_bad_arguments(lib):
    call = lib.unet_prob_stats_f32_batch
    name = b"unet_prob_stats_f32_batch"
    scores = C.cast((C.c_float * 32)(), C.c_void_p)
    out_words = (C.c_uint64 * (2 * 4 + 1))()
    out = C.cast(out_words, C.c_void_p)
    assert _refused(lib, call(0, None, 2, 16, 0.5, out, None), name)                     # null pointers
    assert _refused(lib, call(0, scores, 2, 16, 0.5, None, None), name)
    assert _refused(lib, call(0, scores, 0, 16, 0.5, out, None), name)                   # non-positive sizes
    assert _refused(lib, call(0, scores, -2, 16, 0.5, out, None), name)
    assert _refused(lib, call(0, scores, 2, 0, 0.5, out, None), name)
    for numel in (1 << 31, (1 << 31) + 1, 1 << 40):                                      # numel_per_frame >= 2^31
        assert _refused(lib, call(0, scores, 1, numel, 0.5, out, None), name), numel
        assert b"2^31" in lib.unet_op_last_error()
    assert _refused(lib, call(0, scores, 2, 16, float("nan"), out, None), name)          # a NaN threshold
    assert b"threshold" in lib.unet_op_last_error()
    assert _refused(lib, call(0, scores, 2, 16, 0.5, C.c_void_p(C.addressof(out_words) + 4), None), name)
    assert not any(out_words)
    for numel, thr in ((16, 0.5), (1, float("inf")), ((1 << 31) - 1, float("-inf"))):
        assert call(1 << 20, scores, 1, numel, thr, out, None) == _lib.UNET_ERR_HIP
        assert b"hipSetDevice" in lib.unet_op_last_error()
    assert not any(out_words)


# ---- the model and the host formulas against numpy ------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(5, 7), (67, 131), (1, 9), (9, 1), (2, 2)])
def test_model_mean_and_sharpness_are_numpys(h, w):
    from unet_lane_detection_amd.diagnose import FrameStats
    rng = np.random.default_rng(100 * h + w)
    frames = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    rec = DM.frame_records(frames)
    stats = FrameStats(rec, h, w)
    for i, img in enumerate(frames):
        lap = DM.laplacian(DM.gray(img))
        if h > 2 and w > 2:     # cv2's border spelled the way numpy pads: the two statements of reflect-101 agree
            y = np.pad(DM.gray(img), 1, mode="reflect")
            assert np.array_equal(lap, y[:-2, 1:-1] + y[2:, 1:-1] + y[1:-1, :-2] + y[1:-1, 2:] - 4 * y[1:-1, 1:-1])
        var, mean = float(lap.astype(np.float64).var()), float(img.mean())
        got_var, got_mean = DM.frame_sharpness(rec[i], h, w), DM.frame_mean(rec[i], h, w)
        print(f"{h}x{w} frame {i}: variance {got_var!r} against {var!r}, mean {got_mean!r} against {mean!r}")
        assert abs(got_var - var) <= 1e-12 * var
        assert abs(got_mean - mean) <= 1e-12 * mean
        assert stats.sharpness[i] == got_var and stats.mean[i] == got_mean     # the package's formulas are the model's
        assert (stats.min[i], stats.max[i]) == (int(img.min()), int(img.max()))


def test_hand_made_frames():
    from unet_lane_detection_amd.diagnose import FrameStats
    const = np.full((1, 6, 9, 3), 77, dtype=np.uint8)
    rec = DM.frame_records(const)
    assert rec[0].tolist() == [77, 77, 77 * 6 * 9 * 3, 0, 0, 0, 0, 0]
    st = FrameStats(rec, 6, 9)
    assert st.sharpness[0] == 0.0 and st.blurry[0] and not st.too_dark[0] and not st.overexposed[0]
    assert "warning: the image may be blurred" in st.report(0)
    # a 0 / 255 checkerboard: reflect-101 keeps the parity, so every neighbour of a pixel - the reflected ones too - is
    # of the other colour and L = +-1020 at every pixel, borders included
    for h, w in ((256, 256), (5, 8), (7, 7)):
        board = DM.checkerboard(h, w)
        assert set(np.unique(DM.laplacian(DM.gray(board[0]))).tolist()) == {-1020, 1020}
        rec = DM.frame_records(board)[0]
        n = h * w
        assert int(rec[4]) == n * 1020 * 1020
        assert DM.frame_s1(rec) == 1020 * (n % 2)      # +1020 on the dark pixels, -1020 on the bright ones
        st = FrameStats(rec[None], h, w)
        assert not st.blurry[0] and (st.min[0], st.max[0]) == (0, 255)
    assert DM.frame_records(DM.checkerboard(256, 256), border="replicate")[0, 4] != 256 * 256 * 1020 * 1020
    # brightness on either side of the reference's limits: 30 bytes whose sums are 1497, 1500, 6000 and 6003
    for total, dark, bright in ((1497, True, False), (1500, False, False), (6000, False, False), (6003, False, True)):
        img = np.full(30, total // 30, dtype=np.uint8)
        img[:total - 30 * (total // 30)] += 1
        st = FrameStats(DM.frame_records(img.reshape(1, 2, 5, 3)), 2, 5)
        assert st.mean[0] == total / 30 and (bool(st.too_dark[0]), bool(st.overexposed[0])) == (dark, bright), total
    st = FrameStats(DM.frame_records(np.full((1, 2, 5, 3), 100, np.uint8)), 2, 5, dark_limit=120, bright_limit=90, blur_limit=0)
    assert st.too_dark[0] and st.overexposed[0] and not st.blurry[0]      # the limits can be changed


def test_probability_records_by_hand():
    from unet_lane_detection_amd.diagnose import OutputStats
    v = DM.special_values(0.5)
    assert np.isnan(v[0]) and v[4] > 0 and v[4] < np.finfo(np.float32).tiny and v[6] > v[5] == np.float32(0.5)
    rec = DM.prob_records(v[None], 0.5)[0]
    # minimum -inf, maximum +inf; above 0.5: its successor, 1.0, 1.5, +inf; the sum: 0.5 -> 2^31, its successor
    # 0.5 + 2^-24 -> 2^31 + 2^8, three values clamped to 1 -> 2^32 each, everything else 0; one NaN
    assert rec.tolist() == [(0x7F800000 << 32) | 0xFF800000, 4, (1 << 31) + (1 << 31) + 256 + 3 * (1 << 32), 1]
    assert DM.prob_min_max(rec) == (-np.inf, np.inf)
    for zeros in ([0.0, -0.0], [-0.0, 0.0]):                  # -0.0 orders below +0.0
        rec = DM.prob_records(np.array([zeros], dtype=np.float32), 0.0)[0]
        assert rec.tolist() == [(0x00000000 << 32) | 0x80000000, 0, 0, 0]
    rec = DM.prob_records(np.full((1, 5), np.nan, dtype=np.float32))[0]
    assert rec.tolist() == [(0xFF800000 << 32) | 0x7F800000, 0, 0, 5]            # +inf below, -inf above
    rec = DM.prob_records(np.array([[0.25, 0.75, 0.75, 1.0]], dtype=np.float32), 0.75)
    st = OutputStats(rec, 4, 0.75)
    assert (st.min[0], st.max[0], st.share_above[0], st.mean[0], st.nan_count[0]) == (0.25, 1.0, 0.25, 0.6875, 0)
    assert st.mean[0] == DM.prob_mean(rec[0], 4)
    # the mean is the plane's to within 2^-32
    p = np.random.default_rng(3).random((2, 67 * 131), dtype=np.float32)
    st = OutputStats(DM.prob_records(p, 0.5), p.shape[1], 0.5)
    assert np.abs(st.mean - p.astype(np.float64).mean(axis=1)).max() <= 2.0 ** -32
    assert np.array_equal(st.share_above, (p > 0.5).mean(axis=1))


# ---- the discrimination proof ----------------------------------------------------------------------------------

def test_gpu_frames_tell_the_look_alikes_apart():
    """The frames tests/test_diagnose_gpu.py uses (same generator, same seeds): every look-alike gives another record
    - another border rule and exchanged R and B on every case with more than one pixel a side, a 32-bit sum of squares
    per 8,192 pixels on every case whose frames have that many, counted padding on the padded case."""
    seen = dict(border=0, swap=0, s2=0)
    for n, h, w in DM.FRAME_CASES:
        frames = DM.make_frames(DM.frames_seed(n, h, w), n, h, w)
        for bgr in (True, False):
            rule = DM.frame_records(frames, bgr)
            if h * w > 1:
                assert (DM.frame_records(frames, bgr, border="replicate")[:, 3:5] != rule[:, 3:5]).any(axis=1).all(), (n, h, w)
                assert (DM.frame_records(frames, bgr, swap=True)[:, 3:5] != rule[:, 3:5]).any(axis=1).all(), (n, h, w)
                seen["border"] += 1
                seen["swap"] += 1
            if h * w >= 8192:
                assert (DM.frame_records(frames, bgr, s2_chunk=8192)[:, 4] != rule[:, 4]).all(), (n, h, w)
                seen["s2"] += 1
    assert seen["border"] >= 10 and seen["s2"] >= 6
    (n, h, w), stride = DM.PADDED_CASE
    rows = DM.padded_rows(DM.make_frames(DM.frames_seed(n, h, w), n, h, w), stride)
    rule, counted = DM.frame_records(rows, width=w), DM.frame_records(rows, width=w, count_padding=True)
    assert (counted[:, 2] != rule[:, 2]).all() and np.array_equal(counted[:, 3:], rule[:, 3:])
    assert np.array_equal(rule, DM.frame_records(DM.make_frames(DM.frames_seed(n, h, w), n, h, w)))
    # uniformly random colours alone would not do for the 32-bit sum: 8,192 of their squares stay below 2^32
    noise = np.random.default_rng(0).integers(0, 256, (1, 128, 128, 3), dtype=np.uint8)
    assert np.array_equal(DM.frame_records(noise, s2_chunk=8192), DM.frame_records(noise))
