"""Lane following's host side: the two entry points are exported and refuse bad arguments before a device is touched,
tests/follow_model.py and follow.LineFollower reproduce the reference's `LineFollower` (tests/golden/lane_follow.npz),
the model's morphology has the properties of a closing and an opening, and the painted test frames of
tests/test_follow_gpu.py are a test of the morphology: a model whose erosions pad with 0 cannot pass them."""
import ctypes as C
import os

import numpy as np
import pytest

import follow_model as FM
from unet_lane_detection_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lane_follow.npz")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the entry points ------------------------------------------------------------------------------------------

def test_symbols_exported(lib):
    for name in ("unet_hsv_lanes_u8_batch", "unet_lane_center_u8_batch"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def _refused(lib, rc, call):
    msg = lib.unet_op_last_error()
    return rc == 1 and msg.startswith(b"invalid argument") and call in msg


def test_hsv_lanes_refuses_bad_arguments(lib):
    call = lib.unet_hsv_lanes_u8_batch
    name = b"unet_hsv_lanes_u8_batch"
    frames = C.cast((C.c_uint8 * (2 * 4 * 4 * 3))(), C.c_void_p)
    out_bytes = (C.c_uint8 * (2 * 4 * 4))()
    out = C.cast(out_bytes, C.c_void_p)
    lo, hi = (C.c_uint8 * 3)(0, 0, 185), (C.c_uint8 * 3)(180, 40, 255)
    lo, hi = C.cast(lo, C.c_void_p), C.cast(hi, C.c_void_p)
    for kc, ko in ((2, 5), (5, 4), (0, 5), (5, 0), (9, 5), (5, 9), (-3, 3), (6, 6)):     # even or out-of-set sizes
        assert _refused(lib, call(0, frames, 2, 4, 4, 1, lo, hi, kc, ko, out, None), name), (kc, ko)
        assert b"ksize" in lib.unet_op_last_error()
    assert _refused(lib, call(0, None, 2, 4, 4, 1, lo, hi, 5, 5, out, None), name)       # null pointers
    assert _refused(lib, call(0, frames, 2, 4, 4, 1, None, hi, 5, 5, out, None), name)
    assert _refused(lib, call(0, frames, 2, 4, 4, 1, lo, None, 5, 5, out, None), name)
    assert _refused(lib, call(0, frames, 2, 4, 4, 1, lo, hi, 5, 5, None, None), name)
    assert _refused(lib, call(0, frames, 0, 4, 4, 1, lo, hi, 5, 5, out, None), name)     # n <= 0 and empty images
    assert _refused(lib, call(0, frames, -1, 4, 4, 1, lo, hi, 5, 5, out, None), name)
    assert _refused(lib, call(0, frames, 2, 0, 4, 1, lo, hi, 5, 5, out, None), name)
    assert _refused(lib, call(0, frames, 2, 4, 0, 1, lo, hi, 5, 5, out, None), name)
    assert _refused(lib, call(0, frames, 2, 1 << 15, 1 << 15, 1, lo, hi, 5, 5, out, None), name)   # 2^31 pixels
    assert b"2^31" in lib.unet_op_last_error()
    assert not any(out_bytes)
    # what passes the checks goes on to the device: an ordinal the runtime refuses shows it got that far
    for kc, ko in ((5, 5), (1, 1), (7, 3)):
        assert call(1 << 20, frames, 2, 4, 4, 0, lo, hi, kc, ko, out, None) == _lib.UNET_ERR_HIP
        assert b"hipSetDevice" in lib.unet_op_last_error()


def test_lane_center_refuses_bad_arguments(lib):
    call = lib.unet_lane_center_u8_batch
    name = b"unet_lane_center_u8_batch"
    masks = C.cast((C.c_uint8 * (2 * 8 * 8))(), C.c_void_p)
    out_words = (C.c_uint32 * (2 * 65 * 2))()
    out = C.cast(out_words, C.c_void_p)

    def rows(*v):
        return (C.c_int * len(v))(*v)
    ok = rows(5)
    assert _refused(lib, call(0, None, 2, 8, 8, ok, 1, 127, out, None), name)            # null pointers
    assert _refused(lib, call(0, masks, 2, 8, 8, None, 1, 127, out, None), name)
    assert _refused(lib, call(0, masks, 2, 8, 8, ok, 1, 127, None, None), name)
    assert _refused(lib, call(0, masks, 0, 8, 8, ok, 1, 127, out, None), name)           # n <= 0
    assert _refused(lib, call(0, masks, -2, 8, 8, ok, 1, 127, out, None), name)
    assert _refused(lib, call(0, masks, 2, 8, 8, rows(8), 1, 127, out, None), name)      # a row outside the image
    assert b"row" in lib.unet_op_last_error()
    assert _refused(lib, call(0, masks, 2, 8, 8, rows(-1), 1, 127, out, None), name)
    assert _refused(lib, call(0, masks, 2, 8, 8, rows(0, 7, 8), 3, 127, out, None), name)
    assert _refused(lib, call(0, masks, 2, 8, 8, ok, 0, 127, out, None), name)           # n_rows of 0 and of 65
    assert _refused(lib, call(0, masks, 2, 8, 8, rows(*([1] * 65)), 65, 127, out, None), name)
    assert b"n_rows" in lib.unet_op_last_error()
    assert _refused(lib, call(0, masks, 2, 8, 8, ok, 1, 256, out, None), name)           # level of 256, and below 0
    assert b"level" in lib.unet_op_last_error()
    assert _refused(lib, call(0, masks, 2, 8, 8, ok, 1, -1, out, None), name)
    assert _refused(lib, call(0, masks, 1, 1, 65536, rows(0), 1, 127, out, None), name)  # width of 65536
    assert b"65535" in lib.unet_op_last_error()
    assert not any(out_words)
    bad = 1 << 20
    assert call(bad, masks, 2, 8, 8, rows(*range(8)), 8, 127, out, None) == _lib.UNET_ERR_HIP
    assert b"hipSetDevice" in lib.unet_op_last_error()
    assert call(bad, masks, 2, 8, 8, rows(*([7] * 64)), 64, 255, out, None) == _lib.UNET_ERR_HIP
    assert call(bad, masks, 1, 1, 65535, rows(0), 1, 0, out, None) == _lib.UNET_ERR_HIP


# ---- the reference's LineFollower ------------------------------------------------------------------------------

def test_model_and_host_centres_reproduce_the_reference():
    from unet_lane_detection_amd import follow as F
    z = np.load(GOLDEN)
    masks, rows, want = z["masks"], z["scan_rows"], z["centers"]
    assert {0, 10, 11} <= {int((m[FM.default_row(m.shape[0])] > 127).sum()) for m in masks}
    assert (want >= 0).any() and (want < 0).any() and (rows >= 0).any()
    for m, r, c in zip(masks, rows, want):
        got = FM.lane_centers(m[None], None if r < 0 else [int(r)])[0][0]
        assert (-1 if got is None else got) == int(c)
        row = FM.default_row(m.shape[0]) if r < 0 else int(r)
        host = F.centers_from_sums(FM.lane_sums(m[None], [row]))[0][0]
        assert host == got
    # counts and sums that only fit an unsigned 32-bit word come back whole through the int32 view of the device
    big = np.array([[[65535, 65535 * 65534 // 2]]], dtype=np.uint32).view(np.int32)
    assert F.centers_from_sums(big) == [[32767]]


def test_line_follower_reproduces_the_reference_trajectory():
    from unet_lane_detection_amd.follow import LineFollower
    z = np.load(GOLDEN)
    pid = LineFollower()
    published = 0
    for mask, want_z, want_x in zip(z["traj_masks"], z["traj_angular"], z["traj_linear"]):
        centre = FM.lane_centers(mask[None])[0][0]
        cmd = pid.update(centre, mask.shape[1])
        if np.isnan(want_z):
            assert centre is None and cmd is None
        else:
            assert cmd is not None and cmd[0] == want_x and cmd[1] == want_z     # exactly: the same operations in order
            published += 1
    assert 20 <= published < 30


# ---- the model itself ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 5, 7])
def test_close_is_extensive_and_open_is_anti_extensive(k):
    rng = np.random.default_rng(k)
    for shape, density in (((23, 31), 0.3), ((9, 40), 0.7), ((5, 5), 0.5), ((1, 17), 0.4)):
        x = ((rng.random(shape) < density) * 255).astype(np.uint8)
        closed, opened = FM.close_open(x, k, 1), FM.close_open(x, 1, k)
        assert (closed >= x).all() and (opened <= x).all()
        assert np.array_equal(FM.close_open(closed, k, 1), closed) and np.array_equal(FM.close_open(opened, 1, k), opened)
    ones = np.full((6, 7), 255, dtype=np.uint8)
    assert np.array_equal(FM.close_open(ones, k, k), ones)       # neutral borders: an all-white image stays white
    assert np.array_equal(FM.erode(ones, k), ones) and not FM.erode(ones, k, pad=0)[0].any()


def test_k1_is_the_identity():
    x = np.random.default_rng(0).integers(0, 2, (13, 11)).astype(np.uint8) * 255
    assert np.array_equal(FM.dilate(x, 1), x) and np.array_equal(FM.erode(x, 1), x)
    assert np.array_equal(FM.close_open(x, 1, 1), x)
    frames = np.random.default_rng(1).integers(0, 256, (2, 6, 5, 3), dtype=np.uint8)
    assert np.array_equal(FM.hsv_lanes(frames, close_ksize=1, open_ksize=1), FM.in_range(frames))


def test_in_range_on_hand_made_pixels():
    px = np.array([[255, 255, 255], [184, 184, 184], [185, 185, 185], [255, 215, 215], [255, 214, 214], [0, 0, 0]],
                  dtype=np.uint8)                           # white, V 184 / 185, S 40 / 41, black
    assert FM.in_range(px[None], bgr=False)[0].tolist() == [255, 0, 255, 255, 0, 0]
    assert FM.in_range(px[None], bgr=True)[0].tolist() == [255, 0, 255, 255, 0, 0]
    blue_rgb = np.array([[[0, 0, 200]]], dtype=np.uint8)    # H = 120 as RGB, H = 0 read as BGR
    assert FM.in_range(blue_rgb, (120, 0, 0), (120, 255, 255), bgr=False)[0, 0] == 255
    assert FM.in_range(blue_rgb, (120, 0, 0), (120, 255, 255), bgr=True)[0, 0] == 0


# ---- the discrimination proof ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w", [(3, 67, 131), (2, 64, 256)])
def test_painted_frames_are_a_test_of_the_morphology(n, h, w):
    """The frames tests/test_follow_gpu.py uses (same generator, same seeds): the output is neither empty nor full,
    the morphology changes a good share of the threshold plane, and the look-alike whose erosions pad with 0 instead
    of the neutral value gives another answer.  Uniformly random colours alone would leave 1.5 % positives."""
    frames, _ = FM.painted_frames(FM.painted_seed(n, h, w), n, h, w)
    plane = FM.in_range(frames)
    out = FM.hsv_lanes(frames, close_ksize=5, open_ksize=5)
    share, changed = float((out == 255).mean()), float((out != plane).mean())
    mutant = int((FM.hsv_lanes(frames, close_ksize=5, open_ksize=5, erode_pad=0) != out).sum())
    print(f"({n},{h},{w}): positive share {share:.3f}, changed by the morphology {changed:.3f}, mutant differs in {mutant} pixels")
    assert 0.1 <= share <= 0.6
    assert changed >= 0.05
    assert mutant >= 1
    noise = np.random.default_rng(0).integers(0, 256, (1, 64, 64, 3), dtype=np.uint8)
    assert (FM.in_range(noise) == 255).mean() < 0.05
