"""The lane view on the GPU (csrc/laneview_kernels.cpp through the C ABI, unet_lane_detection_amd/laneview.py and
follow.LaneFollowPipeline(view=...)) against tests/laneview_model.py: every comparison is bit-exact and covers the
whole view and the whole layer plane.  Every buffer lies between canaries; the small frames come with a base pointer
one byte off and a row pitch that is no multiple of 16 (the byte-wise form and the row tails) and dense and aligned
(the 16-byte form); inputs are verified unmodified.  tests/test_laneview_cpu.py shows that the small cases tell the
model's mutants apart.  Parity of the mask layer with cv2.warpPerspective itself is unpinned."""
import ctypes as C

import numpy as np
import pytest
import torch

import follow_model as FM
import lanefit_model as LM
import laneview_cases as LC
import laneview_model as M
from unet_lane_detection_amd import _lib
from unet_lane_detection_amd import follow as F
from unet_lane_detection_amd import instances as I
from unet_lane_detection_amd import lanefit as LF
from unet_lane_detection_amd import laneview as LV
from unet_lane_detection_amd import ros_bridge as RB

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 64


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=False)


class Buf:
    """`size` device bytes at byte `lead` of a larger buffer filled with a canary: lead = 64 keeps the view 64-byte
    aligned, lead = 65 puts it one byte off; at least 64 canary bytes on either side.  Without data the view itself
    holds the canary."""

    def __init__(self, size, lead=GUARD, data=None):
        self.whole = torch.full((lead + size + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.view = self.whole[lead:lead + size]
        self.lead, self.size = lead, size
        if data is not None:
            self.data = np.array(data).reshape(-1).view(np.uint8)
            self.view.copy_(torch.from_numpy(self.data))

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def numpy(self):
        return self.view.cpu().numpy()

    def intact(self):
        """the canaries on both sides, and for an input its contents"""
        w = self.whole.cpu().numpy()
        ok = bool((w[:self.lead] == CANARY).all() and (w[self.lead + self.size:] == CANARY).all())
        return ok and (not hasattr(self, "data") or np.array_equal(w[self.lead:self.lead + self.size], self.data))


def c_style(style):
    return LC.view_config(style).style()


def rows_of(frames, step):
    """(n, h, w, 3) pixels -> (n, h, step) rows, the padding filled with a value no pixel of the view may take from it"""
    n, h, w = frames.shape[:3]
    rows = np.full((n, h, step), 0x5A, dtype=np.uint8)
    rows[:, :, :3 * w] = frames.reshape(n, h, 3 * w)
    return rows


def run(lib, frames, step, m, warp, masks, curves, style, level=127, lead=GUARD, out_lead=None, want_view=True,
        want_layers=True):
    """one call of unet_lane_view_u8_batch on canaried buffers -> (view or None, layers or None) on the host"""
    n, h, w = frames.shape[:3]
    out_lead = lead if out_lead is None else out_lead
    src = Buf(n * h * step, lead, rows_of(frames, step))
    msk = None if masks is None else Buf(masks.size, lead, masks)
    k = 0 if curves is None else curves.shape[1]
    tab = None if curves is None else Buf(curves.size * 8, GUARD, np.ascontiguousarray(curves, dtype=np.int64))
    view = Buf(n * h * w * 3, out_lead) if want_view else None
    lay = Buf(n * h * w, out_lead) if want_layers else None
    mm = np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(9))
    st = c_style(style)
    rc = lib.unet_lane_view_u8_batch(0, src.ptr(), n, h, w, step, mm.ctypes.data_as(C.POINTER(C.c_double)), warp[0], warp[1],
                                     msk.ptr() if msk else None, level, tab.ptr() if tab else None, k, C.byref(st),
                                     view.ptr() if view else None, lay.ptr() if lay else None, None)
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    for b in (src, msk, tab, view, lay):
        assert b is None or b.intact()
    return (view.numpy().reshape(n, h, w, 3) if view else None, lay.numpy().reshape(n, h, w) if lay else None)


_WANT = {}


def want_small(kind, matrix, style_name):
    """the model's answer for a small case, computed once"""
    key = (kind, matrix, style_name)
    if key not in _WANT:
        case = LC.small(kind, matrix)
        style = getattr(LC, style_name)
        _WANT[key] = M.lane_view(case["frames"], case["m"], *case["warp"], case["masks"], 127, case["curves"], style)
    return _WANT[key]


# ---- the small frames ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,matrix", LC.SMALL)
def test_small_frames_bit_for_bit(lib, kind, matrix):
    """n = 3, a different table per frame (no curve; one; a filling, a crossing, an outside and a refused one), rows
    that start and end inside the image.  "scalar": 37 x 53, step = 3 * 53 + 5, every pointer one byte off - the
    byte-wise form and the row tails; "vector": 32 x 64 dense on 64-byte aligned pointers - the 16-byte form"""
    case = LC.small(kind, matrix)
    lead = GUARD + 1 if kind == "scalar" else GUARD
    for style_name in ("LOUD", "PLAIN"):
        want_view, want_layers = want_small(kind, matrix, style_name)
        view, layers = run(lib, case["frames"], case["step"], case["m"], case["warp"], case["masks"], case["curves"],
                           getattr(LC, style_name), lead=lead)
        assert np.array_equal(layers, want_layers), (style_name, np.argwhere(layers != want_layers)[:5])
        assert np.array_equal(view, want_view), (style_name, np.argwhere(view != want_view)[:5])
    if matrix == "horizon":
        assert (want_layers == 0).any() and (want_layers[2] == 1).any()


def test_both_forms_give_the_same_bits(lib):
    """the dense 32 x 64 frames once more with the input one byte off (byte-wise loads, 16-byte stores) and with the
    outputs one byte off (16-byte loads, byte-wise stores)"""
    case = LC.small("vector", "horizon")
    want = want_small("vector", "horizon", "LOUD")
    for lead, out_lead in ((GUARD + 1, GUARD), (GUARD, GUARD + 1)):
        got = run(lib, case["frames"], case["step"], case["m"], case["warp"], case["masks"], case["curves"], LC.LOUD,
                  lead=lead, out_lead=out_lead)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_null_mask_null_curves_and_either_output(lib):
    case = LC.small("scalar", "horizon")
    args = (case["frames"], case["step"], case["m"], case["warp"])
    model_args = (case["frames"], case["m"], *case["warp"])
    # no mask: curves and area only
    want = M.lane_view(*model_args, None, 127, case["curves"], LC.LOUD)
    got = run(lib, *args, None, case["curves"], LC.LOUD, lead=GUARD + 1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not (want[1] == 2).any()
    # no curves: the mask layer only
    want = M.lane_view(*model_args, case["masks"], 127, None, LC.LOUD)
    got = run(lib, *args, case["masks"], None, LC.LOUD, lead=GUARD + 1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and set(np.unique(want[1])) == {0, 2}
    # neither: every pixel is the frame blended with itself
    want = M.lane_view(*model_args, None, 127, None, LC.LOUD)
    got = run(lib, *args, None, None, LC.LOUD)
    assert np.array_equal(got[0], want[0]) and not got[1].any()
    # each output alone
    want = want_small("scalar", "horizon", "LOUD")
    view, none = run(lib, *args, case["masks"], case["curves"], LC.LOUD, want_layers=False)
    assert none is None and np.array_equal(view, want[0])
    none, layers = run(lib, *args, case["masks"], case["curves"], LC.LOUD, want_view=False)
    assert none is None and np.array_equal(layers, want[1])
    # the layers switched off in the style, and another level
    for style in (M.Style(draw_area=False, thickness=2), M.Style(draw_marking=False, gamma=9.0, thickness=64)):
        want = M.lane_view(*model_args, case["masks"], 200, case["curves"], style)
        got = run(lib, *args, case["masks"], case["curves"], style, level=200)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_records_of_random_words_are_clamped_like_the_model(lib):
    """the kernel cannot have checked a record: 8 records a frame of random 64-bit words, and a second table whose
    flags and rows are tame so that the wild coefficients are really evaluated"""
    case = LC.small("vector", "identity")
    rng = np.random.default_rng(77)
    wild = rng.integers(-(1 << 63), (1 << 63) - 1, (3, 8, M.WORDS), dtype=np.int64, endpoint=True)
    tame = wild.copy()
    tame[:, :, 0] = 7
    tame[:, :, 1], tame[:, :, 2] = 0, 31
    tame[:, :, 3] >>= 36            # coefficients of every size up to and beyond the bounds
    tame[:, 0::2, 4] >>= 20
    tame[:, 1::2, 5] >>= 24
    for table in (wild, tame):
        want = M.lane_view(case["frames"], case["m"], *case["warp"], case["masks"], 127, table, LC.LOUD)
        got = run(lib, case["frames"], case["step"], case["m"], case["warp"], case["masks"], table, LC.LOUD)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    assert want[1].max() >= 3


def test_coefficients_at_the_bound_with_the_largest_y(lib):
    """a 17 x 64 frame stretched over an 8192 x 2048 bird's-eye image: the last camera row is Y = 2^16 - 1 exactly, the
    largest an INSIDE pixel has, and every record sits at the clamp's bound"""
    h, w = 17, 64
    m = np.diag([8191.0 / 63.0, 2047.96875 / 16.0, 1.0])
    valid, X, Y = M.positions(m, w, h)
    assert valid.all() and int(Y.max()) == (1 << 16) - 1 and int(X.max()) == 32 * 8191
    frames = LC.frames_of(9, 1, h, w)
    table = LC.extreme_records()
    beyond = table.copy()
    beyond[:, :, 3:6] *= 4          # beyond the bound: clamped back onto it
    want = M.lane_view(frames, m, 8192, 2048, None, 127, table, LC.PLAIN)
    assert (want[1] == 1).all()     # between -2^30 and +2^30 pixels: the area, on every pixel
    for t in (table, beyond):
        got = run(lib, frames, 3 * w, m, (8192, 2048), None, t, LC.PLAIN)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


# ---- the real size ---------------------------------------------------------------------------------------------

def test_reference_calibration_with_fitted_lanes():
    """480 x 640 through the reference's calibration onto 1055 x 685, painted markings and the fits the lane-fit kernel
    gives for them, through laneview.lane_view (which orients the matrix: the road has w < 0 as
    cv2.getPerspectiveTransform scales it)"""
    h, w, warp = 480, 640, RB.REF_WARP_SIZE
    matrix = RB.get_perspective_transform(RB.REF_SRC_POINTS, RB.REF_DST_POINTS)
    mask = LM.painted_lanes(LM.painted_seed(2, warp[1], warp[0]), 2, warp[1], warp[0])[:1]
    frames = FM.painted_frames(5, 1, h, w)[0]
    mask_dev = torch.from_numpy(mask).cuda()
    fits = LF.lane_fits(mask_dev)
    assert all(lane.coeffs is not None for lane in fits[0].lanes)
    frames_dev = torch.from_numpy(frames).cuda()
    for extent in ("frame", "pixels"):
        cfg = LV.ViewConfig(extent=extent, thickness=6)
        table = LV.curve_table(fits, warp, cfg)
        assert table.shape == (1, 2, 8) and [int(v) for v in table[0, :, 0]] == [7, 5]
        view, layers = LV.lane_view(frames_dev, matrix, warp, mask_dev, table, cfg, layers=True)
        style = M.Style(thickness=6)
        want = M.lane_view(frames, LV.orient(matrix, warp), warp[0], warp[1], mask, 127, table, style)
        assert np.array_equal(layers.cpu().numpy(), want[1]) and np.array_equal(view.cpu().numpy(), want[0])
        counts = np.bincount(want[1].reshape(-1), minlength=5)
        print(f"extent {extent}: pixels per layer {counts.tolist()}")
        assert (counts[:5] > 0).all()        # the sky, the drivable area, both markings' pixels and both curves are there
    only = LV.lane_view(frames_dev[0], matrix, warp, mask_dev[0], table, cfg)
    assert torch.equal(only, view)
    with pytest.raises(ValueError):
        LV.lane_view(frames_dev, matrix, warp, mask_dev, table[:, :, :7], cfg)
    with pytest.raises(TypeError):
        LV.lane_view(frames, matrix, warp)


def test_identity_draws_onto_the_birds_eye_image():
    """matrix = eye(3), warp_size = (width, height): the mask layer is the mask's own pixels"""
    h, w = 40, 72
    frames, masks = LC.frames_of(21, 2, h, w), LC.masks_of(22, 2, w, h)
    view, layers = LV.lane_view(torch.from_numpy(frames).cuda(), np.eye(3), (w, h), torch.from_numpy(masks).cuda(),
                                layers=True)
    assert np.array_equal(layers.cpu().numpy() == 2, masks > 127)
    want = M.lane_view(frames, np.eye(3), w, h, masks, 127, None)
    assert np.array_equal(view.cpu().numpy(), want[0])


# ---- the pipeline ----------------------------------------------------------------------------------------------

class FixedMask:
    """an extractor that answers every frame with one prepared mask: the pipeline's warp still runs in front of it"""

    def __init__(self, mask):
        self.mask = torch.from_numpy(np.array(mask)).cuda()

    def extract(self, frame, bgr=False):
        return self.mask[None].clone()


def _message(img_bgr, pitch_pad=16):
    h, w = img_bgr.shape[:2]
    step = w * 3 + pitch_pad
    rows = np.zeros((h, step), dtype=np.uint8)
    rows[:, :w * 3] = img_bgr.reshape(h, w * 3)
    return RB.ImageMsg(height=h, width=w, encoding="bgr8", data=rows.tobytes(), step=step, header="hdr")


SCAN_ROWS = [120, 300, int(685 * 0.7), 640]


@pytest.fixture(scope="module")
def pipeline_inputs():
    warp = RB.REF_WARP_SIZE
    mask = LM.painted_lanes(LM.painted_seed(2, warp[1], warp[0]), 2, warp[1], warp[0])[0]
    frame = FM.painted_frames(5, 1, 480, 640)[0][0]
    return mask, frame, _message(frame)


@pytest.mark.parametrize("extra", ["fit", "clean", "both", "neither"])
def test_follow_pipeline_with_view(pipeline_inputs, extra):
    """view=ViewConfig() leaves the centres, the fits and the returned mask message as they are without it, and
    last_view is the model's answer on the same rows, mask and curves"""
    mask, frame, msg = pipeline_inputs
    kw = {}
    if extra in ("fit", "both"):
        kw["fit"] = LF.FitConfig()
    if extra in ("clean", "both"):
        kw["clean"] = I.CleanConfig(min_area=200, keep_largest=6, max_components=16384)   # the speckle has ids too

    def make(**more):
        return F.LaneFollowPipeline(None, source="hsv", extractor=FixedMask(mask), scan_rows=SCAN_ROWS, **kw, **more)
    cfg = LV.ViewConfig()
    plain, none, viewed = make(), make(view=None), make(view=cfg)

    def unpack(result):
        (centres, mask_msg), fits = result if "fit" in kw else (result, None)
        return centres, mask_msg, fits
    c0, m0, f0 = unpack(plain.process(msg, return_mask=True))
    c1, m1, f1 = unpack(none.process(msg, return_mask=True))
    c2, m2, f2 = unpack(viewed.process(msg, return_mask=True))
    assert c0 == c1 == c2 and m0.data == m1.data == m2.data and (m2.height, m2.width, m2.encoding) == (685, 1055, "mono8")
    if "fit" in kw:
        assert np.array_equal(f0.words, f1.words) and np.array_equal(f0.words, f2.words)
    assert plain.last_view is None and none.last_view is None and none.view_msg() is None
    assert viewed.process(msg) == plain.process(msg) if "fit" not in kw else True     # the return shape is unchanged
    # the model on the same rows, mask and curves
    used = np.frombuffer(m2.data, dtype=np.uint8).reshape(1, 685, 1055)
    if "fit" in kw:
        table = LV.curve_table(f2, RB.REF_WARP_SIZE, cfg)
    elif "clean" in kw:
        table = LV.curve_table(I.lane_instances(torch.from_numpy(mask).cuda(), kw["clean"]), RB.REF_WARP_SIZE, cfg)
        assert table.shape[1] >= 2
    else:
        table = None
    want = M.lane_view(frame[None], LV.orient(viewed.matrix, RB.REF_WARP_SIZE), 1055, 685, used, 127, table, M.Style())
    view = viewed.last_view
    assert tuple(view.shape) == (1, 480, 640, 3) and view.is_cuda
    assert np.array_equal(viewed.last_view_layers.cpu().numpy(), want[1]) and np.array_equal(view.cpu().numpy(), want[0])
    if table is None:
        assert set(np.unique(want[1])) == {0, 2}
    elif "fit" in kw:
        assert {0, 1, 2, 3, 4} <= set(np.unique(want[1]))         # the lane area and both curves
    else:
        assert {0, 2, 3, 4} <= set(np.unique(want[1])) and table.shape[1] == 6
    out = viewed.view_msg()
    assert (out.height, out.width, out.encoding, out.step, out.header) == (480, 640, "bgr8", 640 * 3, "hdr")
    assert out.data == want[0][0].tobytes()
