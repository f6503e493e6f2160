"""The frame correction inside the two pipelines (follow.LaneFollowPipeline, video.FramePipeline), on the GPU.
Everything compared is an integer; there is no tolerance.

The cast track is the one of tests/test_correct_cpu.py (the reference's failure case 1).  Two kinds of statement:
  - with the reference's bird's-eye warp, a pipeline with `correct=` fed the cast message gives exactly what the same
    pipeline without it gives when fed the message the numpy model corrected: the stage sits in front of the warp and
    changes nothing else;
  - "the centres are those of the uncast frame" is stated under a warp that maps every pixel onto itself.  The
    corrected frame is not the uncast frame (gray world keeps the frame's mean, so white is 216, not 240), and
    under a magnifying bilinear warp the blend of marking and surface crosses V = 185 at another sub-pixel position
    (at a share of 0.61 of the marking for 240 / 100, of 0.75 for 216 / 90), which moves a centre by a pixel or two:
    that is the warp's blending, not the correction.  Without blending the masks are equal bit for bit, as the CPU
    test shows in numpy, and so are the centres."""
import numpy as np
import pytest
import torch

import correct_model as CM
import diagnose_model as DM
import follow_model as FM
from unet_lane_detection_amd import correct as K
from unet_lane_detection_amd import follow as F
from unet_lane_detection_amd import ros_bridge as RB
from unet_lane_detection_amd import state as S

pytestmark = pytest.mark.gpu

H, W = 480, 640
STEP = 3 * W + 16
SCAN = [120, 300, int(685 * 0.7), 640]
GRAY_WORLD = CM.config(white_balance=1)


def message(img, encoding="bgr8"):
    """an ImageMsg with a padded step, the padding set to 255"""
    rows = np.full((H, STEP), 255, dtype=np.uint8)
    rows[:, :3 * W] = img.reshape(H, 3 * W)
    return RB.ImageMsg(height=H, width=W, encoding=encoding, data=rows.tobytes(), step=STEP, header="hdr")


@pytest.fixture(scope="module")
def tracks():
    clean = CM.track(H, W)
    bad = CM.cast(clean)
    fixed = CM.correct(bad[None], GRAY_WORLD)
    return clean, bad, fixed["out"][0], fixed["plan"]


@pytest.fixture(scope="module")
def small_model():
    from unet_lane_detection_amd.model import UNetHIP
    model = UNetHIP(S.seeded_state_dict([8, 16], seed=4), device=0)
    yield model
    model.release()


def test_correct_none_changes_nothing():
    img = FM.painted_frames(5, 1, H, W)[0][0]
    msg = message(img)
    without = F.LaneFollowPipeline(None, source="hsv", scan_rows=SCAN)
    none = F.LaneFollowPipeline(None, source="hsv", scan_rows=SCAN, correct=None)
    want, want_mask = without.process(msg, return_mask=True)
    got, got_mask = none.process(msg, return_mask=True)
    assert got == want and any(c is not None for c in got) and got_mask.data == want_mask.data
    assert none.corrector is None and none.last_correction is None


def test_the_cast_track_without_and_with_the_correction(tracks):
    clean, bad, fixed, plan = tracks
    corners = ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1))
    kw = dict(source="hsv", scan_rows=[100, 240, int(H * 0.7), 470], src_points=corners, dst_points=corners,
              warp_size=(W, H))
    plain = F.LaneFollowPipeline(None, **kw)
    corrected = F.LaneFollowPipeline(None, correct=K.CorrectConfig(white_balance="gray_world"), **kw)
    want = FM.lane_centers(FM.hsv_lanes(clean[None]), kw["scan_rows"])[0]
    assert all(c is not None for c in want)
    assert plain.process(message(clean)) == want
    assert plain.process(message(bad)) == [None] * 4                     # no centre on any scan row
    got, mask = corrected.process(message(bad), return_mask=True)
    assert got == want                                                   # the centres of the uncast frame
    assert np.array_equal(np.frombuffer(mask.data, np.uint8).reshape(H, W), FM.hsv_lanes(clean[None])[0])
    p = corrected.last_correction
    assert np.array_equal(p.words, plan) and p.corrected.tolist() == [True]
    assert p.gains[0, 0] > 1.2 and p.gains[0, 1] < 1.0
    # the same frame sent as rgb8: the gains follow the channels
    assert corrected.process(message(bad[..., ::-1].copy(), "rgb8")) == want
    assert np.array_equal(corrected.last_correction.words[0, 1:4], plan[0, [3, 2, 1]])


@pytest.mark.parametrize("source", ["hsv", "unet"])
def test_the_stage_sits_in_front_of_the_warp(tracks, small_model, source):
    """the reference's warp: correct= on the cast message == no correct= on the message the model corrected"""
    clean, bad, fixed, plan = tracks
    model = small_model if source == "unet" else None
    kw = dict(source=source, scan_rows=SCAN)
    if source == "unet":
        kw.update(input_size=(32, 32), precision="fp32")
    plain = F.LaneFollowPipeline(model, **kw)
    corrected = F.LaneFollowPipeline(model, correct=K.CorrectConfig(), **kw)
    want, want_mask = plain.process(message(fixed), return_mask=True)
    got, got_mask = corrected.process(message(bad), return_mask=True)
    assert got == want and got_mask.data == want_mask.data
    if source == "hsv":
        assert any(c is not None for c in got) and plain.process(message(bad)) == [None] * 4
    assert np.array_equal(corrected.last_correction.words, plan)


def test_diagnose_and_view_still_see_the_raw_rows(tracks):
    from unet_lane_detection_amd.laneview import ViewConfig
    clean, bad, fixed, plan = tracks
    cfg = K.CorrectConfig()
    diag = F.LaneFollowPipeline(None, source="hsv", scan_rows=SCAN, diagnose=True, correct=cfg)
    centres, stats = diag.process(message(bad))
    assert np.array_equal(stats.words, DM.frame_records(bad[None])) and any(c is not None for c in centres)
    raw_view = F.LaneFollowPipeline(None, source="hsv", scan_rows=SCAN, view=ViewConfig())
    assert raw_view.process(message(bad)) == [None] * 4                  # nothing found: every pixel is layer 0
    assert not raw_view.last_view_layers.any()
    fixed_view = F.LaneFollowPipeline(None, source="hsv", scan_rows=SCAN, view=ViewConfig())
    fixed_view.process(message(fixed))
    view = F.LaneFollowPipeline(None, source="hsv", scan_rows=SCAN, view=ViewConfig(), correct=cfg)
    assert view.process(message(bad)) == centres
    assert torch.equal(view.last_view_layers, fixed_view.last_view_layers) and view.last_view_layers.any()
    untouched = (view.last_view_layers == 0)[..., None].expand_as(view.last_view)
    assert torch.equal(view.last_view[untouched], raw_view.last_view[untouched])   # drawn on what the camera saw


def test_frame_pipeline_with_correct(small_model):
    from unet_lane_detection_amd import video as V
    kw = dict(threshold=0.5, input_size=(32, 32), precision="fp32")
    cfg = CM.config(white_balance=1, lo_bp=100, hi_bp=100, clahe=1, grid_x=4, grid_y=3)
    config = K.CorrectConfig(stretch=(1.0, 1.0), clahe=K.Clahe(2.0, (4, 3)))
    frames = CM.scene(21, 5, 45, 61)
    fixed = CM.correct(frames, cfg)["out"]
    plain, corrected = V.FramePipeline(small_model, **kw), V.FramePipeline(small_model, correct=config, **kw)
    overlay, mask = plain.process(fixed)
    overlay_c, mask_c = corrected.process(frames)
    assert torch.equal(overlay, overlay_c) and torch.equal(mask, mask_c)
    chunks, fixed_chunks = [frames[0:2], frames[2:5]], [fixed[0:2], fixed[2:5]]
    want = list(plain.run(fixed_chunks))
    got = list(corrected.run(chunks))
    assert len(got) == 2
    for (w_ov, w_mk), (g_ov, g_mk) in zip(want, got):
        assert np.array_equal(w_ov, g_ov) and np.array_equal(w_mk, g_mk)
    # with diagnose the chunk is measured as it came
    both = V.FramePipeline(small_model, correct=config, diagnose=True, **kw)
    (ov, mk), stats = both.process(frames)
    assert torch.equal(ov, overlay) and np.array_equal(stats.words, DM.frame_records(frames))
    # and without correct= nothing of the stage exists
    assert plain.corrector is None and V.FramePipeline(small_model, correct=None, **kw).corrector is None
