"""The lane fit on the GPU (csrc/lanefit_kernels.cpp through the C ABI, unet_lane_detection_amd/lanefit.py and
follow.LaneFollowPipeline(fit=...)) against tests/lanefit_model.py: every comparison is bit-exact and covers all 16
words of every record.  There is no reference code for the fit; parity with any outside implementation is unpinned
(see the model's header).  tests/test_lanefit_cpu.py shows that the crafted and painted masks used here tell the
model's two mutants apart."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import follow_model as FM
import lanefit_model as LM
from unet_lane_detection_amd import _lib, state as S
from unet_lane_detection_amd import follow as F
from unet_lane_detection_amd import lanefit as LF
from unet_lane_detection_amd import ros_bridge as RB

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 64
INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=False)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Buf:
    """`size` device bytes at byte `lead` of a larger buffer filled with a canary: lead = 64 keeps the view 64-byte
    aligned, lead = 65 puts it one byte off; at least 64 canary bytes on either side.  Without data the view itself
    holds the canary."""

    def __init__(self, size, lead=GUARD, data=None):
        self.whole = torch.full((lead + size + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.view = self.whole[lead:lead + size]
        self.lead, self.size = lead, size
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1).view(np.uint8)))

    def numpy(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        w = self.whole.cpu().numpy()
        return bool((w[:self.lead] == CANARY).all() and (w[self.lead + self.size:] == CANARY).all())


def run_fit(lib, masks, level, n_windows, margin, min_pixels, prior=None, lead=GUARD):
    """-> (n, 2, 16) uint64.  The output starts out as the canary, so a word the kernel left alone shows; guards and
    inputs are checked after the call."""
    n, h, w = masks.shape
    mk = Buf(masks.size, lead, masks)
    out = Buf(n * 2 * 16 * 8, GUARD)              # the words themselves stay 8-byte aligned
    pr = None
    if prior is not None:
        assert prior.dtype == np.int32 and prior.shape == (n, 2, h)
        pr = Buf(prior.nbytes, GUARD, prior)      # ... and the table 4-byte aligned
    rc = lib.unet_lane_fit_u8_batch(0, _p(mk.view), n, h, w, level, n_windows, margin, min_pixels,
                                    _p(pr.view) if pr is not None else None, _p(out.view), None)
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    assert out.guards_intact() and mk.guards_intact() and (pr is None or pr.guards_intact())
    assert np.array_equal(mk.numpy(), masks.reshape(-1))
    assert pr is None or np.array_equal(pr.numpy().view(np.int32), prior.reshape(-1))
    return out.numpy().view(np.uint64).reshape(n, 2, 16)


def check(lib, masks, level, n_windows, margin, min_pixels, prior=None, leads=(GUARD, GUARD + 1), what=""):
    ref = LM.records(masks, level, n_windows, margin, min_pixels, prior)
    for lead in leads:
        got = run_fit(lib, masks, level, n_windows, margin, min_pixels, prior, lead)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (f"{what} shape {masks.shape} level {level} n_windows {n_windows} margin {margin} min_pixels "
                               f"{min_pixels} lead {lead} {'prior' if prior is not None else 'window'}: (frame, lane, word) "
                               f"{bad[:6].tolist()} got {[int(got[tuple(b)]) for b in bad[:6]]} want {[int(ref[tuple(b)]) for b in bad[:6]]}")
    return ref


def contents(n, h, w):
    rng = np.random.default_rng(LM.painted_seed(n, h, w))
    return {"zeros": np.zeros((n, h, w), np.uint8), "full": np.full((n, h, w), 255, np.uint8),
            "random": rng.integers(0, 256, (n, h, w), dtype=np.uint8),
            "painted": LM.painted_lanes(LM.painted_seed(n, h, w), n, h, w)}


SHAPES = [(1, 1, 1), (2, 1, 40), (2, 40, 1), (3, 37, 53), (2, 90, 131), (2, 64, 256), (1, 685, 1055)]
MARGINS, LEVELS, MIN_PIXELS = (1, 6, 100, 512), (0, 127, 254, 255), (0, 3, 50)


def window_counts(h):
    return sorted({k for k in (1, 5, 9, min(h, 64)) if k <= h})


# ---- window mode -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w", SHAPES)
def test_window_mode_against_the_model(lib, n, h, w):
    """every n_windows x margin on every content; level and min_pixels cycle through their values so that each meets
    each content and margin somewhere; the base pointer alternates between aligned and one byte off (both on the
    painted masks).  The large frame takes a diagonal of that grid."""
    big = h * w > 100000
    k = 0
    for name, masks in contents(n, h, w).items():
        for i, nw in enumerate(window_counts(h)):
            for j, margin in enumerate(MARGINS):
                if big and (i + j) % 4 != (0 if name in ("painted", "random") else 1):
                    continue
                level, minpix = LEVELS[(k + j) % 4], MIN_PIXELS[(k + i) % 3]
                leads = (GUARD, GUARD + 1) if name == "painted" else ((GUARD, GUARD + 1)[k % 2],)
                check(lib, masks, level, nw, margin, minpix, leads=leads, what=name)
                k += 1
        k += 1
    painted = contents(n, h, w)["painted"]
    for level in LEVELS:                                   # the default search at every level
        check(lib, painted, level, min(9, h), 100, 50, what="painted")
    if big:                                                # the whole frame in both lanes' windows
        check(lib, contents(n, h, w)["full"], 127, 9, 512, 50, leads=(GUARD + 1,), what="full")


def test_crafted_windows(lib):
    """exactly min_pixels and min_pixels + 1 pixels in a window, an ON pixel at x == c + margin, windows clipped at
    both borders (tests/test_lanefit_cpu.py: each mutant of the model gives other records here)"""
    mask, kw = LM.crafted()
    ref = check(lib, mask, kw["level"], kw["n_windows"], kw["margin"], kw["min_pixels"], what="crafted")
    for mutant in (dict(closed_upper=True), dict(recentre_ge=True)):
        assert not np.array_equal(LM.records(mask, **kw, **mutant), ref)
    table = np.full((1, 2, 40), -1, dtype=np.int32)
    table[0, 0, 12] = 5                                    # the band [-1, 11) of row 12: the pixel at 11 is outside
    check(lib, mask, kw["level"], kw["n_windows"], kw["margin"], 0, prior=table, what="crafted")


def test_sum_bound_and_width_bound(lib):
    """(1, 2048, 64) of 255 with margin 512: every pixel in both lanes, the largest S_4 a 64-column frame can give
    (64 sum y^4 = 0.025 * 2^64; the header derives 0.4 * 2^64 for 1024 columns), in both modes; (1, 8, 8192): the whole
    histogram in LDS, windows at either end of a row"""
    tall = np.full((1, 2048, 64), 255, np.uint8)
    for nw in (1, 64):
        ref = check(lib, tall, 127, nw, 512, 50, leads=(GUARD + 1,), what="tall")
    assert int(ref[0, 0, 9]) == int(ref[0, 1, 9]) == 64 * sum(y ** 4 for y in range(2048))
    check(lib, tall, 254, 64, 512, 50, prior=np.full((1, 2, 2048), 32, np.int32), leads=(GUARD + 1,), what="tall")
    rng = np.random.default_rng(8)
    wide = rng.integers(0, 256, (1, 8, 8192), dtype=np.uint8)
    edge = np.zeros((1, 8, 8192), np.uint8)
    edge[0, 3:, :3] = 200
    edge[0, 4:, 8189:] = 200
    edge[0, :3, 40:60] = 129
    for masks, name in ((wide, "wide random"), (edge, "wide edges"), (LM.painted_lanes(5, 1, 8, 8192), "wide painted")):
        for nw, margin, level in ((1, 512, 127), (8, 100, 128), (5, 6, 0)):
            check(lib, masks, level, nw, margin, 3, what=name)
    table = np.stack([np.full((1, 8), 2, np.int32), np.full((1, 8), 8191, np.int32)], axis=1)
    check(lib, edge, 127, 1, 512, 0, prior=table, what="wide edges")


# ---- prior mode ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w", SHAPES)
def test_prior_mode_against_the_model(lib, n, h, w):
    c = contents(n, h, w)
    painted = c["painted"]
    fitted = LM.prior_table(LM.records(painted, 127, min(9, h), 100, 50), h)          # the model's own fits
    ys = np.arange(h)
    outside = np.empty((n, 2, h), np.int32)
    outside[:, 0] = np.resize(np.array([-2, -1000, INT_MIN, 0, w - 1, w // 2], np.int32), h)
    outside[:, 1] = np.resize(np.array([w, w + 1, w + 5, w + 99, w + 100, w + 511, w + 512, w + 10 ** 6, INT_MAX - 1], np.int32), h)
    split = np.full((n, 2, h), -1, np.int32)
    split[:, 0, ys % 2 == 0] = w // 3                       # the left lane on even rows, the right one on the top half
    split[:, 1, : (h + 1) // 2] = (2 * w) // 3
    tables = {"fitted": fitted, "none": np.full((n, 2, h), -1, np.int32), "outside": outside,
              "int_max": np.full((n, 2, h), INT_MAX, np.int32), "split": split}
    big = h * w > 100000
    k = 0
    for tname, table in tables.items():
        for j, margin in enumerate(MARGINS):
            for name in ("painted", "random", "full", "zeros"):
                if name in ("full", "zeros") and (big or tname in ("none", "int_max")) and j != k % 4:
                    continue
                level = LEVELS[(k + j) % 4]
                leads = (GUARD, GUARD + 1) if (name == "painted" and not big) else ((GUARD, GUARD + 1)[k % 2],)
                ref = check(lib, c[name], level, min(9, h), margin, 50, prior=table, leads=leads, what=f"{name}/{tname}")
                k += 1
                if tname == "none":                        # nothing searched: the record of a lane that is not there
                    assert not ref[:, :, :13].any() and (ref[:, :, 13] == h).all() and not ref[:, :, 14:].any()
    # what the tables are there to show
    ref = LM.records(painted, 127, 1, 100, 50, prior=tables["int_max"])
    assert (ref[:, :, 3] == h).all() and not ref[:, :, 2].any() and (ref[:, :, 0] == 1).all()
    ref = LM.records(c["full"], 127, 1, 100, 50, prior=tables["outside"])
    assert int(ref[0, 1, 5]) > 0 or w == 1                  # a prior beyond the right border still reaches into the image
    ref = LM.records(c["full"], 127, 1, 6, 50, prior=split)
    assert int(ref[0, 0, 3]) == (h + 1) // 2 and int(ref[0, 1, 3]) == (h + 1) // 2


# ---- the Python layer ------------------------------------------------------------------------------------------

def test_records_fits_and_tracker_on_a_sequence():
    n, h, w = 3, 90, 131
    cfg = LF.FitConfig(margin=12, min_pixels=6)
    frames = LM.painted_lanes(LM.painted_seed(n, h, w), n, h, w)
    dev = torch.from_numpy(frames).cuda()
    rec = LF.lane_fit_records(dev, cfg)
    assert rec.is_cuda and rec.dtype == torch.int64 and tuple(rec.shape) == (n, 2, 16)
    ref = LM.records(frames, cfg.level, cfg.n_windows, cfg.margin, cfg.min_pixels)
    assert np.array_equal(rec.cpu().numpy().view(np.uint64), ref)
    fits = LF.LaneFits.from_records(rec.cpu().numpy(), h, w, cfg)
    table = LF.prior_table(fits, h)
    assert np.array_equal(table, LM.prior_table(ref, h))
    for i in range(n):
        for lane, words in zip(fits[i].lanes, ref[i]):
            assert lane.coeffs == LM.coeffs_of(words) and lane.confidence == LM.confidence(words)
    assert fits[0].left.coeffs is not None and fits[0].right.coeffs is not None and isinstance(fits[0].center_px(60), int)
    # prior mode through the Python layer, table from numpy and from a device tensor; a 2-d mask is one frame
    rec_p = LF.lane_fit_records(dev, cfg, prior=table).cpu().numpy().view(np.uint64)
    assert np.array_equal(rec_p, LM.records(frames, cfg.level, cfg.n_windows, cfg.margin, cfg.min_pixels, prior=table))
    one = LF.lane_fit_records(dev[1], cfg, prior=torch.from_numpy(table[1:2]).cuda()).cpu().numpy().view(np.uint64)
    assert np.array_equal(one, rec_p[1:2])
    assert np.array_equal(LF.lane_fits(dev, cfg).words, ref)
    with pytest.raises(TypeError):
        LF.lane_fit_records(torch.from_numpy(frames), cfg)
    with pytest.raises(ValueError):
        LF.lane_fit_records(dev, cfg, prior=table[:1])
    with pytest.raises(_lib.UnetError, match="margin"):
        LF.lane_fit_records(dev, LF.FitConfig(margin=513))
    # the tracker: window, prior, prior on an empty mask (which loses the lanes), window again
    sequence = [frames[0], frames[1], np.zeros((h, w), np.uint8), frames[0]]
    tracker, model = LF.LaneTracker(cfg), LM.Tracker(cfg.level, cfg.n_windows, cfg.margin, cfg.min_pixels)
    for mask in sequence:
        got = tracker.update(torch.from_numpy(mask).cuda())
        mode, want = model.update(mask)
        assert tracker.mode == mode and np.array_equal(got.words, want)
    assert tracker.modes == ["window", "prior", "prior", "window"]
    assert got[0].left.coeffs is not None


# ---- the pipeline ----------------------------------------------------------------------------------------------

def _message(img_bgr, pitch_pad=16):
    h, w = img_bgr.shape[:2]
    step = w * 3 + pitch_pad
    rows = np.zeros((h, step), dtype=np.uint8)
    rows[:, :w * 3] = img_bgr.reshape(h, w * 3)
    return RB.ImageMsg(height=h, width=w, encoding="bgr8", data=rows.tobytes(), step=step, header="hdr")


@pytest.fixture(scope="module")
def messages(golden_dir):
    """the two messages of tests/test_follow_gpu.py: the committed real frame in the lower middle of a 480 x 640 bgr8
    message, and one painted frame"""
    real = np.fromfile(os.path.join(golden_dir, "frame_001410_rgb_u8.bin"), dtype=np.uint8).reshape(224, 224, 3)
    img = np.full((480, 640, 3), 40, dtype=np.uint8)
    img[240:464, 208:432] = real[..., ::-1]
    painted = FM.painted_frames(5, 1, 480, 640)[0][0]
    return [("real", _message(img)), ("painted", _message(painted))]


SCAN_ROWS = [120, 300, int(685 * 0.7), 640]


def _pipeline_case(messages, make):
    cfg = LF.FitConfig()
    plain, fitted, both = make(), make(fit=cfg), make(fit=cfg, diagnose=True)
    model, model_both = LM.Tracker(), LM.Tracker()
    for name, msg in messages:
        want_centres, want_mask = plain.process(msg, return_mask=True)
        (centres, got_mask), fits = fitted.process(msg, return_mask=True)
        assert centres == want_centres and got_mask.data == want_mask.data, name        # as with fit=None
        mask = np.frombuffer(got_mask.data, dtype=np.uint8).reshape(got_mask.height, got_mask.width)
        assert mask.shape == (685, 1055)
        mode, want = model.update(mask)
        assert isinstance(fits, LF.LaneFits) and len(fits) == 1 and (fits.height, fits.width) == (685, 1055)
        assert fitted.tracker.mode == mode and np.array_equal(fits.words, want), name
        for lane, words in zip(fits[0].lanes, want[0]):
            assert lane.coeffs == LM.coeffs_of(words)
        # with diagnose the (result, fits) pair is the first element of the existing pair
        out = both.process(msg)
        assert isinstance(out, tuple) and len(out) == 2 and len(out[0]) == 2
        (centres_d, fits_d), stats = out
        assert centres_d == want_centres and np.array_equal(fits_d.words, model_both.update(mask)[1])
        assert type(stats).__name__ == "FrameStats" and len(stats) == 1
        assert plain.process(msg) == want_centres
        lanes = fits[0]
        print(f"{name}: mode {mode}, pixels {lanes.left.pixels} / {lanes.right.pixels}, confidence "
              f"{lanes.left.confidence:.2f} / {lanes.right.confidence:.2f}, centre at row 479: {lanes.center_px(479)}")
    assert plain.tracker is None and fitted.tracker.modes[0] == "window"


def test_follow_pipeline_with_fit_unet(messages):
    from unet_lane_detection_amd.model import UNetHIP
    net = UNetHIP(S.seeded_state_dict([8, 16], seed=4), device=0)
    kw = dict(threshold=0.5, input_size=(224, 224), precision="fp32")
    _pipeline_case(messages, lambda **extra: F.LaneFollowPipeline(net, source="unet", scan_rows=SCAN_ROWS, **extra, **kw))
    net.release()


def test_follow_pipeline_with_fit_hsv(messages):
    _pipeline_case(messages, lambda **extra: F.LaneFollowPipeline(None, source="hsv", scan_rows=SCAN_ROWS, **extra))
