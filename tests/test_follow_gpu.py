"""Lane following on the GPU (csrc/follow_kernels.cpp through the C ABI, unet_lane_detection_amd/follow.py) against
tests/follow_model.py: every comparison is bit-exact.  The model's HSV plane is augment.rgb_to_hsv; parity against cv2
itself is unpinned (see the model's header).  tests/test_follow_cpu.py shows that the painted frames used here tell a
wrong border rule apart."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import follow_model as FM
from unet_lane_detection_amd import _lib, metrics, state as S
from unet_lane_detection_amd import follow as F
from unet_lane_detection_amd import ros_bridge as RB
from unet_lane_detection_amd.augment import rgb_to_hsv

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 64


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=False)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Buf:
    """`size` device bytes at byte `lead` of a larger buffer filled with a canary: lead = 64 keeps the view 64-byte
    aligned, lead = 65 puts it one byte off; at least 64 canary bytes on either side."""

    def __init__(self, size, lead=GUARD, data=None):
        self.whole = torch.full((lead + size + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.view = self.whole[lead:lead + size]
        self.lead, self.size = lead, size
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)))

    def numpy(self, shape):
        return self.view.cpu().numpy().reshape(shape)

    def guards_intact(self):
        w = self.whole.cpu().numpy()
        return bool((w[:self.lead] == CANARY).all() and (w[self.lead + self.size:] == CANARY).all())


def run_hsv(lib, frames, kc, ko, bgr, lower=FM.DEFAULT_LOWER, upper=FM.DEFAULT_UPPER, lead=GUARD):
    n, h, w, _ = frames.shape
    fr, out = Buf(frames.size, lead, frames), Buf(n * h * w, lead)
    lo, hi = np.array(lower, dtype=np.uint8), np.array(upper, dtype=np.uint8)
    rc = lib.unet_hsv_lanes_u8_batch(0, _p(fr.view), n, h, w, 1 if bgr else 0, lo.ctypes.data_as(C.c_void_p),
                                     hi.ctypes.data_as(C.c_void_p), kc, ko, _p(out.view), None)
    lo[:] = 0   # consumed before the call returned
    hi[:] = 0
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    assert out.guards_intact() and fr.guards_intact()
    assert np.array_equal(fr.numpy(frames.shape), frames)
    return out.numpy((n, h, w))


def run_center(lib, masks, rows, level, lead=GUARD):
    n, h, w = masks.shape
    mk = Buf(masks.size, lead, masks)
    out = Buf(n * len(rows) * 8, GUARD)     # the words themselves stay 4-byte aligned
    arr = (C.c_int * len(rows))(*rows)
    rc = lib.unet_lane_center_u8_batch(0, _p(mk.view), n, h, w, arr, len(rows), level, _p(out.view), None)
    for j in range(len(rows)):
        arr[j] = -1   # consumed before the call returned
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    assert out.guards_intact() and mk.guards_intact()
    assert np.array_equal(mk.numpy(masks.shape), masks)
    return out.numpy((n * len(rows) * 8,)).view(np.uint32).reshape(n, len(rows), 2).astype(np.int64)


# ---- the extractor ---------------------------------------------------------------------------------------------

# more than one tile in either direction ((2,200,300): 232-column and 64-row tiles at (5,5), 4 x 2 tiles), rows of 393
# and 210 bytes, and the degenerate ones
SHAPES = [(3, 67, 131), (2, 64, 256), (1, 130, 70), (2, 200, 300), (2, 5, 9), (2, 1, 40), (2, 40, 1), (1, 1, 1)]
KSIZES = [(5, 5), (3, 7), (7, 3), (1, 5), (5, 1), (1, 1)]


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_extractor_against_the_model(lib, n, h, w):
    frames, _ = FM.painted_frames(FM.painted_seed(n, h, w), n, h, w)
    for bgr in (0, 1):
        plane = FM.in_range(frames, bgr=bool(bgr))
        for kc, ko in KSIZES:
            ref = np.stack([FM.close_open(p, kc, ko) for p in plane])
            for lead in (GUARD, GUARD + 1):
                got = run_hsv(lib, frames, kc, ko, bgr, lead=lead)
                bad = int((got != ref).sum())
                assert bad == 0, f"{bad} of {ref.size} mask bytes differ: ksize ({kc},{ko}), is_bgr {bgr}, lead {lead}"
                assert set(np.unique(got)) <= {0, 255}


@pytest.mark.parametrize("lower,upper", [((20, 50, 50), (100, 255, 255)), ((0, 0, 255), (0, 0, 255))],
                         ids=["hue_window", "lower_equals_upper"])
def test_extractor_with_other_bounds(lib, lower, upper):
    """a hue window that wraps nothing, on random colours, and lower == upper, which only pure white passes"""
    n, h, w = 3, 67, 131
    rng = np.random.default_rng(7)
    frames, field = FM.painted_frames(FM.painted_seed(n, h, w), n, h, w)
    frames = frames.copy()
    frames[field & (rng.random(field.shape) < 0.7)] = 255          # pure white: H = 0, S = 0, V = 255
    share = float((FM.in_range(frames, lower, upper) == 255).mean())
    assert 0.05 < share < 0.6, share
    for kc, ko in ((5, 5), (3, 7)):
        for lead in (GUARD, GUARD + 1):
            ref = FM.hsv_lanes(frames, lower, upper, kc, ko, bgr=True)
            assert np.array_equal(run_hsv(lib, frames, kc, ko, 1, lower, upper, lead=lead), ref)


def test_in_range_on_colour_coverage(lib):
    """inRange alone (k = 1, 1).  Not all 2^24 colours: all colours with two channels free and the third stepped by 5,
    once per stepped channel from the offsets 0, 1 and 2 - 3 x 52 x 65,536 pixels, about 3 s with the model.  Every
    value of diff and of V, the hue boundaries 0 and 179 and both sides of S = 40 | 41 and V = 184 | 185 occur."""
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    other = ((11, 42, 0), (170, 255, 184))     # the complement in S and V, a hue window inside [0, 180)
    values = set()
    for ch in range(3):
        steps = np.arange(ch, 256, 5, dtype=np.uint8)
        planes = [None, None, None]
        planes[ch] = np.broadcast_to(steps[:, None, None], (steps.size, 256, 256))
        planes[(ch + 1) % 3] = np.broadcast_to(a[None], (steps.size, 256, 256))
        planes[(ch + 2) % 3] = np.broadcast_to(b[None], (steps.size, 256, 256))
        rgb = np.ascontiguousarray(np.stack(planes, axis=-1))
        hsv = rgb_to_hsv(rgb)
        i64 = rgb.astype(np.int64)
        diff = i64.max(axis=-1) - i64.min(axis=-1)
        assert np.unique(diff).size == 256
        values |= set(np.unique(hsv[..., 2]).tolist())
        assert np.unique(hsv[..., 0]).size == 180 and hsv[..., 0].min() == 0 and hsv[..., 0].max() == 179
        for c, v in ((1, 40), (1, 41), (2, 184), (2, 185)):
            assert (hsv[..., c] == v).any()
        for lower, upper in ((FM.DEFAULT_LOWER, FM.DEFAULT_UPPER), other):
            ref = FM.in_range_hsv(hsv, lower, upper)
            assert 0 < int((ref == 255).sum()) < ref.size
            got = run_hsv(lib, rgb, 1, 1, 0, lower, upper)
            bad = int((got != ref).sum())
            assert bad == 0, f"{bad} of {ref.size} colours differ, stepped channel {ch}, bounds {lower} {upper}"
    assert len(values) == 256     # V = 0 needs the stepped channel at 0: the first of the three sets
    # is_bgr on one slice: the same colours read the other way round
    assert np.array_equal(run_hsv(lib, rgb[:4], 1, 1, 1), FM.in_range(rgb[:4], bgr=True))


# ---- the lane centre -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [1, 10, 11, 12, 63, 64, 65, 1055, 7680])
def test_lane_center_against_the_model(lib, width):
    """masks: random bytes, all 0, all 255, a binary mask resized bilinearly (any byte value), sparse; rows 0 and h-1
    alone and 64 rows in one call; an aligned base and one a byte off (with odd widths the rows are unaligned anyway)"""
    from oracle.camera_oracle import resize_linear
    h = 6
    rng = np.random.default_rng(width)
    small = ((rng.random((3, max(width // 5, 1))) < 0.4) * 255).astype(np.uint8)
    sparse = np.zeros((h, width), dtype=np.uint8)
    sparse[:, rng.choice(width, min(width, 11), replace=False)] = 128
    masks = np.stack([rng.integers(0, 256, (h, width), dtype=np.uint8), np.zeros((h, width), np.uint8),
                      np.full((h, width), 255, np.uint8), resize_linear(small, width, h), sparse])
    if width >= 63:
        assert np.unique(masks[3]).size > 2
    many = [0, h - 1] + [int(r) for r in rng.integers(0, h, 62)]
    for rows in ([0], [h - 1], many):
        for level in (0, 127, 254, 255):
            ref = FM.lane_sums(masks, rows, level)
            for lead in (GUARD, GUARD + 1):
                got = run_center(lib, masks, rows, level, lead=lead)
                assert np.array_equal(got, ref), (width, len(rows), level, lead)
    # the Python layer: default row, the "more than 10" rule, counts and sums read back
    dev = torch.from_numpy(masks).cuda()
    assert F.lane_centers(dev) == FM.lane_centers(masks)
    assert F.lane_centers(dev, scan_rows=many, level=200, min_pixels=0) == FM.lane_centers(masks, many, 200, 0)
    if width == 7680:
        assert F.lane_centers(dev)[2] == [(width - 1) // 2]
    if width == 10:
        assert F.lane_centers(dev)[2] == [None] and F.lane_centers(dev, min_pixels=9)[2] == [4]


# ---- the pipeline ----------------------------------------------------------------------------------------------

def _message(img_bgr, pitch_pad=16):
    h, w = img_bgr.shape[:2]
    step = w * 3 + pitch_pad
    rows = np.zeros((h, step), dtype=np.uint8)
    rows[:, :w * 3] = img_bgr.reshape(h, w * 3)
    return RB.ImageMsg(height=h, width=w, encoding="bgr8", data=rows.tobytes(), step=step, header="hdr")


@pytest.fixture(scope="module")
def messages(golden_dir):
    """the committed real frame in the lower middle of a 480 x 640 bgr8 message, and one painted frame"""
    real = np.fromfile(os.path.join(golden_dir, "frame_001410_rgb_u8.bin"), dtype=np.uint8).reshape(224, 224, 3)
    img = np.full((480, 640, 3), 40, dtype=np.uint8)
    img[240:464, 208:432] = real[..., ::-1]
    painted = FM.painted_frames(5, 1, 480, 640)[0][0]
    return {"real": (img, _message(img)), "painted": (painted, _message(painted))}


SCAN_ROWS = [120, 300, int(685 * 0.7), 640]


@pytest.mark.parametrize("precision,feats,input_size", [("fp32", [8, 16], (224, 224)), ("f16x3", [64, 128], (56, 40))])
def test_follow_pipeline_unet(messages, precision, feats, input_size):
    from unet_lane_detection_amd.model import UNetHIP
    model = UNetHIP(S.seeded_state_dict(feats, seed=4), device=0)
    kw = dict(threshold=0.5, input_size=input_size, precision=precision)
    plain = RB.LanePipelineGPU(model, **kw)
    follow = F.LaneFollowPipeline(model, source="unet", scan_rows=SCAN_ROWS, **kw)
    default = F.LaneFollowPipeline(model, source="unet", **kw)
    for name, (_, msg) in messages.items():
        want = plain.process(msg)
        mask = np.frombuffer(want.data, dtype=np.uint8).reshape(want.height, want.width)
        centres, got = follow.process(msg, return_mask=True)
        assert (got.height, got.width, got.encoding, got.step, got.header) == (685, 1055, "mono8", 1055, "hdr")
        assert got.data == want.data, name
        assert centres == FM.lane_centers(mask[None], SCAN_ROWS)[0], name
        assert follow.process(msg) == centres
        assert default.process(msg) == FM.lane_centers(mask[None])[0]
        print(f"{precision} {name}: lane share {float((mask > 127).mean()):.3f}, centres {centres}")
    model.release()


def test_follow_pipeline_hsv(messages):
    follow = F.LaneFollowPipeline(None, source="hsv", scan_rows=SCAN_ROWS)
    stage = RB.CameraStage(0)
    seen = []
    for name, (img, msg) in messages.items():
        warped = stage.prestage(torch.from_numpy(img), follow.matrix, RB.REF_WARP_SIZE, RB.REF_WARP_SIZE).cpu().numpy()
        assert warped.shape == (685, 1055, 3)
        mask = FM.hsv_lanes(warped[None], bgr=False)
        centres, out = follow.process(msg, return_mask=True)
        assert np.array_equal(np.frombuffer(out.data, dtype=np.uint8).reshape(685, 1055), mask[0]), name
        assert centres == FM.lane_centers(mask, SCAN_ROWS)[0], name
        print(f"hsv {name}: lane share {float((mask > 127).mean()):.3f}, centres {centres}")
        seen += centres
    assert any(c is not None for c in seen)
    # a PID step on what came out, as the reference's callback does
    pid = F.LineFollower()
    cmds = [pid.update(c, 1055) for c in seen]
    assert all((cmd is None) == (c is None) for cmd, c in zip(cmds, seen))


def test_extractor_evaluate_equals_the_model_sweep():
    n, h, w = 3, 67, 131
    frames, field = FM.painted_frames(FM.painted_seed(n, h, w), n, h, w)
    ext = F.HSVLaneExtractor()
    assert np.array_equal(ext.extract(frames).cpu().numpy(), FM.hsv_lanes(frames))
    assert np.array_equal(ext.extract(torch.from_numpy(frames[0]), bgr=False).cpu().numpy(), FM.hsv_lanes(frames[:1], bgr=False))
    scores = (FM.hsv_lanes(frames).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    for targets in (field.astype(np.float32)[:, None], (field * 255).astype(np.uint8)):
        sw = ext.evaluate(frames, targets, batch=2)              # two batches accumulate
        assert isinstance(sw, metrics.ThresholdSweep) and len(sw) == 1 and sw.pixels == n * h * w
        assert np.array_equal(sw.counts, metrics.sweep_model(scores, targets, [0.5]))
        at = sw.at(0.5)
        assert 0.3 < at["iou"] < 1.0 and at["tp"] + at["fn"] == int(field.sum())
    with pytest.raises(ValueError):
        F.HSVLaneExtractor(close_ksize=4)
