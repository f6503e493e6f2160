"""Lane instances on the GPU (csrc/label_kernels.cpp through the C ABI, unet_lane_detection_amd/instances.py and
follow.LaneFollowPipeline(clean=...)) against tests/label_model.py: every comparison is bit-exact and covers the whole
label map, all header words and all 16 words of every record.  Every buffer, the workspace included, lies between
canaries; the mask pointer is both 64-byte aligned and one byte off; inputs are verified unmodified.
tests/test_label_cpu.py holds the model to scipy.ndimage on these very cases and shows that the contents tell the
model's mutants apart.  Parity with cv2's label numbering is unpinned."""
import ctypes as C

import numpy as np
import pytest
import torch

import follow_model as FM
import label_model as M
from unet_lane_detection_amd import _lib
from unet_lane_detection_amd import follow as F
from unet_lane_detection_amd import instances as I
from unet_lane_detection_amd import lanefit as LF
from unet_lane_detection_amd import ros_bridge as RB

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 64


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
            self.view.copy_(torch.from_numpy(np.array(data).reshape(-1).view(np.uint8)))    # a copy: the contents are read-only

    def numpy(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        w = self.whole.cpu().numpy()
        return bool((w[:self.lead] == CANARY).all() and (w[self.lead + self.size:] == CANARY).all())


class Labelled:
    """one call of unet_label_u8_batch: the device buffers (kept for a keep call) and the results on the host"""

    def __init__(self, lib, masks, level, conn, cap, lead=GUARD, stream=None):
        n, h, w = masks.shape
        self.shape, self.cap, self.masks = (n, h, w), cap, masks
        self.mk = Buf(masks.size, lead, masks)
        self.lab = Buf(n * h * w * 4)
        self.head = Buf(n * 4 * 8)
        self.rec = Buf(n * cap * 16 * 8)
        wb = lib.unet_label_work_bytes(n, h, w)
        assert wb > 0
        self.work = Buf(wb)
        torch.cuda.synchronize()
        rc = lib.unet_label_u8_batch(0, _p(self.mk.view), n, h, w, level, conn, _p(self.lab.view), cap, _p(self.head.view),
                                     _p(self.rec.view), _p(self.work.view), wb, stream)
        assert rc == 0, lib.unet_op_last_error()
        torch.cuda.synchronize()
        for b in (self.mk, self.lab, self.head, self.rec, self.work):
            assert b.guards_intact()
        assert np.array_equal(self.mk.numpy(), masks.reshape(-1))
        self.labels = self.lab.numpy().view(np.int32).reshape(n, h, w)
        self.header = self.head.numpy().view(np.uint64).reshape(n, 4)
        self.records = self.rec.numpy().view(np.uint64).reshape(n, cap, 16)


def assert_equal(got, ref, what):
    """got: Labelled; ref: the model's (labels, header, records)"""
    labels, header, records = ref
    bad = np.argwhere(got.header != header)
    assert bad.size == 0, f"{what}: header (frame, word) {bad[:4].tolist()} got {got.header[tuple(bad[0])]} want {header[tuple(bad[0])]}"
    bad = np.argwhere(got.labels != labels)
    assert bad.size == 0, (f"{what}: {len(bad)} label(s) differ, first (frame, y, x) {bad[:4].tolist()} got "
                           f"{[int(got.labels[tuple(b)]) for b in bad[:4]]} want {[int(labels[tuple(b)]) for b in bad[:4]]}")
    bad = np.argwhere(got.records != records)
    assert bad.size == 0, (f"{what}: record (frame, component - 1, word) {bad[:6].tolist()} got "
                           f"{[int(got.records[tuple(b)]) for b in bad[:6]]} want {[int(records[tuple(b)]) for b in bad[:6]]}")


# ---- the labelling against the model ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w", M.SHAPES)
def test_label_against_the_model(lib, n, h, w):
    """every case of label_model.cases (its docstring says which): all contents, both connectivities, levels 0 / 127 /
    254 / 255, caps 1 / 7 / 1024 (K > cap among them: the checkerboard, the diagonal and the random masks with 4).  The
    mask pointer alternates between aligned and one byte off, and is both on the two kinds of painted masks."""
    truncated = 0
    for k, (name, level, conn, cap) in enumerate(M.cases(n, h, w)):
        ref = M.reference(name, n, h, w, level, conn, cap)
        leads = (GUARD, GUARD + 1) if name in ("painted", "lanes") else ((GUARD, GUARD + 1)[k % 2],)
        for lead in leads:
            got = Labelled(lib, M.content(name, n, h, w), level, conn, cap, lead)
            assert_equal(got, ref, f"{name} shape {(n, h, w)} level {level} connectivity {conn} cap {cap} lead {lead}")
        if int(ref[1][0, 0]) > cap:
            truncated += 1
            assert int(ref[1][0, 2]) == cap and not ref[2][0, cap:].any() and int(ref[0][0].max()) == int(ref[1][0, 0])
    assert truncated > 0 or h * w == 1


def test_large_frame_closed_form(lib):
    """one full 2048 x 2048 frame: K = 1, the largest sums the domain allows (S_4 = 0.8 * 2^64), no model run"""
    h = w = 2048
    got = Labelled(lib, np.full((1, h, w), 200, np.uint8), 127, 4, 3, GUARD + 1)
    assert got.header[0].tolist() == [1, h * w, 1, 0]
    assert (got.labels == 1).all()
    assert [int(v) for v in got.records[0, 0]] == M.full_frame_record(h, w)
    assert int(got.records[0, 0, 9]) == 14739386724520034304 and not got.records[0, 1:].any()


def test_batch_equals_single_frames_and_repeats(lib):
    n, h, w = 3, 37, 53
    masks = np.stack([M.content("random41", n, h, w)[0], M.content("painted", n, h, w)[1], M.content("spiral", n, h, w)[2]])
    for conn in (4, 8):
        both = Labelled(lib, masks, 127, conn, 64)
        assert_equal(both, M.label(masks, 127, conn, 64), f"mixed batch, connectivity {conn}")
        for i in range(n):
            one = Labelled(lib, masks[i:i + 1], 127, conn, 64, GUARD + 1)
            assert np.array_equal(one.labels[0], both.labels[i]) and np.array_equal(one.header[0], both.header[i])
            assert np.array_equal(one.records[0], both.records[i])
    big = M.content("random59", 2, 150, 200)
    a, b = Labelled(lib, big, 127, 4, 1024), Labelled(lib, big, 127, 4, 1024)
    assert a.lab.numpy().tobytes() == b.lab.numpy().tobytes() and a.rec.numpy().tobytes() == b.rec.numpy().tobytes()
    assert a.head.numpy().tobytes() == b.head.numpy().tobytes()


def test_non_default_stream(lib):
    n, h, w = 2, 150, 200
    stream = torch.cuda.Stream()
    got = Labelled(lib, M.content("painted", n, h, w), 127, 8, 1024, GUARD + 1, stream=C.c_void_p(stream.cuda_stream))
    ref = M.reference("painted", n, h, w, 127, 8, 1024)
    assert_equal(got, ref, "non-default stream")
    table, mask = run_keep(lib, got, dict(min_area=64), stream=C.c_void_p(stream.cuda_stream))
    want = M.keep(*ref, 1024, min_area=64)
    assert np.array_equal(table, want[0]) and np.array_equal(mask, want[1])


# ---- the filter ------------------------------------------------------------------------------------------------

def run_keep(lib, got, kw, lead=GUARD, in_place=False, stream=None):
    """unet_keep_components_u8_batch on the buffers of a Labelled -> (keep (n, cap), mask (n, h, w)); with in_place the
    mask goes over the source mask"""
    n, h, w = got.shape
    keep = Buf(n * got.cap, lead)
    out = got.mk if in_place else Buf(n * h * w, lead)
    rc = lib.unet_keep_components_u8_batch(0, _p(got.lab.view), n, h, w, _p(got.head.view), _p(got.rec.view), got.cap,
                                           kw.get("min_area", 0), kw.get("min_height", 0), kw.get("min_width", 0),
                                           kw.get("keep_largest", 0), _p(keep.view), _p(out.view), stream)
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    for b in (keep, out, got.lab, got.head, got.rec):
        assert b.guards_intact()
    assert np.array_equal(got.lab.numpy().view(np.int32).reshape(n, h, w), got.labels)        # inputs unmodified
    assert np.array_equal(got.rec.numpy().view(np.uint64).reshape(n, got.cap, 16), got.records)
    assert np.array_equal(got.head.numpy().view(np.uint64).reshape(n, 4), got.header)
    return keep.numpy().reshape(n, got.cap), out.numpy().reshape(n, h, w)


@pytest.mark.parametrize("n,h,w", [(2, 1, 40), (3, 37, 53), (2, 150, 200)])
def test_keep_against_the_model(lib, n, h, w):
    """the table and the mask over min_area 0 / 1 / 64 / hw, min_height, min_width and keep_largest 0 / 1 / 2 / 5; the
    checkerboard with 4 (every area 1) and the random masks have equal-area ties, and the checkerboard has components
    beyond the cap, which are dropped"""
    hw = h * w
    grid = [dict(), dict(min_area=1), dict(min_area=64), dict(min_area=hw), dict(min_height=3), dict(min_width=4),
            dict(min_height=2, min_width=2, min_area=5), dict(keep_largest=1), dict(keep_largest=2), dict(keep_largest=5),
            dict(keep_largest=2, min_area=2), dict(keep_largest=5, min_width=2), dict(keep_largest=2000)]
    k = 0
    for name, conn, cap in (("checker", 4, 7), ("random05", 8, 1024), ("random41", 4, 1024), ("painted", 8, 1024),
                            ("full", 4, 1), ("zeros", 8, 7), ("rings", 8, 1024)):
        ref = M.reference(name, n, h, w, 127, conn, cap)
        got = Labelled(lib, M.content(name, n, h, w), 127, conn, cap, (GUARD, GUARD + 1)[k % 2])
        assert_equal(got, ref, name)
        for kw in grid:
            want = M.keep(*ref, cap, **kw)
            table, mask = run_keep(lib, got, kw, (GUARD, GUARD + 1)[k % 2])
            assert np.array_equal(table, want[0]), (name, kw, np.argwhere(table != want[0])[:5].tolist())
            assert np.array_equal(mask, want[1]), (name, kw, np.argwhere(mask != want[1])[:5].tolist())
            k += 1
        if name == "checker":                               # ties: the two lowest ids win; beyond the cap: dropped
            table, mask = run_keep(lib, got, dict(keep_largest=2))
            assert table[0].tolist() == [1, 1, 0, 0, 0, 0, 0]
            table, mask = run_keep(lib, got, dict())
            assert int(ref[1][0, 0]) > cap and np.array_equal(mask == 255, (ref[0] > 0) & (ref[0] <= cap))
    # in place: the mask goes over the bytes the labels were computed from
    ref = M.reference("painted", n, h, w, 127, 8, 1024)
    for lead in (GUARD, GUARD + 1):
        got = Labelled(lib, M.content("painted", n, h, w), 127, 8, 1024, lead)
        table, mask = run_keep(lib, got, dict(min_area=64 if hw > 1000 else 3), in_place=True)
        want = M.keep(*ref, 1024, min_area=64 if hw > 1000 else 3)
        assert np.array_equal(table, want[0]) and np.array_equal(mask, want[1])


def test_keep_with_the_largest_cap(lib):
    """cap 65536 and more components than that with records of one pixel each: the selection among 65536 equal areas"""
    n, h, w = 1, 300, 600
    masks = np.where((np.add.outer(np.arange(h), np.arange(w)) % 2) == 0, 255, 0).astype(np.uint8)[None]
    got = Labelled(lib, masks, 127, 4, 65536)
    assert got.header[0].tolist() == [h * w // 2, h * w // 2, 65536, 0]
    ref = M.label(masks, 127, 4, 65536)
    assert_equal(got, ref, "checkerboard, cap 65536")
    for kw in (dict(keep_largest=3), dict(keep_largest=40000), dict(keep_largest=65536), dict(min_area=2)):
        table, mask = run_keep(lib, got, kw)
        want = M.keep(*ref, 65536, **kw)
        assert np.array_equal(table, want[0]) and np.array_equal(mask, want[1]), kw


# ---- the Python layer ------------------------------------------------------------------------------------------

def test_label_clean_and_lane_instances():
    n, h, w = 2, 150, 200
    masks = M.content("painted", n, h, w)
    dev = torch.from_numpy(np.array(masks)).cuda()
    ref = M.reference("painted", n, h, w, 127, 8, 1024)
    comp = I.label(dev)
    assert comp.labels.is_cuda and comp.labels.dtype == torch.int32 and np.array_equal(comp.labels.cpu().numpy(), ref[0])
    assert np.array_equal(comp.header, ref[1]) and comp.count == [int(v) for v in ref[1][:, 0]]
    m = comp.records.shape[1]
    assert m == max(comp.count) and np.array_equal(comp.records, ref[2][:, :m]) and comp.truncated == [False, False]
    key = (0, int(torch.cuda.current_stream().cuda_stream), n, h, w)
    work = I._WORK[key]
    four = I.label(dev, connectivity=4, max_components=7)
    assert I._WORK[key] is work                              # the workspace is kept for the shape and stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # another stream gets a workspace of its own
        other = I.label(dev)
    side.synchronize()
    assert I._WORK[(0, int(side.cuda_stream), n, h, w)] is not work and np.array_equal(other.labels.cpu().numpy(), ref[0])
    for k in range(I._WORK_SLOTS + 2):                       # ... and the cache is bounded
        I.label(dev[:1, :8 + k, :8])
    assert len(I._WORK) <= I._WORK_SLOTS
    r4 = M.reference("painted", n, h, w, 127, 4, 7)
    assert np.array_equal(four.labels.cpu().numpy(), r4[0]) and np.array_equal(four.records, r4[2]) and four.truncated == [True, True]
    one = I.label(dev[1])                                    # a 2-d mask is one frame
    assert len(one) == 1 and np.array_equal(one.labels.cpu().numpy()[0], ref[0][1])
    cfg = I.CleanConfig(min_area=64)
    mask, comp2, keep = I.clean(dev, cfg)
    want = M.keep(*ref, 1024, min_area=64)
    assert mask.is_cuda and mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), want[1])
    assert np.array_equal(keep.cpu().numpy(), want[0]) and np.array_equal(comp2.header, ref[1])
    assert np.array_equal(dev.cpu().numpy(), masks)          # the input is left as it is
    frames = I.lane_instances(dev, cfg)
    host = I.instances_of(I.Components(None, ref[1], ref[2], h, w), want[0])
    assert len(frames) == n
    for got_f, want_f in zip(frames, host):
        assert len(got_f) == 3                               # three markings, left to right
        xs = [s.x_at(h - 1) for s in got_f]
        assert xs == sorted(xs) and [abs(x - b * w) < 0.04 * w for x, b in zip(xs, (0.15, 0.45, 0.75))] == [True] * 3
        assert [(s.id, s.area, s.bbox, s.confidence, s.fit.coeffs) for s in got_f] == \
               [(s.id, s.area, s.bbox, s.confidence, s.fit.coeffs) for s in want_f]
        assert max(s.confidence for s in got_f) == 1.0 and all(isinstance(s.fit, LF.LaneFit) for s in got_f)
    with pytest.raises(TypeError):
        I.label(torch.from_numpy(np.array(masks)))
    with pytest.raises(_lib.UnetError, match="connectivity"):
        I.label(dev, connectivity=6)
    with pytest.raises(_lib.UnetError, match="min_area"):
        I.clean(dev, I.CleanConfig(min_area=-1))


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


def test_follow_pipeline_with_clean():
    """the node's own mask size.  Without clean the speckle counts in every scan row; with it the centres are those of
    the model's cleaned mask, which is also what return_mask gives"""
    h, w = 685, 1055
    speckled = M.content("painted", 1, h, w)[0]
    msg = _message(FM.painted_frames(5, 1, 480, 640)[0][0])
    cfg = I.CleanConfig(min_area=64)

    def make(**extra):
        return F.LaneFollowPipeline(None, source="hsv", extractor=FixedMask(speckled), scan_rows=SCAN_ROWS, **extra)
    plain, none, cleaned = make(), make(clean=None), make(clean=cfg)
    want_plain = FM.lane_centers(speckled[None], SCAN_ROWS)[0]
    centres, mask_msg = plain.process(msg, return_mask=True)
    assert centres == want_plain and mask_msg.data == speckled.tobytes() and plain.last_components is None
    # clean=None: byte-identical to a pipeline built without the argument
    centres_n, mask_n = none.process(msg, return_mask=True)
    assert centres_n == centres and mask_n.data == mask_msg.data and (mask_n.height, mask_n.width) == (h, w)
    assert none.process(msg) == plain.process(msg) and none.last_components is None
    ref = M.reference("painted", 1, h, w, 127, 8, 1024)
    table, want_mask = M.keep(*ref, 1024, min_area=64)
    want_clean = FM.lane_centers(want_mask, SCAN_ROWS)[0]
    centres_c, mask_c = cleaned.process(msg, return_mask=True)
    assert centres_c == want_clean and mask_c.data == want_mask[0].tobytes() and (mask_c.height, mask_c.width) == (h, w)
    assert cleaned.process(msg) == want_clean                     # the return shape is unchanged
    comp = cleaned.last_components
    assert isinstance(comp, I.Components) and np.array_equal(comp.header, ref[1]) and comp.count[0] > 3
    assert int(table.sum()) == 3
    # the speckle moved a centre, and no longer does: the cleaned centres are those of the three markings alone
    moved = [r for r, a, b in zip(SCAN_ROWS, want_plain, want_clean) if a != b]
    print(f"scan rows {SCAN_ROWS}: centres {want_plain} with the speckle, {want_clean} cleaned; K = {comp.count[0]}")
    assert moved
    # with a fit the cleaned mask is what is fitted, and the pair's shape is as without clean
    fitted = make(clean=cfg, fit=LF.FitConfig())
    (centres_f, mask_f), fits = fitted.process(msg, return_mask=True)
    assert centres_f == want_clean and mask_f.data == mask_c.data and isinstance(fits, LF.LaneFits)
    import lanefit_model as LM
    assert np.array_equal(fits.words, LM.Tracker().update(want_mask[0])[1])


def test_follow_pipeline_hsv_with_clean():
    """the real extractor in front: the cleaned mask is the model's filter of the plain pipeline's mask"""
    msg = _message(FM.painted_frames(5, 1, 480, 640)[0][0])
    cfg = I.CleanConfig(min_area=200, keep_largest=4)
    plain = F.LaneFollowPipeline(None, source="hsv", scan_rows=SCAN_ROWS)
    cleaned = F.LaneFollowPipeline(None, source="hsv", scan_rows=SCAN_ROWS, clean=cfg)
    _, mask_msg = plain.process(msg, return_mask=True)
    mask = np.frombuffer(mask_msg.data, dtype=np.uint8).reshape(1, mask_msg.height, mask_msg.width)
    ref = M.label(mask, 127, 8, 1024)
    table, want_mask = M.keep(*ref, 1024, min_area=200, keep_largest=4)
    centres, got = cleaned.process(msg, return_mask=True)
    assert got.data == want_mask[0].tobytes() and centres == FM.lane_centers(want_mask, SCAN_ROWS)[0]
    assert np.array_equal(cleaned.last_components.header, ref[1])
