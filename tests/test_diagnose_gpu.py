"""The diagnostics on the GPU (csrc/diagnose_kernels.cpp through the C ABI, unet_lane_detection_amd/diagnose.py)
against tests/diagnose_model.py: every record is compared bit for bit.  Parity against cv2 itself is unpinned (see the
model's header).  tests/test_diagnose_cpu.py shows that the frames used here tell a wrong border rule, counted padding,
exchanged channels and a 32-bit sum of squares apart.  Every output buffer starts filled with a canary, so a record
that comes out right was written whole by the call."""
import ctypes as C

import numpy as np
import pytest
import torch

import diagnose_model as DM
from unet_lane_detection_amd import _lib, state as S
from unet_lane_detection_amd import diagnose as D

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 64


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=False)


def _p(t):
    return C.c_void_p(t.data_ptr())


class Buf:
    """`size` device bytes at byte `lead` of a larger buffer filled with a canary: lead = 64 keeps the view 64-byte
    aligned, lead = 65 puts it one byte off; at least 64 canary bytes on either side."""

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


def run_frames(lib, data, n, h, w, stride, bgr, lead=GUARD, out=None):
    """data: the frames' bytes as they lie in memory (dense frames or raw rows whose last row may end with its pixels)"""
    fr = Buf(data.size, lead, data)
    out = Buf(n * 64) if out is None else out
    rc = lib.unet_frame_stats_u8_batch(0, _p(fr.view), n, h, w, stride, 1 if bgr else 0, _p(out.view), None)
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    assert out.guards_intact() and fr.guards_intact()
    assert np.array_equal(fr.numpy(), np.ascontiguousarray(data).reshape(-1))
    return out.numpy().view(np.uint64).reshape(n, 8)


def run_probs(lib, scores, threshold, lead=GUARD, out=None):
    n, numel = scores.shape
    sc = Buf(scores.size * 4, lead, scores)
    out = Buf(n * 32) if out is None else out
    rc = lib.unet_prob_stats_f32_batch(0, _p(sc.view), n, numel, threshold, _p(out.view), None)
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    assert out.guards_intact() and sc.guards_intact()
    assert np.array_equal(sc.numpy(), scores.reshape(-1).view(np.uint8))
    return out.numpy().view(np.uint64).reshape(n, 4)


# ---- frames ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w", DM.FRAME_CASES)
def test_frame_stats_against_the_model(lib, n, h, w):
    """BGR and RGB, from an aligned base pointer and from one a byte off"""
    frames = DM.make_frames(DM.frames_seed(n, h, w), n, h, w)
    for bgr in (True, False):
        ref = DM.frame_records(frames, bgr)
        for lead in (GUARD, GUARD + 1):
            got = run_frames(lib, frames, n, h, w, 0, bgr, lead)
            assert np.array_equal(got, ref), f"({n},{h},{w}) bgr {bgr} lead {lead}:\n{got}\n{ref}"
    assert np.array_equal(run_frames(lib, frames, n, h, w, 3 * w, True), DM.frame_records(frames))   # the dense stride, spelled out


def test_frame_stats_with_a_row_stride(lib):
    """rows of 21 pixel bytes and 5 bytes of padding set to 255: the padding is neither counted nor read as pixels; the
    buffer ends with the last row's pixels, and with the whole last row"""
    (n, h, w), stride = DM.PADDED_CASE
    frames = DM.make_frames(DM.frames_seed(n, h, w), n, h, w)
    rows = DM.padded_rows(frames, stride)
    ref = DM.frame_records(rows, width=w)
    assert np.array_equal(ref, DM.frame_records(frames))
    flat = rows.reshape(-1)
    for lead in (GUARD, GUARD + 1):
        for data in (flat, flat[:flat.size - (stride - 3 * w)]):
            assert np.array_equal(run_frames(lib, data, n, h, w, stride, True, lead), ref), (lead, data.size)
    # a wider frame with a stride that is no multiple of anything: (2, 40, 300) in rows of 1003 bytes
    n, h, w, stride = 2, 40, 300, 1003
    frames = DM.make_frames(5, n, h, w)
    rows = DM.padded_rows(frames, stride)
    assert np.array_equal(run_frames(lib, rows.reshape(-1), n, h, w, stride, False), DM.frame_records(frames, False))


def test_frame_stats_on_hand_made_frames(lib):
    for value in (0, 255):
        frames = np.full((2, 33, 255, 3), value, dtype=np.uint8)
        got = run_frames(lib, frames, 2, 33, 255, 0, True)
        assert got.tolist() == [[value, value, value * 33 * 255 * 3, 0, 0, 0, 0, 0]] * 2
    board = DM.checkerboard(256, 256)
    got = run_frames(lib, board, 1, 256, 256, 0, True)
    assert got.tolist() == [[0, 255, 255 * 3 * 256 * 128, 0, 256 * 256 * 1020 * 1020, 0, 0, 0]]
    assert np.array_equal(got, DM.frame_records(board))


def test_a_second_call_overwrites_the_records(lib):
    out = Buf(3 * 64)
    a = DM.make_frames(1, 3, 40, 50)
    b = DM.make_frames(2, 3, 20, 300)
    first = run_frames(lib, a, 3, 40, 50, 0, True, out=out).copy()
    second = run_frames(lib, b, 3, 20, 300, 0, True, out=out)
    assert np.array_equal(first, DM.frame_records(a)) and np.array_equal(second, DM.frame_records(b))
    pout = Buf(2 * 32)
    rng = np.random.default_rng(0)
    p, q = rng.random((2, 1000), dtype=np.float32), rng.random((2, 77), dtype=np.float32)
    assert np.array_equal(run_probs(lib, p, 0.5, out=pout), DM.prob_records(p, 0.5))
    assert np.array_equal(run_probs(lib, q, 0.25, out=pout), DM.prob_records(q, 0.25))


# ---- probability planes ------------------------------------------------------------------------------------------

def _planes(seed, n, numel):
    """mostly probabilities, some values outside [0, 1], exact 0 and 1, a few NaNs"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, numel), dtype=np.float32)
    p = np.where(rng.random((n, numel)) < 0.1, rng.normal(0.5, 1.0, (n, numel)).astype(np.float32), p)
    p = np.where(rng.random((n, numel)) < 0.05, np.float32(1.0), p)
    p = np.where(rng.random((n, numel)) < 0.05, np.float32(0.0), p)
    return np.where(rng.random((n, numel)) < 0.01, np.float32(np.nan), p).astype(np.float32)


@pytest.mark.parametrize("n,numel", [(3, 67 * 131), (4, 1), (2, 5), (1, 300 * 700)])
def test_prob_stats_against_the_model(lib, n, numel):
    p = _planes(numel + n, n, numel)
    for thr in (0.5, 0.0, float(p[0, 0]) if not np.isnan(p[0, 0]) else 0.3):
        ref = DM.prob_records(p, thr)
        for lead in (GUARD, GUARD + 4, GUARD + 12):       # 16-byte aligned and not
            got = run_probs(lib, p, thr, lead)
            assert np.array_equal(got, ref), f"({n},{numel}) threshold {thr} lead {lead}:\n{got}\n{ref}"


def test_prob_stats_on_special_values(lib):
    v = DM.special_values(0.5)[None]
    want = [(0x7F800000 << 32) | 0xFF800000, 4, (1 << 32) + 256 + 3 * (1 << 32), 1]
    assert run_probs(lib, v, 0.5).tolist() == [want]
    assert np.array_equal(run_probs(lib, v, 0.5, GUARD + 4), DM.prob_records(v, 0.5))
    for thr in (float("inf"), float("-inf"), 1.0):
        assert np.array_equal(run_probs(lib, v, thr), DM.prob_records(v, thr))
    zeros = np.array([[0.0, -0.0], [-0.0, 0.0]], dtype=np.float32)
    assert run_probs(lib, zeros, 0.0).tolist() == [[0x80000000, 0, 0, 0]] * 2
    nans = np.full((2, 1001), np.nan, dtype=np.float32)
    assert run_probs(lib, nans, 0.5).tolist() == [[(0xFF800000 << 32) | 0x7F800000, 0, 0, 1001]] * 2
    ones = np.ones((1, 1 << 20), dtype=np.float32)
    assert run_probs(lib, ones, 0.5).tolist() == [[(0x3F800000 << 32) | 0x3F800000, 1 << 20, 1 << 52, 0]]


# ---- the Python layer --------------------------------------------------------------------------------------------

def test_frame_stats_and_output_stats_objects():
    n, h, w = 3, 67, 131
    frames = DM.make_frames(DM.frames_seed(n, h, w), n, h, w)
    ref = DM.frame_records(frames)
    for given in (frames, torch.from_numpy(frames), torch.from_numpy(frames).cuda()):
        st = D.frame_stats(given)
        assert np.array_equal(st.words, ref) and len(st) == n
    assert np.array_equal(D.frame_stats(frames[0], bgr=False).words, DM.frame_records(frames[:1], False))
    assert st.mean.tolist() == [DM.frame_mean(r, h, w) for r in ref]
    assert st.sharpness.tolist() == [DM.frame_sharpness(r, h, w) for r in ref]
    assert not st.blurry.any() and len(st.report(1)) == 6
    rows = DM.padded_rows(frames, 3 * w + 7)
    assert np.array_equal(D.frame_stats(rows, row_stride=3 * w + 7, width=w).words, ref)
    dark = D.frame_stats(np.full((1, 8, 8, 3), 20, np.uint8))
    assert dark.too_dark[0] and dark.blurry[0] and not dark.overexposed[0]
    p = _planes(9, 2, 32 * 32).reshape(2, 1, 32, 32)
    for given in (p, torch.from_numpy(p).cuda()):
        out = D.output_stats(given, 0.4)
        assert np.array_equal(out.words, DM.prob_records(p, 0.4)) and out.numel == 1024
    assert out.nan_count.tolist() == np.isnan(p).sum(axis=(1, 2, 3)).tolist() and len(out.report(0)) == 3


def test_dataset_report():
    from unet_lane_detection_amd.augment import DeviceDataset
    rng = np.random.default_rng(2)
    images = DM.make_frames(3, 7, 32, 48)
    images[1] = 20                                              # dark and flat
    images[4] = 240                                             # overexposed and flat
    images[5] = rng.integers(100, 104, (32, 48, 3))             # neither, but without contrast
    ds = DeviceDataset(images, np.zeros((7, 32, 48), np.uint8))
    rep = D.dataset_report(ds, batch=3)
    assert (rep["frames"], rep["too_dark"], rep["overexposed"], rep["blurry"]) == (7, 1, 1, 3)
    assert (rep["too_dark_idx"], rep["overexposed_idx"], rep["blurry_idx"]) == ([1], [4], [1, 4, 5])
    assert np.array_equal(rep["stats"].words, DM.frame_records(images, bgr=False))


@pytest.fixture(scope="module")
def small_model():
    from unet_lane_detection_amd.model import UNetHIP
    model = UNetHIP(S.seeded_state_dict([8, 16], seed=4), device=0)
    yield model
    model.release()


def test_frame_pipeline_with_diagnose(small_model):
    from unet_lane_detection_amd import video as V
    kw = dict(threshold=0.5, input_size=(32, 32), precision="fp32")
    plain, diag = V.FramePipeline(small_model, **kw), V.FramePipeline(small_model, diagnose=True, **kw)
    frames = DM.make_frames(21, 5, 45, 61)
    overlay, mask = plain.process(frames)
    (overlay_d, mask_d), stats = diag.process(frames)
    assert torch.equal(overlay, overlay_d) and torch.equal(mask, mask_d)
    assert np.array_equal(stats.words, D.frame_stats(frames).words)
    assert np.array_equal(stats.words, DM.frame_records(frames)) and (stats.height, stats.width) == (45, 61)
    chunks = [frames[0:2], frames[2:5]]
    want = list(plain.run(chunks))
    got = list(diag.run(chunks))
    for c, (w_ov, w_mk), ((g_ov, g_mk), st) in zip(chunks, want, got):
        assert np.array_equal(w_ov, g_ov) and np.array_equal(w_mk, g_mk)
        assert np.array_equal(st.words, DM.frame_records(c))
    count, _ = V.predict_video(diag, list(frames), lambda f: None, chunk=2)
    assert count == 5


def test_follow_pipeline_with_diagnose():
    from unet_lane_detection_amd import follow as F
    from unet_lane_detection_amd import ros_bridge as RB
    import follow_model as FM
    img = FM.painted_frames(5, 1, 480, 640)[0][0]
    h, w = img.shape[:2]
    step = 3 * w + 16
    rows = np.full((h, step), 255, dtype=np.uint8)
    rows[:, :3 * w] = img.reshape(h, 3 * w)
    msg = RB.ImageMsg(height=h, width=w, encoding="bgr8", data=rows.tobytes(), step=step, header="hdr")
    scan = [120, 300, int(685 * 0.7), 640]
    plain = F.LaneFollowPipeline(None, source="hsv", scan_rows=scan)
    diag = F.LaneFollowPipeline(None, source="hsv", scan_rows=scan, diagnose=True)
    want = plain.process(msg)
    got, stats = diag.process(msg)
    assert got == want and any(c is not None for c in got)
    assert np.array_equal(stats.words, DM.frame_records(img[None])) and (stats.height, stats.width) == (h, w)
    (centres, out), stats2 = diag.process(msg, return_mask=True)
    assert centres == want and out.data == plain.process(msg, return_mask=True)[1].data
    assert np.array_equal(stats2.words, stats.words)
    rgb = RB.ImageMsg(height=h, width=w, encoding="rgb8", data=rows.tobytes(), step=step, header="hdr")
    assert np.array_equal(diag.process(rgb)[1].words, DM.frame_records(img[None], bgr=False))


def test_quick_test_equals_output_stats():
    from unet_lane_detection_amd.model import UNetHIP
    model = UNetHIP(S.seeded_state_dict([4, 8], seed=3), device=0)
    frames = S.synthetic_frames(3, 32, 32, seed=2)
    for thr in (0.5, 0.45):
        stats, mask = D.quick_test(model, frames, threshold=thr, precision="fp32")
        _, probs = model.run_u8(torch.from_numpy(frames).cuda(), return_probs=True, precision="fp32")
        direct = D.output_stats(probs, thr)
        assert np.array_equal(stats.words, direct.words)
        assert np.array_equal(stats.words, DM.prob_records(probs.cpu().numpy(), thr))
        counts = (mask.cpu().numpy() == 255).reshape(3, -1).sum(axis=1)
        print(f"threshold {thr}: share above {stats.share_above}, mean {stats.mean}, range {stats.min} .. {stats.max}")
        assert (stats.share_above * stats.numel).tolist() == counts.tolist()
        assert stats.numel == 32 * 32 and stats.nan_count.tolist() == [0, 0, 0]
    model.release()
