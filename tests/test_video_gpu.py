"""The video path on the GPU (csrc/video_kernels.cpp through the C ABI, unet_lane_detection_amd/video.py) against
tests/video_model.py: every comparison is bit-exact.  The model restates OpenCV's 8-bit resize and an fp32 addWeighted;
parity against cv2 itself is unpinned (see the model's header)."""
import ctypes as C

import numpy as np
import pytest
import torch

import video_model as VM
from oracle import camera_oracle as CO
from oracle import unet_oracle as O
from unet_lane_detection_amd import _lib, state as S
from unet_lane_detection_amd import video as V

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


def run_overlay(lib, frames, masks, lut, alpha, beta, gamma, want_mask, lead=GUARD):
    n, h, w, _ = frames.shape
    fr, mk = Buf(frames.size, lead, frames), Buf(masks.size, lead, masks)
    out = Buf(frames.size, lead)
    mo = Buf(n * h * w, lead) if want_mask else None
    table = np.ascontiguousarray(lut, dtype=np.uint8).copy()
    rc = lib.unet_overlay_u8_batch(0, _p(fr.view), n, h, w, _p(mk.view), masks.shape[1], masks.shape[2],
                                   table.ctypes.data_as(C.c_void_p), alpha, beta, gamma, _p(out.view),
                                   _p(mo.view) if mo else None, None)
    table[:] = 0   # consumed before the call returned
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    assert out.guards_intact() and (mo is None or mo.guards_intact())
    assert np.array_equal(fr.numpy(frames.shape), frames) and np.array_equal(mk.numpy(masks.shape), masks)
    return out.numpy(frames.shape), (mo.numpy((n, h, w)) if mo else None)


def run_resize(lib, src, out_w, out_h, swap, lead=GUARD):
    n, h, w = src.shape[:3]
    cn = 1 if src.ndim == 3 else src.shape[3]
    shape = (n, out_h, out_w) if src.ndim == 3 else (n, out_h, out_w, cn)
    s, d = Buf(src.size, lead, src), Buf(int(np.prod(shape)), lead)
    rc = lib.unet_resize_u8_batch(0, _p(s.view), n, h, w, cn, 1 if swap else 0, out_w, out_h, _p(d.view), None)
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    assert d.guards_intact()
    return d.numpy(shape)


def lane_masks(rng, n, h, w):
    """binary 0/255 masks of a random field at 30 % density"""
    return ((rng.random((n, h, w)) < 0.3) * 255).astype(np.uint8)


# ---- overlay ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("abg", [(0.7, 0.3, 0.0), (0.45, 0.8, -20.5)])
def test_overlay_all_byte_pairs(lib, abg):
    """every (frame byte, mask value) pair, with a table that is no ramp; the second setting saturates at both ends"""
    x = np.arange(256, dtype=np.uint8)
    frames = np.ascontiguousarray(np.broadcast_to(x[None, None, :, None], (1, 256, 256, 3)))
    masks = np.ascontiguousarray(np.broadcast_to(x[None, :, None], (1, 256, 256)))
    lut = np.stack([x, 255 - x, x ^ 0x55], axis=1).astype(np.uint8)
    ref, ref_m = VM.overlay_batch(frames, masks, lut, *abg)
    assert np.array_equal(ref_m, masks)
    if abg[2] < 0:
        assert ref.min() == 0 and ref.max() == 255
    got, got_m = run_overlay(lib, frames, masks, lut, *abg, want_mask=True)
    assert np.array_equal(got_m, masks)
    bad = int((got != ref).sum())
    assert bad == 0, f"{bad} of {ref.size} overlay bytes differ"


# (n, mask (h, w), frame (H, W)): rows of 183 bytes and 8,235 pixels, no multiple of 16; a downscale; runs that span
# several rows and an image boundary
SHAPES = [(3, (32, 32), (45, 61)), (2, (48, 64), (30, 40)), (2, (8, 8), (17, 5))]


@pytest.mark.parametrize("n,msize,fsize", SHAPES)
@pytest.mark.parametrize("lead", [GUARD, GUARD + 1], ids=["aligned", "one_byte_off"])
def test_overlay_shapes(lib, n, msize, fsize, lead):
    rng = np.random.default_rng(100 * n + fsize[0])
    frames = rng.integers(0, 256, size=(n,) + fsize + (3,), dtype=np.uint8)
    masks = lane_masks(rng, n, *msize)
    lut = V.jet_table()
    ref, ref_m = VM.overlay_batch(frames, masks, lut, 0.7, 0.3, 0.0)
    assert np.array_equal(ref_m, np.stack([CO.resize_linear(m, fsize[1], fsize[0]) for m in masks]))
    if msize[0] < fsize[0] and n == 3:
        assert len(np.unique(ref_m)) > 200   # the upscaled mask is not binary
    got, got_m = run_overlay(lib, frames, masks, lut, 0.7, 0.3, 0.0, want_mask=True, lead=lead)
    assert np.array_equal(got_m, ref_m)
    assert np.array_equal(got, ref)
    alone, none = run_overlay(lib, frames, masks, lut, 0.7, 0.3, 0.0, want_mask=False, lead=lead)
    assert none is None and np.array_equal(alone, got)


# ---- batched resize --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,out,swap", [((3, 45, 61, 3), (32, 32), True), ((2, 30, 40, 3), (64, 48), False),
                                            ((4, 31, 17), (17, 31), False)])
@pytest.mark.parametrize("lead", [GUARD, GUARD + 1], ids=["aligned", "one_byte_off"])
def test_resize_batch(lib, shape, out, swap, lead):
    """out = (width, height); the last case keeps the size, which is a copy"""
    from unet_lane_detection_amd.ros_bridge import CameraStage
    rng = np.random.default_rng(shape[1])
    src = rng.integers(0, 256, size=shape, dtype=np.uint8)
    got = run_resize(lib, src, out[0], out[1], swap, lead=lead)
    assert np.array_equal(got, VM.resize_batch(src, out[0], out[1], swap_rb=swap))
    stage = CameraStage(0)
    for img, g in zip(src, got):
        one = np.ascontiguousarray(img[..., ::-1]) if swap else img
        assert np.array_equal(g, stage.resize(torch.from_numpy(one), out).cpu().numpy())


def test_resize_batch_swap_of_a_copy(lib):
    """equal sizes with the colour swap: the bytes of every pixel are exchanged on the 16-byte path and in the tail"""
    src = np.random.default_rng(5).integers(0, 256, size=(2, 9, 7, 3), dtype=np.uint8)
    assert np.array_equal(run_resize(lib, src, 7, 9, True), src[..., ::-1])


# ---- argument checks -------------------------------------------------------------------------------------------

def test_video_abi_rejects_bad_arguments(lib):
    src = torch.full((2, 8, 8, 3), 9, dtype=torch.uint8, device="cuda")
    dst = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device="cuda")
    msk = torch.zeros((2, 4, 4), dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(src)
    lut = V.jet_table()
    lp = lut.ctypes.data_as(C.c_void_p)
    nan = float("nan")

    def refused(rc):
        return rc != 0 and len(lib.unet_op_last_error()) > 0

    rs, ov = lib.unet_resize_u8_batch, lib.unet_overlay_u8_batch
    assert refused(rs(0, None, 2, 8, 8, 3, 0, 4, 4, _p(dst), None))             # null pointers
    assert refused(rs(0, _p(src), 2, 8, 8, 3, 0, 4, 4, None, None))
    assert refused(rs(0, _p(src), 0, 8, 8, 3, 0, 4, 4, _p(dst), None))          # n = 0
    assert refused(rs(0, _p(src), 2, 8, 8, 2, 0, 4, 4, _p(dst), None))          # channels = 2
    assert rs(0, _p(src), 2, 8, 8, 1, 1, 4, 4, _p(dst), None) == 1              # swap_rb with one channel: INVALID_ARG
    assert b"swap_rb" in lib.unet_op_last_error()
    assert refused(rs(0, _p(src), 2, 8, 8, 3, 0, 0, 4, _p(dst), None))          # a zero output size
    assert refused(rs(0, _p(src), 2, 8, 8, 3, 0, 4, 0, _p(dst), None))
    assert refused(ov(0, None, 2, 8, 8, _p(msk), 4, 4, lp, 0.7, 0.3, 0.0, _p(out), None, None))
    assert refused(ov(0, _p(src), 2, 8, 8, None, 4, 4, lp, 0.7, 0.3, 0.0, _p(out), None, None))
    assert refused(ov(0, _p(src), 2, 8, 8, _p(msk), 4, 4, None, 0.7, 0.3, 0.0, _p(out), None, None))
    assert refused(ov(0, _p(src), 2, 8, 8, _p(msk), 4, 4, lp, 0.7, 0.3, 0.0, None, None, None))
    assert refused(ov(0, _p(src), 0, 8, 8, _p(msk), 4, 4, lp, 0.7, 0.3, 0.0, _p(out), None, None))
    assert refused(ov(0, _p(src), 2, 8, 0, _p(msk), 4, 4, lp, 0.7, 0.3, 0.0, _p(out), None, None))
    assert refused(ov(0, _p(src), 2, 8, 8, _p(msk), 4, 4, lp, nan, 0.3, 0.0, _p(out), None, None))   # NaN alpha
    torch.cuda.synchronize()
    assert not dst.any() and not out.any()   # nothing was launched
    # valid calls afterwards
    assert rs(0, _p(src), 2, 8, 8, 3, 1, 4, 4, _p(dst), None) == 0
    assert ov(0, _p(src), 2, 8, 8, _p(msk), 4, 4, lp, 0.7, 0.3, 0.0, _p(out), None, None) == 0
    torch.cuda.synchronize()


# ---- the pipeline ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_model():
    from unet_lane_detection_amd.model import UNetHIP
    sdn = S.seeded_state_dict([8, 16], seed=4)
    model = UNetHIP(sdn, device=0)
    yield sdn, model
    model.release()


def test_pipeline_against_the_oracle(small_model):
    """frames -> overlay and mask against oracle resize -> oracle network -> threshold -> the model's overlay.  Pixels
    that a small-mask pixel within 1e-4 of the threshold reaches are left out; they must stay below 1 %."""
    sdn, model = small_model
    pipe = V.FramePipeline(model, threshold=0.5, input_size=(32, 32), precision="fp32")
    frames = np.random.default_rng(11).integers(0, 256, (3, 45, 61, 3)).astype(np.uint8)
    overlay, mask = pipe.process(frames)
    assert overlay.shape == (3, 45, 61, 3) and mask.shape == (3, 45, 61) and overlay.is_cuda and mask.is_cuda
    small = VM.resize_batch(frames, 32, 32, swap_rb=True)
    with torch.no_grad():
        logits = O.forward(O.to_torch_state(sdn), O.normalize_u8_nhwc(small))[:, 0].numpy()
    prob = 1.0 / (1.0 + np.exp(-logits))
    lane = (prob > 0.5).astype(np.uint8) * 255
    ref, ref_m = VM.overlay_batch(frames, lane, V.jet_table(), 0.7, 0.3, 0.0)
    unsure = VM.resize_batch((np.abs(prob - 0.5) < 1e-4).astype(np.uint8) * 255, 61, 45) > 0
    print(f"lane share of the small mask {lane.mean() / 255:.3f}, pixels left out {unsure.mean():.4%}")
    assert unsure.mean() < 0.01
    assert np.array_equal(mask.cpu().numpy()[~unsure], ref_m[~unsure])
    assert np.array_equal(overlay.cpu().numpy()[~unsure], ref[~unsure])
    # the same frames from the device
    again, _ = pipe.process(torch.from_numpy(frames).cuda())
    assert torch.equal(again, overlay)


def test_run_streams_chunks_in_order(small_model):
    _, model = small_model
    pipe = V.FramePipeline(model, input_size=(32, 32), precision="fp32")
    frames = np.random.default_rng(12).integers(0, 256, (7, 45, 61, 3)).astype(np.uint8)
    chunks = [frames[0:3], frames[3:6], frames[6:7]]
    want = [tuple(t.cpu().numpy() for t in pipe.process(c)) for c in chunks]
    gen = pipe.run(iter(chunks))
    first = next(gen)
    kept = (first[0].copy(), first[1].copy())
    rest = list(gen)
    got = [first] + rest
    assert len(got) == 3
    for (o, m), (wo, wm) in zip(got, want):
        assert isinstance(o, np.ndarray) and isinstance(m, np.ndarray)
        assert np.array_equal(o, wo) and np.array_equal(m, wm)
    assert np.array_equal(first[0], kept[0]) and np.array_equal(first[1], kept[1])
    # more chunks than staging slots, sizes that change: still in order, still each chunk's own result
    many = [frames[i:i + 1 + (i % 2)] for i in range(0, 6)]
    for c, (o, m) in zip(many, pipe.run(many)):
        wo, wm = pipe.process(c)
        assert np.array_equal(o, wo.cpu().numpy()) and np.array_equal(m, wm.cpu().numpy())
    assert list(pipe.run([])) == []


def test_pipeline_on_the_int8_tier():
    from unet_lane_detection_amd import quant
    from unet_lane_detection_amd.int8 import UNetInt8, calibrate
    from unet_lane_detection_amd.model import UNetHIP
    sdn = S.seeded_state_dict([32, 64, 128], seed=0)
    fm = UNetHIP(sdn, device=0)
    ranges = calibrate(fm, torch.from_numpy(S.synthetic_frames(6, 64, 64, seed=1)), batch=4)
    fm.release()
    net = UNetInt8(quant.quantize_model(sdn, ranges), device=0)
    pipe = V.FramePipeline(net, input_size=(64, 64))
    assert pipe.precision is None
    frames = np.random.default_rng(13).integers(0, 256, (2, 90, 70, 3)).astype(np.uint8)
    overlay, mask = pipe.process(frames)
    small = VM.resize_batch(frames, 64, 64, swap_rb=True)
    own = net.run_u8(torch.from_numpy(small).cuda(), return_mask=True)[-1].cpu().numpy()
    ref, ref_m = VM.overlay_batch(frames, own, V.jet_table(), 0.7, 0.3, 0.0)
    assert np.array_equal(mask.cpu().numpy(), ref_m) and np.array_equal(overlay.cpu().numpy(), ref)
    (o, m), = list(pipe.run([frames]))
    assert np.array_equal(o, ref) and np.array_equal(m, ref_m)
    net.release()
