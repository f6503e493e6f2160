"""The video path's host side: the default colour table's pins, that tests/video_model.py tells the blend's look-alikes
apart (so a kernel that contracts, rounds half up or computes in float64 cannot pass tests/test_video_gpu.py), and
predict_video's loop."""
import hashlib

import numpy as np

import video_model as VM
from unet_lane_detection_amd import video as V


def test_jet_table_pins():
    lut = V.jet_table()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert tuple(lut[0]) == (128, 0, 0) and tuple(lut[255]) == (0, 0, 128)
    assert int(lut.astype(np.int64).sum()) == 93760
    assert hashlib.sha256(lut.tobytes()).hexdigest().startswith("67b2eede4f90d505")
    # the formula itself, entry by entry in plain integers
    for i in (0, 1, 63, 64, 127, 128, 191, 192, 254, 255):
        for k, c in enumerate((1, 2, 3)):
            assert int(lut[i, k]) == (min(max(765 - 2 * abs(4 * i - 255 * c), 0), 510) + 1) // 2


def _all_pairs():
    f, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return f, c


def test_model_tells_a_contracted_blend_apart():
    f, c = _all_pairs()
    ref = VM.blend(f, c, 0.7, 0.3, 0.0)
    a32, b32 = np.float64(np.float32(0.7)), np.float64(np.float32(0.3))
    cb = (c.astype(np.float32) * np.float32(0.3)).astype(np.float32)
    # fma(frame, alpha, fl(colour * beta)): the product enters the sum unrounded (exact in float64), one rounding
    fused = (f.astype(np.float64) * a32 + cb.astype(np.float64)).astype(np.float32)
    fused = np.clip(np.rint(fused), 0, 255).astype(np.uint8)
    # ... and the other way round, fma(colour, beta, fl(frame * alpha))
    fa = (f.astype(np.float32) * np.float32(0.7)).astype(np.float32)
    fused2 = (c.astype(np.float64) * b32 + fa.astype(np.float64)).astype(np.float32)
    fused2 = np.clip(np.rint(fused2), 0, 255).astype(np.uint8)
    n1, n2 = int((fused != ref).sum()), int((fused2 != ref).sum())
    print(f"contracted blends differ from the model on {n1} and {n2} of 65536 byte pairs")
    assert n1 >= 1 and n2 >= 1


def test_model_tells_round_half_up_apart():
    f, c = _all_pairs()
    ref = VM.blend(f, c, 0.7, 0.3, 0.0)
    f32 = np.float32
    v = ((f.astype(f32) * f32(0.7)).astype(f32) + (c.astype(f32) * f32(0.3)).astype(f32)).astype(f32)
    half_up = np.clip(np.floor(v.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)
    n = int((half_up != ref).sum())
    print(f"round-half-up differs from the model on {n} of 65536 byte pairs")
    assert n >= 1


def test_model_tells_a_float64_blend_apart():
    f, c = _all_pairs()
    ref = VM.blend(f, c, 0.7, 0.3, 0.0)
    wide = np.clip(np.rint(f.astype(np.float64) * 0.7 + c.astype(np.float64) * 0.3), 0, 255).astype(np.uint8)
    n = int((wide != ref).sum())
    print(f"a float64 blend differs from the model on {n} of 65536 byte pairs")
    assert n >= 1


def test_overlay_model_on_a_small_case():
    """the model's own plumbing: equal sizes copy the mask, the table is indexed by it, gamma saturates"""
    frames = np.full((1, 2, 2, 3), 200, dtype=np.uint8)
    masks = np.array([[[0, 255], [7, 128]]], dtype=np.uint8)
    lut = V.jet_table()
    out, m = VM.overlay_batch(frames, masks, lut, 1.0, 1.0, 0.0)
    assert np.array_equal(m, masks)
    assert np.array_equal(out[0, 0, 0], np.minimum(200 + lut[0].astype(int), 255))
    assert np.array_equal(out[0, 1, 1], np.minimum(200 + lut[128].astype(int), 255))
    out, _ = VM.overlay_batch(frames, masks, lut, 0.0, 0.0, -3.5)
    assert not out.any()


class _StubPipeline:
    """run() in pure numpy: the overlay of a frame is the frame plus one, so order and identity show"""

    def __init__(self):
        self.sizes = []

    def run(self, chunks):
        for chunk in chunks:
            self.sizes.append(len(chunk))
            yield chunk + np.uint8(1), chunk[..., 0]


def test_predict_video_writes_every_frame_once_in_order():
    frames = [np.full((4, 6, 3), i, dtype=np.uint8) for i in range(11)]
    written = []
    stub = _StubPipeline()
    count, seconds = V.predict_video(stub, iter(frames), written.append, chunk=4)
    assert count == 11 and seconds >= 0.0
    assert stub.sizes == [4, 4, 3]
    assert len(written) == 11
    for i, w in enumerate(written):
        assert w.shape == (4, 6, 3) and (w == i + 1).all()
    # no frames at all: nothing is written
    assert V.predict_video(_StubPipeline(), [], written.append)[0] == 0 and len(written) == 11
