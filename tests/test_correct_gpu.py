"""The frame correction on the GPU (csrc/correct_kernels.cpp through the C ABI, unet_lane_detection_amd/correct.py)
against tests/correct_model.py: the whole work buffer - channel histograms, plan words, channel tables, tile
histograms, tile tables - and the output are compared bit for bit; nothing here has a tolerance.  Parity with cv2's
CLAHE is unpinned (see the model's header).  tests/test_correct_cpu.py shows that the cases used here tell the listed
mistakes apart.  Every buffer lies inside a larger one filled with a canary: the guards must stay intact, the output's
padding must stay canary, and the input must be unchanged unless the call is in place."""
import ctypes as C

import numpy as np
import pytest
import torch

import correct_model as CM
from unet_lane_detection_amd import _lib
from unet_lane_detection_amd import correct as K

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


def cfg_struct(cfg):
    s = _lib.CorrectConfigStruct()
    for k, v in cfg.items():
        if k == "tone":
            C.memmove(s.tone, v.ctypes.data, 256)
        else:
            setattr(s, k, v)
    return s


def raw_bytes(frames, pad):
    """the frames as they lie in memory with `pad` bytes of padding (255) a row; the last row ends with its pixels"""
    n, h, w, _ = frames.shape
    if not pad:
        return frames.reshape(-1)
    rows = CM.padded_rows(frames, 3 * w + pad).reshape(-1)
    return rows[:rows.size - pad]


def run(lib, frames, cfg, bgr=True, pad=0, lead=0, inplace=False, out_pad=None):
    """-> (work buffer bytes, output frames (n,h,w,3)); checks guards, padding and the input on the way"""
    n, h, w, _ = frames.shape
    data = raw_bytes(frames, pad)
    fr = Buf(data.size, GUARD + lead, data)
    out_pad = pad if out_pad is None or inplace else out_pad
    ostride = 3 * w + out_pad
    out = fr if inplace else Buf((n * h - 1) * ostride + 3 * w, GUARD + lead)
    work = Buf(CM.work_bytes(n, cfg["grid_x"], cfg["grid_y"]))
    s = cfg_struct(cfg)
    rc = lib.unet_correct_u8_batch(0, _p(fr.view), n, h, w, 3 * w + pad if pad else 0, 1 if bgr else 0, C.byref(s),
                                   _p(out.view), ostride if out_pad else 0, _p(work.view), work.size, None)
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    assert out.guards_intact() and fr.guards_intact() and work.guards_intact()
    if not inplace:
        assert np.array_equal(fr.numpy(), data)
    got = np.concatenate([out.numpy(), np.full(out_pad, 255 if inplace else CANARY, np.uint8)]).reshape(n, h, ostride)
    assert (got[:, :, 3 * w:] == (255 if inplace else CANARY)).all(), "padding was written"
    return work.numpy(), np.ascontiguousarray(got[:, :, :3 * w]).reshape(n, h, w, 3)


def compare(work, out, ref, label):
    """region by region, so that a failure names the first pass that went wrong"""
    n = ref["hist"].shape[0]
    want = CM.pack_work(ref)
    assert work.size == want.size
    per = want.size // n
    tiles = ref["tile_hist"].shape[1] * ref["tile_hist"].shape[2]
    bounds = [("hist", 3072), ("plan", 32), ("lut", 768), ("tile_hist", tiles * 1024), ("tile_lut", tiles * 256)]
    for i in range(n):
        o = i * per
        for name, size in bounds:
            g, r = work[o:o + size], want[o:o + size]
            if name in ("hist", "plan", "tile_hist"):
                g, r = g.view(np.uint32), r.view(np.uint32)
            bad = np.flatnonzero(g != r)
            assert bad.size == 0, f"{label}: frame {i} {name}: {bad.size} differ, first at {bad[0]}: {g[bad[0]]} != {r[bad[0]]}"
            o += size
    bad = np.argwhere(out != ref["out"])
    assert bad.size == 0, f"{label}: output: {len(bad)} bytes differ, first at {bad[0]}: " \
                          f"{out[tuple(bad[0])]} != {ref['out'][tuple(bad[0])]}"


_model = {}


def model(name, bgr):
    """the model's answer, computed once"""
    if (name, bgr) not in _model:
        frames, cfg, _ = CM.case(name)
        _model[(name, bgr)] = CM.correct(frames, cfg, bgr)
    return _model[(name, bgr)]


@pytest.mark.parametrize("name", list(CM.CASES))
def test_case_against_the_model(lib, name):
    """every case with is_bgr 1 and 0"""
    frames, cfg, extras = CM.case(name)
    for bgr in (True, False):
        work, out = run(lib, frames, cfg, bgr, pad=extras.get("stride", 0), lead=extras.get("lead", 0),
                        inplace=extras.get("inplace", False))
        compare(work, out, model(name, bgr), f"{name} bgr {bgr}")


def test_the_two_paths_give_the_same_bits(lib):
    """16 x 64 dense from a 64-byte aligned base (16-byte loads and stores) and the same frames at byte offset 65 with
    row_stride = 3 w + 5 (bytes): equal to each other and to the model; and a mixed call (aligned in, unaligned out)"""
    frames, cfg, _ = CM.case("aligned_16x64")
    ref = model("aligned_16x64", True)
    work_a, out_a = run(lib, frames, cfg, True)
    work_b, out_b = run(lib, frames, cfg, True, pad=5, lead=1)
    work_c, out_c = run(lib, frames, cfg, True, pad=0, out_pad=16)
    assert np.array_equal(out_a, out_b) and np.array_equal(work_a, work_b)
    assert np.array_equal(out_a, out_c) and np.array_equal(work_a, work_c)
    compare(work_a, out_a, ref, "aligned")


def test_in_place_equals_out_of_place(lib):
    frames, cfg, _ = CM.case("in_place")
    for pad in (0, 3, 16):
        work_i, out_i = run(lib, frames, cfg, True, pad=pad, inplace=True)
        work_o, out_o = run(lib, frames, cfg, True, pad=pad, inplace=False)
        assert np.array_equal(out_i, out_o) and np.array_equal(work_i, work_o), pad
        compare(work_i, out_i, model("in_place", True), f"in place, pad {pad}")


def test_only_flagged_leaves_a_normal_frame_alone(lib):
    frames, cfg, _ = CM.case("only_flagged")
    work, out = run(lib, frames, cfg, True, pad=7)
    per = work.size // 3
    flags = [int(work[i * per + 3072:i * per + 3076].view(np.uint32)[0]) for i in range(3)]
    assert [f & 1 for f in flags] == [1, 0, 1] and flags[1] == 0
    assert np.array_equal(out[1], frames[1]) and not np.array_equal(out[0], frames[0])


def test_a_second_call_overwrites_everything(lib):
    """one work buffer and one output, two different calls: the second's results do not depend on the first's"""
    fa, ca, _ = CM.case("odd_37x53_grid4x3")
    fb, cb, _ = CM.case("only_flagged")
    size = max(CM.work_bytes(3, 4, 3), CM.work_bytes(3, 3, 2))
    work = Buf(size)
    out = Buf(3 * 37 * 53 * 3)
    for frames, cfg, name in ((fa, ca, "odd_37x53_grid4x3"), (fb, cb, "only_flagged"), (fa, ca, "odd_37x53_grid4x3")):
        n, h, w, _ = frames.shape
        fr = Buf(frames.size, data=frames)
        s = cfg_struct(cfg)
        rc = lib.unet_correct_u8_batch(0, _p(fr.view), n, h, w, 0, 1, C.byref(s), _p(out.view), 0, _p(work.view),
                                       work.size, None)
        assert rc == 0, lib.unet_op_last_error()
        torch.cuda.synchronize()
        assert work.guards_intact() and out.guards_intact()
        need = CM.work_bytes(n, cfg["grid_x"], cfg["grid_y"])
        compare(work.numpy()[:need], out.numpy()[:frames.size].reshape(frames.shape), model(name, True), name)


# ---- the Python layer ----------------------------------------------------------------------------------------------

def test_frame_corrector():
    frames, cfg, _ = CM.case("odd_37x53_grid4x3")
    ref = model("odd_37x53_grid4x3", True)
    config = K.CorrectConfig(stretch=(1.0, 1.0), tone=CM.TONE, clahe=K.Clahe(2.0, (4, 3)))
    fc = K.FrameCorrector(config)
    dev = torch.from_numpy(frames).cuda()
    out = fc.correct(dev)
    assert out.shape == dev.shape and out.data_ptr() != dev.data_ptr()
    assert np.array_equal(out.cpu().numpy(), ref["out"]) and np.array_equal(dev.cpu().numpy(), frames)
    assert fc.last_plan.is_cuda and tuple(fc.last_plan.shape) == (3, 8)
    plan = fc.plan()
    assert np.array_equal(plan.words, ref["plan"]) and plan.corrected.all()
    assert np.array_equal(plan.gains, ref["plan"][:, 1:4] / 65536.0)
    assert plan.lo.tolist() == ref["plan"][:, 4].tolist() and plan.hi.tolist() == ref["plan"][:, 5].tolist()
    assert plan.mean.tolist() == [float(f.astype(np.int64).sum()) / f.size for f in frames]
    # in place, one frame without the batch dimension, RGB, and raw rows with a stride
    same = fc.correct(dev, out=dev)
    assert same.data_ptr() == dev.data_ptr() and np.array_equal(dev.cpu().numpy(), ref["out"])
    one = fc.correct(torch.from_numpy(frames[1]).cuda(), bgr=False)
    assert one.shape == (37, 53, 3) and np.array_equal(one.cpu().numpy(), model("odd_37x53_grid4x3", False)["out"][1])
    rows = CM.padded_rows(frames, 3 * 53 + 9)
    got = fc.correct(torch.from_numpy(rows).cuda(), row_stride=3 * 53 + 9, width=53)
    assert np.array_equal(got.cpu().numpy()[:, :, :3 * 53].reshape(frames.shape), ref["out"])
    # the images of a device-resident data set, as they are
    from unet_lane_detection_amd.augment import DeviceDataset
    ds = DeviceDataset(frames, np.zeros(frames.shape[:3], np.uint8))
    assert np.array_equal(fc.correct(ds.images, bgr=False).cpu().numpy(), model("odd_37x53_grid4x3", False)["out"])
    with pytest.raises(TypeError):
        fc.correct(frames)                       # no CPU fallback: a host array is refused
    with pytest.raises(_lib.UnetError, match="unet_correct_u8_batch"):
        K.FrameCorrector(K.CorrectConfig(clahe=K.Clahe(2.0, (8, 8)))).correct(torch.zeros((1, 9, 64, 3), dtype=torch.uint8).cuda())
