"""The polygon rasteriser on the GPU (csrc/annotate_kernels.cpp through the C ABI and unet_lane_detection_amd/annotate.py)
against tests/annotate_model.py: every comparison is bit-exact.  Parity with cv2.fillPoly itself is unpinned (see the
model's header).  Every output buffer starts filled with 0xAA between guard bytes, so a byte the kernel leaves out or
writes outside shows."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import annotate_cases as AC
import annotate_model as AM
import video_model as VM
from unet_lane_detection_amd import _lib, state as S
from unet_lane_detection_amd import annotate as A
from unet_lane_detection_amd import augment as G

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xAA, 64


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=False)


def _p(t):
    return C.c_void_p(t.data_ptr())


def run_kernel(lib, frames, src, out=None, lead=GUARD):
    """the frames' polygons through unet_fill_polygons_u8_batch into `size` bytes at byte `lead` of a buffer of 0xAA:
    lead = 64 keeps the output 16-byte aligned, 65 puts it one byte off"""
    out = tuple(src) if out is None else tuple(out)
    batch = A.PolygonBatch(frames).to(0)
    n, size = batch.n, batch.n * out[0] * out[1]
    whole = torch.full((lead + size + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    view = whole[lead:lead + size]
    v, po, pv, fo = batch._dev
    rc = lib.unet_fill_polygons_u8_batch(0, _p(v), _p(po), _p(pv), _p(fo), n, src[0], src[1], out[0], out[1], _p(view), None)
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    w = whole.cpu().numpy()
    assert (w[:lead] == CANARY).all() and (w[lead + size:] == CANARY).all(), "a byte outside the output was written"
    return w[lead:lead + size].reshape((n,) + out)


def same(got, want):
    bad = int((got != want).sum())
    assert bad == 0, f"{bad} of {want.size} mask bytes differ"


@pytest.mark.parametrize("name", sorted(AC.HAND))
def test_hand_made_cases(lib, name):
    polygons, src, rows = AC.HAND[name]
    got = run_kernel(lib, [polygons], src)
    same(got[0], AM.fill_polygons(polygons, src))
    same(got[0], AC.bitmap(rows))


@pytest.mark.parametrize("out", [(1, 1), (5, 7), (3, 17), (9, 64), (9, 67), (1, 67), (70, 130)])
@pytest.mark.parametrize("lead", [64, 65])
def test_output_widths_and_alignments(lib, out, lead):
    """rows that end inside a 16-byte group, rows whose start is not aligned (width 67; any width one byte off), rows
    that leave as 16-byte stores (width 64, aligned), one row, one pixel, and more than one tile either way"""
    src = (37, 53)
    rng = np.random.default_rng(out[0] * 1000 + out[1])
    frames = [AC.lane_frame(rng, *src) + AC.random_polygons(rng, *src, 3, spread=0.3), AC.random_polygons(rng, *src, 2)]
    want = AM.fill_batch(frames, src, out)
    assert out == (1, 1) or want.any()
    same(run_kernel(lib, frames, src, out, lead=lead), want)


@pytest.mark.parametrize("src,out", AC.RESAMPLE)
def test_resampling(lib, src, out):
    polygons = AC.resample_polygons(src)
    want = AM.fill_polygons(polygons, src, out)
    same(run_kernel(lib, [polygons], src, out)[0], want)
    same(run_kernel(lib, [polygons], src)[0], AM.fill_polygons(polygons, src))


def test_empty_frames_and_uneven_offsets(lib):
    src = (45, 70)
    rng = np.random.default_rng(21)
    frames = [AC.random_polygons(rng, *src, k, spread=0.5) for k in (0, 3, 0, 1, 40)]
    assert [len(f) for f in frames] == [0, 3, 0, 1, 40]
    want = AM.fill_batch(frames, src)
    assert not want[0].any() and not want[2].any() and want[4].any()
    same(run_kernel(lib, frames, src), want)
    same(run_kernel(lib, [[], []], src), np.zeros((2,) + src, dtype=np.uint8))        # no polygon at all


@pytest.mark.parametrize("src", [(64, 64), (100, 130)])
def test_long_polygon_is_carried_across_chunks(lib, src):
    """6000 edges, all of which meet every tile's rows: several times the LDS budget of records, so parity, outline,
    polygon and value cross chunk boundaries; the small polygon after it must paint over it"""
    zig = AC.zigzag(6000, *src)
    frames = [[([[5, 5], [50, 9], [30, 40]], 77), (zig, 200), ([[20, 20], [40, 22], [28, 45]], 90)]]
    want = AM.fill_batch(frames, src)
    assert {77, 200, 90} <= set(np.unique(want)) and (want == 0).any()
    same(run_kernel(lib, frames, src), want)


@pytest.mark.parametrize("spread", [20.0, 11000.0])      # the second reaches 0.95 of the coordinate limit
def test_vertices_far_outside_the_frame(lib, spread):
    src, out = (60, 90), (48, 80)
    rng = np.random.default_rng(int(spread))
    frames = [AC.random_polygons(rng, *src, 3, spread=spread, near=0.5) for _ in range(8)]
    assert max(np.abs(p).max() for f in frames for p, _ in f if len(p)) > spread * 40
    want = AM.fill_batch(frames, src, out)
    assert sum(len(np.unique(f)) > 1 for f in want) >= 4          # long edges do pass through the frames
    same(run_kernel(lib, frames, src, out), want)


def test_python_path_on_another_stream():
    src, out = (50, 66), (31, 47)
    rng = np.random.default_rng(8)
    frames = [AC.lane_frame(rng, *src) for _ in range(3)]
    batch = A.PolygonBatch(frames).to(0)
    assert batch.device == torch.device("cuda", 0) and batch.n == 3
    want = AM.fill_batch(frames, src, out)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = A.rasterize(batch, src, out)
        into = torch.full((3,) + out, CANARY, dtype=torch.uint8, device="cuda")
        assert A.rasterize(batch, src, out, out=into) is into
    stream.synchronize()
    assert got.is_cuda and got.dtype == torch.uint8
    same(got.cpu().numpy(), want)
    same(into.cpu().numpy(), want)
    same(A.rasterize(batch, src).cpu().numpy(), AM.fill_batch(frames, src))
    with pytest.raises(ValueError):
        A.rasterize(batch, src, out, out=into[:2])
    with pytest.raises(ValueError):
        A.rasterize(batch, src, (0, 4))


@pytest.mark.parametrize("bgr", [False, True])
def test_training_source_and_two_steps(lib, bgr):
    from unet_lane_detection_amd.trainer import UNetTrainer
    n, h, w = 6, 40, 56
    rng = np.random.default_rng(13)
    frames_u8 = S.synthetic_frames(n, h, w, seed=3)
    polys = [AC.lane_frame(rng, h, w) for _ in range(n)]
    source = A.TrainingSource(frames_u8, A.PolygonBatch(polys), bgr=bgr, device=0)
    assert len(source) == n
    for s in (16, 24):
        ds = source.at(s)
        assert isinstance(ds, G.DeviceDataset) and ds.images.shape == (n, s, s, 3) and ds.masks.shape == (n, s, s)
        # the images are unet_resize_u8_batch's own output ...
        own = torch.empty((n, s, s, 3), dtype=torch.uint8, device="cuda")
        src_dev = torch.from_numpy(frames_u8).cuda()
        assert lib.unet_resize_u8_batch(0, _p(src_dev), n, h, w, 3, 1 if bgr else 0, s, s, _p(own), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(ds.images, own)
        assert np.array_equal(own.cpu().numpy(), VM.resize_batch(frames_u8, s, s, swap_rb=bgr))
        # ... and the masks are the rule at that size, not a resized mask
        same(ds.masks.cpu().numpy(), AM.fill_batch(polys, (h, w), (s, s)))
    full = source.at(None)
    assert full.images.shape == (n, h, w, 3)
    same(full.masks.cpu().numpy(), AM.fill_batch(polys, (h, w)))
    # two steps of the tiny model on batches built from it
    tr = UNetTrainer(S.seeded_state_dict([4, 8], seed=1), device=0, lr=1e-3)
    batches = G.AugmentedBatches(source.at(16), 3, G.Augmenter(seed=2))
    losses = [float(tr.step(images, targets)) for images, targets in batches()]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    tr.reset_optimizer()
    assert tr.step_count == 0 and not tr.exp_avg.any() and not tr.exp_avg_sq.any()
    assert tr.device_error() == 0
    tr.release()
