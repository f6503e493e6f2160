"""The polygon rasteriser without a GPU: the rule (tests/annotate_model.py) against bitmaps worked out by hand, its two
ways of sampling, painter's order and the slivers; the package's host path (unet_lane_detection_amd/annotate.py)
against the rule; load_labelme, the CSR tables and every ValueError; loop.fit_progressive on a fake trainer; the
library's argument checks, which refuse before any device is touched; and Pillow as an independent plausibility check
(Pillow is not the specification)."""
import ctypes as C
import os

import numpy as np
import pytest

import annotate_cases as AC
import annotate_model as AM
from unet_lane_detection_amd import _lib, loop
from unet_lane_detection_amd import annotate as A
from unet_lane_detection_amd.augment import Augmenter

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _norm(polygons):
    return [(np.asarray(p, dtype=np.int32).reshape(-1, 2), v) for p, v in polygons]


# ---- the rule ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(AC.HAND))
def test_model_gives_the_hand_made_bitmap(name):
    polygons, src, rows = AC.HAND[name]
    want = AC.bitmap(rows)
    assert want.shape == src
    got = AM.fill_polygons(polygons, src)
    assert np.array_equal(got, want), "\n" + "\n".join("".join("%4d" % v for v in r) for r in got)
    # the package's host path states the same rule
    assert np.array_equal(A.rasterize(A.PolygonBatch([_norm(polygons)]), src)[0], want)


def test_line_does_not_depend_on_its_direction_or_on_the_first_vertex():
    rng = np.random.default_rng(3)
    for _ in range(200):
        pts = rng.integers(-6, 30, (int(rng.integers(2, 7)), 2))
        a = AM.fill_polygons([(pts, 255)], (23, 19))
        assert np.array_equal(a, AM.fill_polygons([(pts[::-1], 255)], (23, 19)))
        assert np.array_equal(a, AM.fill_polygons([(np.roll(pts, 2, axis=0), 255)], (23, 19)))


@pytest.mark.parametrize("src,out", AC.RESAMPLE)
def test_sampling_is_rasterise_at_source_size_then_nearest(src, out):
    polygons = AC.resample_polygons(src)
    direct = AM.fill_polygons(polygons, src, out)
    assert direct.shape == out and direct.any()
    assert np.array_equal(direct, AM.fill_polygons_via_source(polygons, src, out))
    sy, sx = AM.sample_points(src, out)
    assert np.array_equal(direct, AM.fill_polygons(polygons, src)[sy[:, 0]][:, sx[0]])
    assert np.array_equal(AM.fill_polygons(polygons, src, src), AM.fill_polygons(polygons, src))   # equal sizes: identity
    assert np.array_equal(A.rasterize(A.PolygonBatch([polygons]), src, out)[0], direct)


def test_host_path_equals_the_model_on_random_batches():
    rng = np.random.default_rng(11)
    for _ in range(60):
        src = tuple(int(v) for v in rng.integers(1, 40, 2))
        out = tuple(int(v) for v in rng.integers(1, 40, 2))
        frames = [AC.random_polygons(rng, *src, int(rng.integers(0, 4))) for _ in range(int(rng.integers(1, 4)))]
        assert np.array_equal(A.rasterize(A.PolygonBatch(frames), src, out), AM.fill_batch(frames, src, out))


def test_slivers_stay_in_one_piece():
    """a marking's far end is thinner than a pixel: with the outline every lane quad is one 8-connected component"""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for _ in range(1000):
        h, w = (int(v) for v in rng.integers(8, 90, 2))
        width = int(rng.integers(1, 8))
        xb, xt = int(rng.integers(0, w - width)), int(rng.integers(0, w - 1))
        mask = AM.fill_polygons([(AM.lane_quad(xb, xt, width, h), 255)], (h, w))
        _, pieces = ndimage.label(mask, structure=np.ones((3, 3), dtype=int))
        assert pieces == 1, (h, w, xb, xt, width)
        assert mask[0].any() and mask[h - 1].any()


def test_model_limits():
    with pytest.raises(ValueError):
        AM.fill_polygons([([[AC.BIG + 1, 0]], 255)], (4, 4))
    with pytest.raises(ValueError):
        AM.fill_polygons([([[0, -AC.BIG - 1]], 255)], (4, 4))
    for src, out in (((0, 4), (4, 4)), ((4, 16385), (4, 4)), ((4, 4), (4, 0)), ((4, 4), (16385, 4))):
        with pytest.raises(ValueError):
            AM.fill_polygons([], src, out)
    with pytest.raises(ValueError):
        AM.fill_polygons([([[0, 0]], 256)], (4, 4))
    assert AM.fill_polygons([], (16384, 1)).shape == (16384, 1)


# ---- Pillow, an independent rasteriser -------------------------------------------------------------------------

def test_plausible_against_pillow():
    """Every pixel Pillow's polygon (filled, with outline) sets lies within the 3 x 3 neighbourhood of a pixel the rule
    sets, and over 2000 polygons the two differ in at most 0.04 of the rule's area.  The reverse containment does not
    hold on shallow edges, where the two line rules shift runs by several pixels, and is not asserted."""
    pytest.importorskip("PIL")
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(0)
    outside, differ, area = 0, 0, 0
    for i in range(2000):
        h, w = (int(v) for v in rng.integers(8, 90, 2))
        if i % 2:
            pts = AC.star_polygon(rng, h, w)
        else:
            width = int(rng.integers(1, 8))
            pts = np.array(AM.lane_quad(int(rng.integers(0, w - width)), int(rng.integers(0, w - 1)), width, h))
        ours = AM.fill_polygons([(pts, 255)], (h, w)) > 0
        img = Image.new("L", (w, h), 0)
        ImageDraw.Draw(img).polygon([(int(x), int(y)) for x, y in pts], fill=255, outline=255)
        theirs = np.asarray(img) > 0
        grown = np.zeros((h + 2, w + 2), dtype=bool)
        for dy in range(3):
            for dx in range(3):
                grown[dy:dy + h, dx:dx + w] |= ours
        outside += int((theirs & ~grown[1:-1, 1:-1]).sum())
        differ += int((theirs != ours).sum())
        area += int(ours.sum())
    print("pillow: %d pixels outside the neighbourhood, %d of %d differ (%.4f)" % (outside, differ, area, differ / area))
    assert outside == 0
    assert differ <= 0.04 * area


# ---- LabelMe ---------------------------------------------------------------------------------------------------

def test_load_labelme_follows_the_reference_rule():
    path = os.path.join(GOLDEN, "labelme_small.json")
    polygons, size = A.load_labelme(path)
    assert size == (12, 16) and len(polygons) == 2
    # np.array(points, dtype=np.int32) truncates towards zero: -0.7 -> 0, 9.99 -> 9
    assert polygons[0][0].dtype == np.int32 and polygons[0][0].tolist() == [[1, 2], [9, 2], [9, 8], [0, 8]]
    assert polygons[1][0].tolist() == [[11, 6], [13, 6], [12, 10]]
    assert [v for _, v in polygons] == [255, 255]
    # another label; a negative point truncates towards zero as well (-3.6 -> -3)
    road, _ = A.load_labelme(path, label="road")
    assert len(road) == 1 and road[0][0].tolist() == [[-3, 4], [15, 5], [15, 11], [0, 11]]
    # two labels as a label plane, in file order: the second lane is painted over the road
    both, _ = A.load_labelme(path, values={"lane": 200, "road": 100})
    assert [v for _, v in both] == [200, 100, 200]
    plane = A.rasterize(A.PolygonBatch([both]), size)[0]
    assert np.array_equal(plane, AM.fill_polygons(both, size))
    assert set(np.unique(plane)) == {0, 100, 200} and plane[8, 12] == 200 and plane[9, 5] == 100 and plane[3, 5] == 200
    # a dict is taken as the parsed file
    import json
    with open(path) as f:
        again, _ = A.load_labelme(json.load(f))
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(again, polygons))
    with pytest.raises(ValueError):
        A.load_labelme(path, values={"lane": 256})
    # the reference's batch loop
    masks = A.labelme_to_masks([path, path])
    assert masks.shape == (2, 12, 16) and np.array_equal(masks[1], AM.fill_polygons(polygons, size))
    small = A.labelme_to_masks([path], out_size=(6, 8))
    assert np.array_equal(small[0], AM.fill_polygons(polygons, size, (6, 8)))
    with pytest.raises(ValueError):
        A.labelme_to_masks([])


# ---- CSR tables ------------------------------------------------------------------------------------------------

def test_polygon_batch_builds_csr_tables():
    frames = [[], [([[1, 2], [3, 4], [5, 6]], 7), ([], 8), ([[9, 9]], 255)], [], [(np.array([[0, 1], [2, 3]]), 0)]]
    b = A.PolygonBatch(frames)
    assert b.n == 4 and len(b) == 4 and b.device is None
    assert b.vertices.dtype == np.int32 and b.vertices.tolist() == [[1, 2], [3, 4], [5, 6], [9, 9], [0, 1], [2, 3]]
    assert b.poly_offsets.dtype == np.int32 and b.poly_offsets.tolist() == [0, 3, 3, 4, 6]
    assert b.poly_values.dtype == np.uint8 and b.poly_values.tolist() == [7, 8, 255, 0]
    assert b.frame_offsets.dtype == np.int32 and b.frame_offsets.tolist() == [0, 0, 3, 3, 4]
    back = b.frames()
    assert [len(f) for f in back] == [0, 3, 0, 1] and back[1][2][0].tolist() == [[9, 9]] and back[1][1][1] == 8
    again = A.PolygonBatch.from_arrays(b.vertices, b.poly_offsets, b.poly_values, b.frame_offsets)
    assert np.array_equal(A.rasterize(again, (8, 8)), A.rasterize(b, (8, 8)))
    # a batch of frames without any polygon is all zeros
    assert not A.rasterize(A.PolygonBatch([[], []]), (3, 5)).any()


def test_polygon_batch_refuses_bad_tables():
    v = np.array([[0, 0], [1, 1], [2, 0]], dtype=np.int32)
    ok = (v, [0, 3], [255], [0, 1])
    A.PolygonBatch.from_arrays(*ok)
    bad = [
        (v, [1, 3], [255], [0, 1]),                      # poly_offsets does not start at 0
        (v, [0, 2], [255], [0, 1]),                      # ... does not end at V
        (v, [0, 4], [255], [0, 1]),
        (v, [0, 2, 1, 3], [1, 2, 3], [0, 3]),            # ... decreases
        (v, [0, 3], [255, 1], [0, 2]),                   # one entry more than values
        (v, [0, 3], [255], [1, 1]),                      # frame_offsets does not start at 0
        (v, [0, 3], [255], [0, 2]),                      # ... does not end at P
        (v, [0, 1, 3], [1, 2], [0, 2, 1, 2]),            # ... decreases
        (v, [0, 3], [255], [0]),                         # no frame
        (v, [0, 3], [256], [0, 1]),                      # not a byte
        (v, [0, 3], [-1], [0, 1]),
        (v, [[0, 3]], [255], [0, 1]),                    # not 1-d
        (v, [0.0, 3.0], [255], [0, 1]),                  # not integers
        (v.astype(np.float32), [0, 3], [255], [0, 1]),
        (v.reshape(-1), [0, 6], [255], [0, 1]),          # not (V, 2)
        (v * (AC.BIG + 1), [0, 3], [255], [0, 1]),       # beyond +-2^20
        (-v * (AC.BIG + 1), [0, 3], [255], [0, 1]),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            A.PolygonBatch.from_arrays(*args)
    A.PolygonBatch.from_arrays(np.minimum(v, 1) * AC.BIG, [0, 3], [255], [0, 1])     # the limit itself is allowed
    A.PolygonBatch.from_arrays(np.minimum(v, 1) * -AC.BIG, [0, 3], [255], [0, 1])
    for frames in ([[([[0.5, 1.0]], 255)]], [[([[0, 1, 2]], 255)]], [[([0, 1, 2], 255)]], [[[[0, 1], [2, 3]]]],
                   [[([[0, 1]], 300)]], [[([[AC.BIG + 1, 0]], 1)]], []):
        with pytest.raises(ValueError):
            A.PolygonBatch(frames)


def test_rasterize_refuses_bad_calls():
    b = A.PolygonBatch([[(AC.SQUARE, 255)]])
    for src, out in (((0, 4), None), ((4, 16385), None), ((4, 4), (0, 4)), ((4, 4), (4, 16385)), ((4,), None)):
        with pytest.raises(ValueError):
            A.rasterize(b, src, out)
    with pytest.raises(ValueError):
        A.rasterize(b, (4, 4), out=np.zeros((1, 4, 4), dtype=np.uint8))     # out= is for the device
    with pytest.raises(TypeError):
        A.rasterize([[(AC.SQUARE, 255)]], (4, 4))
    with pytest.raises(ValueError):
        b.to("cpu")


def test_library_refuses_before_touching_a_device():
    lib = _lib.load()
    buf = (C.c_int32 * 16)()
    p = C.cast(buf, C.c_void_p)

    def call(v=p, po=p, pv=p, fo=p, n=1, sh=4, sw=4, oh=4, ow=4, out=p):
        return lib.unet_fill_polygons_u8_batch(0, v, po, pv, fo, n, sh, sw, oh, ow, out, None)
    for kw in (dict(v=None), dict(po=None), dict(pv=None), dict(fo=None), dict(out=None), dict(n=0), dict(n=-1),
               dict(po=C.c_void_p(C.addressof(buf) + 2)), dict(v=C.c_void_p(C.addressof(buf) + 4))):
        assert call(**kw) == 1, kw                                   # UNET_ERR_INVALID_ARG
        assert lib.unet_op_last_error().startswith(b"invalid argument: unet_fill_polygons_u8_batch")
    for kw in (dict(sh=0), dict(sw=0), dict(oh=0), dict(ow=0), dict(sh=16385), dict(sw=16385), dict(oh=16385),
               dict(ow=16385)):
        assert call(**kw) == 2, kw                                   # UNET_ERR_SHAPE
        assert b"unet_fill_polygons_u8_batch" in lib.unet_op_last_error()


# ---- progressive training on a fake trainer ----------------------------------------------------------------------

class _Val:
    def __init__(self, dice):
        self.dice, self.loss = dice, 1.0 - dice


class _FakeTrainer:
    def __init__(self):
        self.lr = 0.5
        self.calls = []
        self.step_count = 0

    def reset_optimizer(self):
        self.calls.append(("reset", self.step_count))
        self.step_count = 0

    def step(self, images, targets):
        self.step_count += 1
        self.calls.append(("step", tuple(images.shape), tuple(targets.shape), self.lr, self.step_count))
        return np.float32(1.0 / self.step_count)

    def validate(self, batches):
        shapes = [tuple(images.shape) for images, _ in batches]
        self.calls.append(("validate", shapes))
        return _Val(0.1 * len([c for c in self.calls if c[0] == "validate"]))

    def save_checkpoint(self, path, epoch=0, best_dice=None, with_optimizer=True):
        self.calls.append(("save", os.path.relpath(path, self.root)))


class _HostSource:
    """what annotate.TrainingSource is on the device, with numpy arrays: frames by nearest pixel, masks by the rule"""

    def __init__(self, n, height, width, seed):
        rng = np.random.default_rng(seed)
        self.frames = rng.integers(0, 256, (n, height, width, 3), dtype=np.uint8)
        self.batch = A.PolygonBatch([AC.lane_frame(rng, height, width) for _ in range(n)])
        self.sizes = []

    def at(self, size):
        self.sizes.append(size)
        h, w = self.frames.shape[1:3]
        sy, sx = AM.sample_points((h, w), (size, size))
        return self.frames[:, sy[:, 0]][:, :, sx[0]], A.rasterize(self.batch, (h, w), (size, size))


def test_fit_progressive_runs_one_fit_per_stage(tmp_path):
    tr = _FakeTrainer()
    tr.root = str(tmp_path)
    train, val = _HostSource(3, 20, 30, 1), _HostSource(2, 20, 30, 2)
    stages = [(8, 2, 1e-3), (12, 1, 1e-4), (16, 2, 1e-5)]
    seen = []
    hist = loop.fit_progressive(tr, train, val, stages, batch_size=2, augmenter=Augmenter(seed=4), save_dir=str(tmp_path),
                                on_epoch=seen.append)
    assert train.sizes == [8, 12, 16] and val.sizes == [8, 12, 16]
    assert [len(h) for h in hist] == [2, 1, 2] and seen == [r for h in hist for r in h]
    assert [[r["lr"] for r in h] for h in hist] == [[1e-3, 1e-3], [1e-4], [1e-5, 1e-5]]
    assert [[r["epoch"] for r in h] for h in hist] == [[1, 2], [1], [1, 2]]
    # every stage: the optimiser is reset before its first step, its steps see the stage's size and rate, and the Adam
    # step count starts again at 1; 3 frames in batches of 2 are two steps an epoch
    kinds = [c[0] for c in tr.calls if c[0] in ("reset", "step")]
    assert kinds == ["reset"] + ["step"] * 4 + ["reset"] + ["step"] * 2 + ["reset"] + ["step"] * 4
    assert [c[1] for c in tr.calls if c[0] == "reset"] == [0, 4, 2]
    steps = [c for c in tr.calls if c[0] == "step"]
    assert [c[1][1:3] for c in steps] == [(8, 8)] * 4 + [(12, 12)] * 2 + [(16, 16)] * 4
    assert all(c[1][3] == 3 and c[2] == (c[1][0], 1) + c[1][1:3] for c in steps)
    assert [c[3] for c in steps] == [1e-3] * 4 + [1e-4] * 2 + [1e-5] * 4
    assert [c[4] for c in steps] == [1, 2, 3, 4, 1, 2, 1, 2, 3, 4]
    vals = [c[1] for c in tr.calls if c[0] == "validate"]
    assert vals == [[(2, 8, 8, 3)]] * 2 + [[(2, 12, 12, 3)]] + [[(2, 16, 16, 3)]] * 2
    # best_dice starts again in every stage (a stage is a run of its own), and each stage has its own directory
    assert [[r["improved"] for r in h] for h in hist] == [[True, True], [True], [True, True]]
    saves = [c[1] for c in tr.calls if c[0] == "save"]
    assert saves == [os.path.join("stage1", "best_model.pth")] * 2 + [os.path.join("stage1", "last_model.pth"),
                     os.path.join("stage2", "best_model.pth"), os.path.join("stage2", "last_model.pth")] + \
        [os.path.join("stage3", "best_model.pth")] * 2 + [os.path.join("stage3", "last_model.pth")]
    assert loop.REFERENCE_STAGES == [(128, 30, 1e-3), (192, 30, 1e-4), (224, 20, 1e-5)]
    # without a directory nothing is written
    tr2 = _FakeTrainer()
    loop.fit_progressive(tr2, train, val, [(8, 1, 1e-3)], batch_size=3, augmenter=Augmenter(seed=4))
    assert not [c for c in tr2.calls if c[0] == "save"]
