"""Connected-component labelling, component statistics and the component filter (include/unet_hip.h, "lane instances
on the device") restated for the tests: a two-pass union-find over the row runs of a frame, ids in raster order of a
component's first pixel, the sixteen record words, the header, the keep rule and the cleaned mask.  Written
independently of unet_lane_detection_amd/instances.py and of the kernels; tests/test_label_cpu.py holds it to
scipy.ndimage.label.  Parity with cv2's label numbering is unpinned (cv2 is not installed where this is tested).

Mutants the tests must tell apart from the definition (tests/test_label_cpu.py):
  connectivity 4 where 8 is asked for
  column_major   ids in column-major order of the first pixel
  drop_corner    a purely diagonal link is dropped where the upper pixel has x % 8 == 7 or y % 8 == 7 (a tile corner)
  ge             a pixel is ON iff its byte is >= level
  tie_high       keep_largest: equal areas are won by the higher id
"""
import functools

import numpy as np

WORDS = 16


# ---- labelling -------------------------------------------------------------------------------------------------

def _runs(on):
    """the row runs of a boolean frame in raster order: arrays y, start, end (half-open)"""
    h, w = on.shape
    pad = np.zeros((h, w + 2), dtype=np.int8)
    pad[:, 1:-1] = on
    d = np.diff(pad, axis=1)
    ys, ss = np.nonzero(d == 1)
    _, es = np.nonzero(d == -1)
    return ys.astype(np.int64), ss.astype(np.int64), es.astype(np.int64)


def label_frame(mask, level=127, connectivity=8, column_major=False, drop_corner=False, ge=False):
    """(h, w) uint8 -> (labels (h, w) int32, K, runs (y, start, end, id))"""
    m = mask.astype(np.int64)
    on = (m >= level) if ge else (m > level)
    h, w = on.shape
    ys, ss, es = _runs(on)
    nr = len(ys)
    parent = list(range(nr))

    def find(i):
        r = i
        while parent[r] != r:
            r = parent[r]
        while parent[i] != r:
            parent[i], i = r, parent[i]
        return r

    row_first = np.searchsorted(ys, np.arange(h + 1))
    Y, S, E = ys.tolist(), ss.tolist(), es.tolist()
    d = 1 if connectivity == 8 else 0
    for y in range(1, h):
        a, a_end = int(row_first[y - 1]), int(row_first[y])
        b, b_end = a_end, int(row_first[y + 1])
        while a < a_end and b < b_end:
            # runs [S[a], E[a]) of row y - 1 and [S[b], E[b]) of row y touch iff they overlap, or with 8 meet at a corner
            if S[a] < E[b] + d and S[b] < E[a] + d:
                link = True
                if drop_corner and (E[a] == S[b] or E[b] == S[a]):
                    ux = E[a] - 1 if E[a] == S[b] else S[a]          # the upper pixel of the diagonal pair
                    link = not (ux % 8 == 7 or (y - 1) % 8 == 7)
                if link:
                    ra, rb = find(a), find(b)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)
            if E[a] < E[b]:
                a += 1
            else:
                b += 1
    ids = np.zeros(nr, dtype=np.int64)
    k = 0
    for i in range(nr):                       # run order is raster order: a root is its component's first run
        r = find(i)
        if r == i:
            k += 1
            ids[i] = k
        else:
            ids[i] = ids[r]
    if column_major and k:
        first = np.full(k + 1, h * w, dtype=np.int64)
        np.minimum.at(first, ids, ss * h + ys)
        order = np.argsort(first[1:], kind="stable")
        renum = np.zeros(k + 1, dtype=np.int64)
        renum[order + 1] = np.arange(1, k + 1)
        ids = renum[ids]
    labels = np.zeros((h, w), dtype=np.int32)
    if nr:
        # paint the runs: +id at a start, -id at an end, cumulative sum along the row
        delta = np.zeros((h, w + 1), dtype=np.int64)
        np.add.at(delta, (ys, ss), ids)
        np.add.at(delta, (ys, es), -ids)
        labels = np.cumsum(delta, axis=1)[:, :w].astype(np.int32)
    return labels, k, (ys, ss, es, ids)


def records_frame(runs, k, h, w, cap):
    """-> (header (4,) uint64, records (cap, 16) uint64) from the runs of label_frame"""
    ys, ss, es, ids = runs
    rec = np.zeros((max(k, 1), WORDS), dtype=np.uint64)
    if k:
        c = ids - 1
        y = ys.astype(np.uint64)
        cnt = (es - ss).astype(np.uint64)
        sx = ((ss + es - 1) * (es - ss) // 2).astype(np.uint64)
        big = np.uint64(np.iinfo(np.uint64).max)
        rec[:k, 1] = big
        rec[:k, 3] = big
        rec[:k, 12] = big
        np.add.at(rec[:, 0], c, cnt)
        np.minimum.at(rec[:, 1], c, ss.astype(np.uint64))
        np.maximum.at(rec[:, 2], c, (es - 1).astype(np.uint64))
        np.minimum.at(rec[:, 3], c, y)
        np.maximum.at(rec[:, 4], c, y)
        np.add.at(rec[:, 5], c, sx)
        for j, p in ((6, 1), (7, 2), (8, 3), (9, 4)):
            np.add.at(rec[:, j], c, cnt * y ** np.uint64(p))
        np.add.at(rec[:, 10], c, sx * y)
        np.add.at(rec[:, 11], c, sx * y * y)
        np.minimum.at(rec[:, 12], c, (ys * w + ss).astype(np.uint64))
        flags = ((ys == 0) * 1 + (ys == h - 1) * 2 + (ss == 0) * 4 + (es == w) * 8).astype(np.uint64)
        np.bitwise_or.at(rec[:, 13], c, flags)
    out = np.zeros((cap, WORDS), dtype=np.uint64)
    keep = min(k, cap)
    out[:keep] = rec[:keep]
    on = int((es - ss).sum())
    return np.array([k, on, keep, 0], dtype=np.uint64), out


def label(masks, level=127, connectivity=8, cap=1024, **mutant):
    """(n, h, w) uint8 -> labels (n, h, w) int32, header (n, 4) uint64, records (n, cap, 16) uint64"""
    n, h, w = masks.shape
    labels = np.zeros((n, h, w), dtype=np.int32)
    header = np.zeros((n, 4), dtype=np.uint64)
    records = np.zeros((n, cap, WORDS), dtype=np.uint64)
    for i in range(n):
        labels[i], k, runs = label_frame(masks[i], level, connectivity, **mutant)
        header[i], records[i] = records_frame(runs, k, h, w, cap)
    return labels, header, records


def keep_table(header, records, cap, min_area=0, min_height=0, min_width=0, keep_largest=0, tie_high=False):
    """one frame: header (4,), records (cap, 16) -> (cap,) uint8"""
    nrec = min(int(header[2]), cap)
    passing = []
    for c in range(nrec):
        r = [int(v) for v in records[c, :5]]
        if r[0] >= min_area and r[4] - r[3] + 1 >= min_height and r[2] - r[1] + 1 >= min_width:
            passing.append((c, r[0]))
    if keep_largest > 0:
        passing.sort(key=lambda t: (-t[1], -t[0] if tie_high else t[0]))
        passing = passing[:keep_largest]
    keep = np.zeros(cap, dtype=np.uint8)
    for c, _ in passing:
        keep[c] = 1
    return keep


def keep(labels, header, records, cap, **kw):
    """-> keep (n, cap) uint8, mask (n, h, w) uint8"""
    n = labels.shape[0]
    table = np.stack([keep_table(header[i], records[i], cap, **kw) for i in range(n)])
    mask = np.zeros(labels.shape, dtype=np.uint8)
    for i in range(n):
        lab = labels[i]
        ok = (lab > 0) & (lab <= cap)
        kept = np.zeros(lab.shape, dtype=bool)
        kept[ok] = table[i][lab[ok] - 1] != 0
        mask[i] = np.where(kept, 255, 0)
    return table, mask


def full_frame_record(h, w):
    """the record of a frame that is ON everywhere, in closed form on Python ints"""
    sy = [sum(y ** k for y in range(h)) for k in range(5)]
    sx = w * (w - 1) // 2
    return [h * w, 0, w - 1, 0, h - 1, sx * h, w * sy[1], w * sy[2], w * sy[3], w * sy[4], sx * sy[1], sx * sy[2], 0, 15, 0, 0]


# ---- inputs ----------------------------------------------------------------------------------------------------

def seed_of(n, h, w):
    return 1000 * n + 7 * h + w


def _spiral(h, w):
    on = np.zeros((h, w), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    on[0, 0] = True
    while True:
        moved = False
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            ahead_on = 0 <= ay < h and 0 <= ax < w and on[ay, ax]
            if 0 <= ny < h and 0 <= nx < w and not on[ny, nx] and not ahead_on:
                y, x = ny, nx
                on[y, x] = True
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return on


def _three_lanes(rng, h, w, speckle=0.01):
    """three solid markings that bend to the right towards the top, and speckle"""
    on = np.zeros((h, w), dtype=bool)
    thick = max(2, w // 50)
    bend = 0.08 + 0.03 * rng.random()
    for y in range(h):
        t = (h - 1 - y) / h
        for x_base in (0.15, 0.45, 0.75):
            x = int(w * (x_base + bend * t * t))
            on[y, max(x, 0):min(x + thick, w)] = True
    return on | (rng.random((h, w)) < speckle)


CONTENTS = ("zeros", "full", "checker", "serpentine", "spiral", "rings", "uw", "diagonal", "random05", "random41",
            "random59", "random90", "straddle", "painted", "lanes")
GREY = ("straddle", "painted", "lanes")     # contents whose bytes are not only 0 and 255


def _pattern(name, h, w, i, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "zeros":
        return np.zeros((h, w), dtype=bool)
    if name == "full":
        return np.ones((h, w), dtype=bool)
    if name == "checker":
        return (yy + xx + i) % 2 == 0
    if name == "serpentine":
        on = yy % 2 == 0
        odd = yy % 2 == 1
        on |= odd & (((yy // 2) % 2 == 0) & (xx == w - 1) | ((yy // 2) % 2 == 1) & (xx == 0))
        return on.T[:h, :w] if (i % 2 == 1 and h == w) else on
    if name == "spiral":
        return _spiral(h, w)
    if name == "rings":
        return np.minimum(np.minimum(yy, xx), np.minimum(h - 1 - yy, w - 1 - xx)) % 2 == (i % 2)
    if name == "uw":
        return (xx % (5 + i) == 0) | (yy == h - 1)      # arms that meet only at the bottom row
    if name == "diagonal":
        return (xx == yy) if i % 2 == 0 else (xx == w - 1 - yy)
    if name.startswith("random"):
        return rng.random((h, w)) < int(name[6:]) / 100.0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def content(name, n, h, w):
    """(n, h, w) uint8, read-only.  ON bytes are 255 and OFF bytes 0, but: `straddle` draws from {126, 127, 128, 129}
    and `painted` has ON bytes from {128, 200, 255} and OFF bytes from {0, 64, 127} (both around level 127).
    `lanes` is lanefit_model.painted_lanes, the lane fit's own masks: two markings, the left one dashed, 1 - 3 % of the
    pixels flipped, bytes on both sides of 127, an empty half in the last frame.  `painted` has three solid markings
    instead, because the Python layer's test recovers three."""
    if name == "lanes":
        import lanefit_model as LM
        out = LM.painted_lanes(seed_of(n, h, w), n, h, w)
        out.setflags(write=False)
        return out
    rng = np.random.default_rng(seed_of(n, h, w) + CONTENTS.index(name))
    out = np.zeros((n, h, w), dtype=np.uint8)
    for i in range(n):
        if name == "straddle":
            out[i] = rng.choice(np.array([126, 127, 128, 129], dtype=np.uint8), size=(h, w))
        elif name == "painted":
            on = _three_lanes(rng, h, w)
            hi = rng.choice(np.array([128, 200, 255], dtype=np.uint8), size=(h, w))
            lo = rng.choice(np.array([0, 64, 127], dtype=np.uint8), size=(h, w))
            out[i] = np.where(on, hi, lo)
        else:
            out[i] = np.where(_pattern(name, h, w, i, rng), 255, 0)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, n, h, w, level, connectivity, cap):
    """the model's (labels, header, records) of content(name, n, h, w), computed once and shared; read-only"""
    out = label(content(name, n, h, w), level, connectivity, cap)
    for a in out:
        a.setflags(write=False)
    return out


SHAPES = [(1, 1, 1), (2, 1, 40), (2, 40, 1), (3, 37, 53), (2, 150, 200), (1, 224, 224), (1, 685, 1055)]
LEVELS = (0, 127, 254, 255)
CAPS = (1, 7, 1024)


BIG = (("zeros", 0, 8, 7), ("zeros", 255, 4, 1), ("full", 127, 8, 1), ("full", 255, 4, 1024), ("checker", 127, 4, 7),
       ("checker", 254, 8, 1024), ("serpentine", 127, 4, 1024), ("serpentine", 0, 8, 1), ("spiral", 127, 4, 1024),
       ("spiral", 0, 8, 7), ("rings", 254, 8, 1024), ("rings", 127, 4, 7), ("uw", 127, 4, 1), ("uw", 0, 8, 1024),
       ("diagonal", 127, 8, 1024), ("diagonal", 0, 4, 7), ("random05", 127, 8, 1024), ("random05", 254, 4, 1),
       ("random41", 127, 8, 1024), ("random41", 254, 4, 7), ("random59", 127, 4, 1024), ("random59", 0, 8, 1),
       ("random90", 127, 8, 7), ("random90", 0, 4, 1024), ("straddle", 127, 8, 1024), ("straddle", 127, 4, 1),
       ("painted", 127, 8, 1024), ("painted", 127, 4, 7), ("lanes", 127, 8, 1024), ("lanes", 127, 4, 7))


def cases(n, h, w):
    """(content, level, connectivity, cap) for a shape.  Every frame but 685 x 1055: every content with both
    connectivities at level 127 and cap 1024; the contents with grey bytes (GREY) with both connectivities at every
    level; the contents whose bytes are only 0 and 255 - for them levels 0, 127 and 254 switch the same pixels on and
    255 none - with two or three of the four levels, cycling with the caps.  685 x 1055 takes a diagonal of that grid,
    written out in BIG: every content with both connectivities, the spiral, the serpentine and the random masks at
    the connectivity they are there for with the large cap, and level 255 only on `zeros` and `full`."""
    if h * w > 500000:
        return sorted(BIG)
    out = []
    for k, name in enumerate(CONTENTS):
        for conn in (4, 8):
            out.append((name, 127, conn, 1024))
            out.append((name, LEVELS[(k + conn // 4) % 4], conn, CAPS[k % 3]))
            if name in GREY:
                out += [(name, level, conn, CAPS[(k + j + conn // 4) % 3]) for j, level in enumerate(LEVELS)]
        out.append((name, LEVELS[(k + 3) % 4], (4, 8)[k % 2], CAPS[(k + 1) % 3]))
    return sorted(set(out))
