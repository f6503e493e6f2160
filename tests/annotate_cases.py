"""TEST INFRASTRUCTURE ONLY - the cases tests/test_annotate_cpu.py and tests/test_annotate_gpu.py share.

HAND: frames whose expected bitmaps were worked out by hand from the rule's text (tests/annotate_model.py), one string
per row, a character per pixel ('.' = 0, '#' = 255, a digit d = 10 * d).  The CPU test holds the model to them; the GPU
test holds the kernel to the model on the same frames.  The generators below are seeded and depend on nothing else."""
import numpy as np

from annotate_model import lane_quad

BIG = 1 << 20
PALETTE = {".": 0, "#": 255, **{str(d): 10 * d for d in range(1, 10)}}


def bitmap(rows):
    return np.array([[PALETTE[c] for c in row] for row in rows], dtype=np.uint8)


SQUARE = [[0, 0], [4, 0], [4, 3], [0, 3]]
BOWTIE = [[0, 0], [6, 6], [6, 0], [0, 6]]
# eight two-vertex polygons from the centre of a 7 x 7 frame, one per octant
STAR_ENDS = [[6, 4], [4, 6], [2, 6], [0, 4], [0, 2], [2, 0], [4, 0], [6, 2]]
STAR_ROWS = ["..#.#..", "..#.#..", "##.#.##", "..###..", "##.#.##", "..#.#..", "..#.#.."]

# name -> (polygons in painter's order, (src_h, src_w), rows)
HAND = {
    # the left and right triangles are filled, the top and bottom ones are empty
    "bowtie": ([(BOWTIE, 255)], (7, 7),
               ["#.....#", "##...##", "###.###", "#######", "###.###", "##...##", "#.....#"]),
    # a horizontal and a vertical edge on the frame border; the right column and the bottom row are outline only
    "square_on_border": ([(SQUARE, 255)], (5, 6), ["#####.", "#####.", "#####.", "#####.", "......"]),
    # the vertex (4, 2) lies exactly on scan row 2: the row counts the lower edge only
    "vertex_on_row": ([([[0, 0], [4, 2], [0, 4]], 255)], (5, 5), ["#....", "###..", "#####", "####.", "##..."]),
    "dot": ([([[2, 1]], 255)], (3, 4), ["....", "..#.", "...."]),
    "octants": ([([[3, 3], end], 255) for end in STAR_ENDS], (7, 7), STAR_ROWS),
    "octants_reversed": ([([end, [3, 3]], 255) for end in STAR_ENDS], (7, 7), STAR_ROWS),
    "diagonal_45": ([([[1, 5], [5, 1]], 255)], (7, 7),
                    [".......", ".....#.", "....#..", "...#...", "..#....", ".#.....", "......."]),
    # left of, above and right of the frame; the one to the right crosses every row twice
    "outside": ([([[-10, -10], [-3, -10], [-3, -2], [-10, -2]], 255), ([[-9, 0], [-2, 1], [-5, 3]], 255),
                 ([[10, 0], [20, 0], [20, 3], [10, 3]], 255), ([[0, 9], [3, 9], [2, 30]], 255)], (4, 4),
                ["....", "....", "....", "...."]),
    "whole_frame": ([([[-5, -5], [50, -5], [50, 50], [-5, 50]], 70)], (5, 4), ["7777"] * 5),
    "duplicate_vertices": ([([[0, 0], [0, 0], [4, 0], [4, 3], [4, 3], [0, 3]], 255)], (5, 6),
                           ["#####.", "#####.", "#####.", "#####.", "......"]),
    # the largest coordinates: a triangle that covers the frame and, over it, the exact diagonal y = x
    "limits": ([([[-BIG, -BIG], [BIG, -BIG], [0, BIG]], 30), ([[-BIG, -BIG], [BIG, BIG]], 255)], (6, 6),
               ["#33333", "3#3333", "33#333", "333#33", "3333#3", "33333#"]),
    # painter's order: the second polygon overwrites the first, an empty one and a value of 0 included
    "painter": ([(SQUARE, 10), ([], 90), ([[2, 1], [5, 1], [5, 4], [2, 4]], 20), ([[0, 0], [1, 0], [1, 1], [0, 1]], 0)],
                (5, 6), ["..111.", "..2222", "112222", "112222", "..2222"]),
    # the holes of a bow-tie leave the earlier value
    "bowtie_over": ([([[-1, -1], [9, -1], [9, 9], [-1, 9]], 50), (BOWTIE, 255)], (7, 7),
                    ["#55555#", "##555##", "###5###", "#######", "###5###", "##555##", "#55555#"]),
}

# (src, out) of the resampling checks
RESAMPLE = [((9, 13), (5, 7)), ((5, 7), (9, 13)), ((480, 640), (224, 224))]


def lane_frame(rng, height, width, count=3):
    """`count` lane quads of bottom width 1..7 that leave the frame at the bottom and narrow to a pixel at the top"""
    polys = []
    for _ in range(count):
        w = int(rng.integers(1, 8))
        xb, xt = int(rng.integers(0, max(1, width - w))), int(rng.integers(0, width))
        polys.append((lane_quad(xb, xt, w, height), 255))
    return polys


def random_polygons(rng, height, width, count, spread=1.0, max_vertices=9, near=0.0):
    """polygons with 0 .. max_vertices vertices whose coordinates reach `spread` frame sizes beyond the frame; the share
    `near` of the vertices lies within 0.3 frame sizes of the frame instead, so that long edges pass through it"""
    polys = []
    for _ in range(count):
        k = int(rng.integers(0, max_vertices + 1))
        xs = rng.integers(-int(spread * width), int((1 + spread) * width) + 1, k)
        ys = rng.integers(-int(spread * height), int((1 + spread) * height) + 1, k)
        close = rng.random(k) < near
        xs = np.where(close, rng.integers(-int(0.3 * width), int(1.3 * width) + 1, k), xs)
        ys = np.where(close, rng.integers(-int(0.3 * height), int(1.3 * height) + 1, k), ys)
        polys.append((np.stack([xs, ys], axis=1).astype(np.int32).reshape(-1, 2), int(rng.integers(1, 256))))
    return polys


def resample_polygons(src):
    """what the resampling checks draw: three lanes, a star and a two-valued pair, sized by the source"""
    h, w = src
    rng = np.random.default_rng(h * 1000 + w)
    return lane_frame(rng, h, w) + random_polygons(rng, h, w, 3, spread=0.2)


def star_polygon(rng, height, width):
    """3..11 vertices at sorted angles around the frame centre, radii 0.2..0.7 of the short side, truncated to int"""
    k = int(rng.integers(3, 12))
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, k))
    rad = rng.uniform(0.2, 0.7, k) * min(height, width)
    xs = (width / 2.0 + rad * np.cos(ang)).astype(np.int32)
    ys = (height / 2.0 + rad * np.sin(ang)).astype(np.int32)
    return np.stack([xs, ys], axis=1)


def zigzag(count, height, width):
    """a saw of `count` vertices, a tooth every 8 columns from above the frame to below it, that runs across the frame
    again and again: every edge meets every row, the teeth leave gaps, and the repeats differ by a few rows outside the
    frame, so that the parity is neither all odd nor all even"""
    i = np.arange(count)
    teeth = (width + 16) // 8
    xs = 8 * ((i // 2) % teeth) + 3 * (i % 2) - 4
    ys = np.where(i % 2 == 0, -3 - (i // 2) % 5, height + 2 + (i // 2) % 3)
    return np.stack([xs, ys], axis=1).astype(np.int32)
