#!/usr/bin/env python3
"""Cost of rasterising annotations on the device (unet_lane_detection_amd/annotate.py).

  python tools/annotate_timing.py --out profiles/r27/annotate.md

Three parts, all in this one process, so that every figure of a row comes from the same run:
  (a) data sets   64 and 960 frames of 480 x 640 with three lane quads each, rasterised to 224 x 224 and to 480 x 640
                  by `unet_fill_polygons_u8_batch`.  A sample is LAUNCHES back-to-back calls between two HIP events,
                  divided by LAUNCHES; median, smallest and largest of ITERS samples after WARMUP.  Beside it, measured
                  the same way: a device-to-device copy of the output's bytes (the least any kernel that writes them
                  could take), and the same call on frames without polygons (tile set-up and stores, no edge).  On the
                  host, per frame over HOST_FRAMES frames: the numpy model of tests/annotate_model.py, the package's
                  host path and, where installed, Pillow's ImageDraw.polygon - the only host rasterisers there are here.
  (b) edges       one 480 x 640 frame with one polygon of 1, 10, 100 and 1000 edges at the source size: the slope is the
                  cost of an edge.
  (c) a stage     `TrainingSource.at(224)` for 960 frames (resize and rasterise, wall clock to a synchronise) against
                  one training step.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

H, W = 480, 640
WARMUP, ITERS, LAUNCHES = 3, 15, 10
HOST_FRAMES = 4
STEP_MS = 42.0        # one training step of the flagship model at batch 64, as measured at the parent commit (README)


def lane_frames(n, seed=0):
    """n frames of three lane quads: 4..28 pixels wide at the bottom row, a pixel wide at a horizon row"""
    import numpy as np
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(n):
        horizon, vanish = int(rng.integers(H // 3, H // 2)), int(rng.integers(W // 3, 2 * W // 3))
        polys = []
        for lane in range(3):
            w = int(rng.integers(4, 29))
            xb = int(rng.integers(0, W - w))
            xt = vanish + (lane - 1) * 6
            polys.append((np.array([[xb, H - 1], [xb + w, H - 1], [xt + 1, horizon], [xt, horizon]], dtype=np.int32), 255))
        frames.append(polys)
    return frames


def star(edges, seed=1):
    """one polygon of `edges` vertices around the frame centre"""
    import numpy as np
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, edges))
    rad = rng.uniform(0.2, 0.45, edges) * min(H, W)
    pts = np.stack([W / 2 + rad * np.cos(ang), H / 2 + rad * np.sin(ang)], axis=1).astype(np.int32)
    return [[(pts, 255)]]


def host_ms(fn, frames):
    """milliseconds per frame of fn(polygons) over the given frames: the median of three passes"""
    passes = []
    for _ in range(3):
        t0 = time.perf_counter()
        for polys in frames:
            fn(polys)
        passes.append((time.perf_counter() - t0) * 1e3 / len(frames))
    return statistics.median(passes)


def host_rasterisers(out_size):
    """name -> function(polygons) for one frame at out_size"""
    import annotate_model as AM
    from unet_lane_detection_amd import annotate as A
    fns = {"numpy model": lambda polys: AM.fill_polygons(polys, (H, W), out_size),
           "host path": lambda polys: A.rasterize(A.PolygonBatch([polys]), (H, W), out_size)}
    try:
        from PIL import Image, ImageDraw
    except ImportError:
        return fns
    if out_size == (H, W):        # Pillow draws at the source size only; a resize would be another operation
        def pillow(polys):
            img = Image.new("L", (W, H), 0)
            draw = ImageDraw.Draw(img)
            for pts, value in polys:
                xy = [(int(x), int(y)) for x, y in pts]
                if len(xy) > 1:
                    draw.polygon(xy, fill=value, outline=value)
                else:                 # Pillow's polygon wants two vertices
                    draw.point(xy, fill=value)
            return img
        fns["Pillow"] = pillow
    return fns


def events_ms(fn):
    import torch
    samples = []
    for it in range(WARMUP + ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            samples.append(a.elapsed_time(b) / LAUNCHES)
    return samples


def spread(samples):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(samples), min(samples), max(samples))


def measure():
    import annotate_model as AM
    import numpy as np
    import torch
    from unet_lane_detection_amd import annotate as A
    if not torch.cuda.is_available():
        raise SystemExit("annotate_timing needs a GPU: nothing here is measured without one")
    rows_a, rows_b = [], []
    for n in (64, 960):
        frames = lane_frames(n)
        batch = A.PolygonBatch(frames).to(0)
        empty = A.PolygonBatch([[] for _ in range(n)]).to(0)
        for out_size in ((224, 224), (H, W)):
            out = torch.empty((n,) + out_size, dtype=torch.uint8, device="cuda")
            other = torch.empty_like(out)
            kernel = events_ms(lambda: A.rasterize(batch, (H, W), out_size, out=out))
            bare = events_ms(lambda: A.rasterize(empty, (H, W), out_size, out=out))
            copy = events_ms(lambda: other.copy_(out))
            host = {k: host_ms(f, frames[:HOST_FRAMES]) for k, f in host_rasterisers(out_size).items()}
            # what was timed is what the model gives: the first and the last frames, bit for bit
            masks = A.rasterize(batch, (H, W), out_size, out=out)
            for i in list(range(HOST_FRAMES)) + [n - 1]:
                if not np.array_equal(masks[i].cpu().numpy(), AM.fill_polygons(frames[i], (H, W), out_size)):
                    raise SystemExit("frame %d of %d at %s differs from the model" % (i, n, out_size))
            covered = float((masks != 0).sum().item()) / masks.numel()
            rows_a.append(dict(n=n, out=out_size, bytes=out.numel(), kernel=kernel, bare=bare, copy=copy, host=host,
                               covered=covered))
    for edges in (1, 10, 100, 1000):
        frames = star(edges)
        batch = A.PolygonBatch(frames).to(0)
        out = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
        other = torch.empty_like(out)
        kernel = events_ms(lambda: A.rasterize(batch, (H, W), out=out))
        copy = events_ms(lambda: other.copy_(out))
        host = {k: host_ms(f, frames) for k, f in host_rasterisers((H, W)).items()}
        rows_b.append(dict(edges=edges, kernel=kernel, copy=copy, host=host))
    # (c) a whole stage: resize of the frames and rasterisation of the masks
    n = 960
    rng = np.random.default_rng(2)
    source = A.TrainingSource(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), A.PolygonBatch(lane_frames(n)), bgr=True)
    stage = []
    for it in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds = source.at(224)
        torch.cuda.synchronize()
        if it >= 2:
            stage.append((time.perf_counter() - t0) * 1e3)
        del ds
    props = torch.cuda.get_device_properties(0)
    return rows_a, rows_b, stage, "%s (%s)" % (props.name, getattr(props, "gcnArchName", "?").split(":")[0])


def report(rows_a, rows_b, stage, device):
    lines = ["# Annotations on the device: what the rasteriser costs", "",
             "`python tools/annotate_timing.py`, one process on %s.  Kernel and copy: milliseconds per call, a sample being"
             % device,
             "%d back-to-back calls between two HIP events; median (smallest .. largest) of %d samples after %d warm-up"
             % (LAUNCHES, ITERS, WARMUP),
             "samples.  Host figures: milliseconds per frame on the host's CPU, median of three passes over %d frames,"
             % HOST_FRAMES,
             "times n for the data set (extrapolated, not run).  Nothing here was profiled kernel by kernel.", "",
             "## (a) data sets of %d x %d frames, three lane quads each" % (H, W), "",
             "| frames | masks | output MB | kernel ms | no polygons ms | device copy ms | kernel / copy | host, ms per frame | host, whole set |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows_a:
        k, c = statistics.median(r["kernel"]), statistics.median(r["copy"])
        host = ", ".join("%s %.2f" % (name, ms) for name, ms in r["host"].items())
        whole = ", ".join("%s %.1f s" % (name, ms * r["n"] / 1e3) for name, ms in r["host"].items())
        lines.append("| %d | %d x %d | %.1f | %s | %s | %s | %.1f | %s | %s |" % (
            r["n"], r["out"][0], r["out"][1], r["bytes"] / 1e6, spread(r["kernel"]), spread(r["bare"]), spread(r["copy"]),
            k / c, host, whole))
    big = rows_a[-1]
    walk = 1.0 - statistics.median(big["bare"]) / statistics.median(big["kernel"])
    lines += ["", "Share of mask pixels set: %s.  The first %d frames and the last one of every row equal the numpy model"
              % (", ".join("%.4f" % r["covered"] for r in rows_a), HOST_FRAMES),
              "bit for bit (checked in this run).  Without polygons the call computes its tiles' source points and stores",
              "zeros; what the full call takes beyond that is the walk over the kept edges: %.0f %% of the last row's time."
              % (100.0 * walk),
              "The kernel is bound by its integer instructions, not by the bytes it writes.  A figure of about 0.01 ms is",
              "the floor of one Python call that enqueues one launch; kernel and enqueue were not separated.", "",
              "## (b) one %d x %d frame, one polygon of k edges" % (H, W), "",
              "| edges | kernel ms | device copy ms | host, ms per frame |", "|---|---|---|---|"]
    for r in rows_b:
        host = ", ".join("%s %.2f" % (name, ms) for name, ms in r["host"].items())
        lines.append("| %d | %s | %s | %s |" % (r["edges"], spread(r["kernel"]), spread(r["copy"]), host))
    lo, hi = rows_b[-2], rows_b[-1]
    per_edge = (statistics.median(hi["kernel"]) - statistics.median(lo["kernel"])) / (hi["edges"] - lo["edges"])
    lines += ["", "From %d to %d edges the call grows by %.2f microseconds an edge for the %d pixels of the frame."
              % (lo["edges"], hi["edges"], per_edge * 1e3, H * W), "",
              "## (c) a training stage: `TrainingSource.at(224)` for 960 frames of %d x %d" % (H, W), "",
              "Resize of the frames and rasterisation of the masks, wall clock to a device synchronise: %s ms"
              % spread(stage),
              "(median, smallest .. largest of %d after 2 warm-ups).  One training step of the flagship model at batch 64"
              % len(stage),
              "takes %.1f ms (measured at the parent commit, README): the stage's data set costs %.2f steps, once per stage;"
              % (STEP_MS, statistics.median(stage) / STEP_MS),
              "an epoch over 960 frames is 15 steps.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27", "annotate.md"))
    args = ap.parse_args()
    text = report(*measure())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
