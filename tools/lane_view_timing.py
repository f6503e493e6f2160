#!/usr/bin/env python3
"""Cost of the lane view on the device (unet_lane_detection_amd/laneview.py): the kernel against a copy of the bytes it
must move, what each of its parts costs, and one callback of `LaneFollowPipeline` with the view on and off.

  python tools/lane_view_timing.py --out profiles/r25/lane_view.md

One measurement in a fresh child process under its own time limit.  Three parts:
  (a) kernel    unet_lane_view_u8_batch on 1 and on 64 resident frames of 480 x 640 through the reference's matrix
                onto 1055 x 685, the curves being the lane fits of the painted masks: a sample is LAUNCHES back-to-back
                launches between two HIP events, divided by LAUNCHES; median of ITERS samples after WARMUP, the frames
                rotating over three buffers.  With and without the mask layer.  Beside each, measured the same way in
                the same run, `Tensor.copy_` of the same n * h * w * 3 bytes, device to device (it reads them once and
                writes them once: the 6 bytes a pixel the kernel must move).
  (b) parts     the same launch with pieces left out through the entry point's own arguments - no curves; the layer
                plane only (no frame is read, no pixel blended or written: the position's double-precision arithmetic,
                its divide first of all, and one byte a pixel are left) - so that the table says what holds the whole
                back.
  (c) callback  `LaneFollowPipeline.process` (model A, f16x3, fit=FitConfig()) with view=ViewConfig() and with
                view=None, against the path there was before for the same picture: `process(return_mask=True)` - the
                722 KB mask comes to the host - plus the numpy model of the view (tests/laneview_model.py) on it.  Wall
                clock of one callback, message bytes in to the view on the device (host path: on the host), median of
                CALLBACKS after 5 warm-ups, alternating rounds.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 480, 640
BATCHES = (1, 64)
WARMUP, ITERS, LAUNCHES, CALLBACKS, HOST_CALLBACKS = 3, 20, 10, 30, 6
LIMIT = 420


def _events_ms(fn, launches=LAUNCHES):
    """fn(i) enqueues launch i; -> ITERS samples of milliseconds per launch"""
    import torch
    ts = []
    k = 0
    for it in range(WARMUP + ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn(k)
            k += 1
        b.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            ts.append(a.elapsed_time(b) / launches)
    return ts


def measure():
    import ctypes as C

    import numpy as np
    import torch

    import follow_model as FM
    import lanefit_model as LM
    import laneview_model as VM
    from unet_lane_detection_amd import _lib, follow as F, lanefit as LF, laneview as LV, ros_bridge as RB, state as S
    from unet_lane_detection_amd.model import UNetHIP

    lib = _lib.load()
    warp = RB.REF_WARP_SIZE
    matrix = LV.orient(RB.get_perspective_transform(RB.REF_SRC_POINTS, RB.REF_DST_POINTS), warp)
    m9 = np.ascontiguousarray(matrix.reshape(9))
    cfg = LV.ViewConfig()
    style = cfg.style()

    ptr = _lib.ptr

    def launch(frames, masks, table, view, plane):     # the entry point itself on preallocated buffers
        n = frames.shape[0]
        rc = lib.unet_lane_view_u8_batch(0, ptr(frames), n, H, W, 3 * W, m9.ctypes.data_as(C.POINTER(C.c_double)), warp[0],
                                         warp[1], ptr(masks), cfg.level, ptr(table), 0 if table is None else table.shape[1],
                                         C.byref(style), ptr(view), ptr(plane),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "unet_lane_view_u8_batch")

    out = {"kernel": [], "callback": {}}
    painted = LM.painted_lanes(11, 9, warp[1], warp[0])[:8]                           # 8 masks with both markings
    camera = FM.painted_frames(5, 8, H, W)[0]
    for n in BATCHES:
        masks = torch.from_numpy(painted[np.arange(n) % 8]).cuda()
        fits = LF.lane_fits(masks)
        table = torch.from_numpy(LV.curve_table(fits, warp, cfg)).cuda()
        frames = [torch.from_numpy(np.roll(camera[(np.arange(n) + r) % 8], 5 * r, axis=2)).cuda().contiguous() for r in range(3)]
        view = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        plane = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        # what is timed is what the tests compare: frame 0 against the numpy model
        launch(frames[0], masks, table, view, plane)
        want = VM.lane_view(frames[0][:1].cpu().numpy(), matrix, warp[0], warp[1], masks[:1].cpu().numpy(), cfg.level,
                            table[:1].cpu().numpy(), VM.Style())
        assert np.array_equal(view[0].cpu().numpy(), want[0][0]) and np.array_equal(plane[0].cpu().numpy(), want[1][0])
        layer_share = np.bincount(plane.cpu().numpy().reshape(-1), minlength=5)[:5] / plane.numel()
        dst = torch.empty_like(view)
        e = {"n": n, "bytes": n * H * W * 6, "layer_share": [float(v) for v in layer_share]}
        e["copy"] = _events_ms(lambda i: dst.copy_(frames[i % 3]))
        e["full"] = _events_ms(lambda i: launch(frames[i % 3], masks, table, view, None))
        e["full_plane"] = _events_ms(lambda i: launch(frames[i % 3], masks, table, view, plane))
        e["no_mask"] = _events_ms(lambda i: launch(frames[i % 3], None, table, view, None))
        e["no_curves"] = _events_ms(lambda i: launch(frames[i % 3], masks, None, view, None))
        e["blend_only"] = _events_ms(lambda i: launch(frames[i % 3], None, None, view, None))
        e["plane_only"] = _events_ms(lambda i: launch(frames[i % 3], masks, table, None, plane))
        e["position_only"] = _events_ms(lambda i: launch(frames[i % 3], None, None, None, plane))
        e["copy_again"] = _events_ms(lambda i: dst.copy_(frames[i % 3]))     # the yardstick's own spread
        out["kernel"].append(e)
        del frames, view, plane, dst

    # (c) one callback
    model = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).numpy()
    img[:, 150:170] = 240
    img[:, 470:490] = 240
    msg = RB.ImageMsg(height=H, width=W, encoding="bgr8", data=img.tobytes())
    fit = LF.FitConfig()
    plain = F.LaneFollowPipeline(model, source="unet", precision="f16x3", fit=fit)
    viewed = F.LaneFollowPipeline(model, source="unet", precision="f16x3", fit=fit, view=cfg)
    hosted = F.LaneFollowPipeline(model, source="unet", precision="f16x3", fit=fit)

    def parent():
        (centres, mm), fits = hosted.process(msg, return_mask=True)
        mask = np.frombuffer(mm.data, dtype=np.uint8).reshape(1, mm.height, mm.width)
        return VM.lane_view(img[None], matrix, warp[0], warp[1], mask, cfg.level, LV.curve_table(fits, warp, cfg), VM.Style())[0]

    def device():
        viewed.process(msg)
        return viewed.last_view

    def wall(fn, count):
        for _ in range(2 if count < CALLBACKS else 5):
            got = fn()
        ts = []
        for _ in range(count):
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts, got
    res = {"parent": [], "view": [], "plain": []}
    got = {}
    for _ in range(2):     # alternating rounds, so that a drifting host shows in all three
        for key, fn, count in (("parent", parent, HOST_CALLBACKS), ("view", device, CALLBACKS),
                               ("plain", lambda: plain.process(msg), CALLBACKS)):
            ts, got[key] = wall(fn, count)
            res[key] += ts
    hosted.tracker.reset()      # the two trackers have seen different numbers of frames: one more step from the same state
    viewed.tracker.reset()
    assert np.array_equal(device().cpu().numpy(), parent())             # both paths draw the same picture
    res["view_msg_ms"] = wall(lambda: viewed.view_msg(), CALLBACKS)[0]
    res["layers"] = [int(v) for v in np.bincount(viewed.last_view_layers.cpu().numpy().reshape(-1), minlength=5)[:5]]
    assert model.device_error() == 0
    out["callback"] = res
    model.release()
    print("RESULT " + json.dumps(out))


ROWS = (("copy, before", "copy"), ("view: mask, 2 curves, area", "full"), ("the same and the layer plane", "full_plane"),
        ("view without the mask layer", "no_mask"), ("view without curves (mask only)", "no_curves"),
        ("view without mask and curves (position + blend)", "blend_only"),
        ("layer plane only (no frame read, no blend)", "plane_only"),
        ("layer plane only, no mask, no curves (the position alone)", "position_only"), ("copy, after", "copy_again"))


def _md(m, out_path):
    med = statistics.median
    lines = ["# Lane view on the device: the kernel against a copy, its parts, one callback", "",
             "Produced by `python tools/lane_view_timing.py --out %s` on one MI355X, one process." % out_path, "",
             "## (a), (b) `unet_lane_view_u8_batch`: 480 x 640 frames, the reference's matrix, 1055 x 685 masks", "",
             "A sample is %d back-to-back launches between two HIP events, divided by %d; median of %d samples after %d"
             % (LAUNCHES, LAUNCHES, ITERS, WARMUP),
             "warm-ups; the frames rotate over three buffers.  The curves are the lane fits of the painted masks (left and",
             "right, the area between them filled), default style.  GB/s is over the 6 bytes a pixel the view must move (3",
             "read, 3 written) for every row, also those that move less or more.  The yardstick is `Tensor.copy_` of the",
             "same n h w 3 bytes, device to device, measured the same way before and after the kernel's rows.", "",
             "| frames | what | ms a launch | min .. max | GB/s | time / copy's time |", "|---|---|---|---|---|---|"]
    for e in m["kernel"]:
        copy_ms = med(e["copy"] + e["copy_again"])
        for label, key in ROWS:
            d = med(e[key])
            ratio = "" if key.startswith("copy") else "%.2f" % (d / copy_ms)
            lines.append("| %d | %s | %.4f | %.4f .. %.4f | %.1f | %s |" % (e["n"], label, d, min(e[key]), max(e[key]),
                                                                          e["bytes"] / d / 1e6, ratio))
    lines += ["", "Share of the pixels on layers 0 .. 4 (nothing, area, marking, left curve, right curve): %s." % "; ".join(
        ", ".join("%.3f" % v for v in e["layer_share"]) for e in m["kernel"]), "",
        "What holds it back, from the differences of the rows above (medians, ms a launch):", "",
        "| frames | view / copy | position (fp64, the divide) | + frame in, blend, view out | + curves | + mask gather |",
        "|---|---|---|---|---|---|"]
    for e in m["kernel"]:
        copy_ms = med(e["copy"] + e["copy_again"])
        full = med(e["full"])
        lines.append("| %d | %.1f | %.4f | %.4f | %.4f | %.4f |" % (
            e["n"], full / copy_ms, med(e["position_only"]), med(e["blend_only"]) - med(e["position_only"]),
            med(e["no_mask"]) - med(e["blend_only"]), full - med(e["no_mask"])))
    lines += ["", "\"position\" is the launch that writes the layer plane only, without mask and curves: three multiply-add pairs and",
              "one divide in double precision a pixel, one byte a pixel written.  The next columns are what each further part adds.",
              "The gather's pattern: a thread's 16 pixels are neighbours, but the 64 lanes of a wave are 16 pixels apart, which the",
              "matrix spreads over the bird's-eye mask, so each of a pixel's four byte loads touches another cache line in every",
              "lane.  Not tried: handing the gather to lanes that hold neighbouring pixels (a transpose of the run through LDS),",
              "and stepping the position along a row in fixed point instead of a divide a pixel.", ""]
    r = m["callback"]
    lines += ["## (c) One callback: a 480 x 640 bgr8 message in, the camera-view picture out", "",
              "Wall clock on the host up to a device synchronise, model A on the f16x3 tier at 224 x 224, warp to 1055 x 685,",
              "fit=FitConfig(); %d callbacks each in two alternating rounds after 5 warm-ups (%d for the host path)."
              % (CALLBACKS, HOST_CALLBACKS),
              "\"before\" is `process(return_mask=True)` - the 722 KB mask comes to the host - followed by the numpy model of the",
              "view (tests/laneview_model.py); it is the only host implementation there is, not a tuned one.", "",
              "| path | ms a callback, median | min .. max |", "|---|---|---|"]
    for label, key in (("before: process(return_mask=True) + the view on the host", "parent"),
                       ("LaneFollowPipeline(fit=..., view=ViewConfig())", "view"),
                       ("LaneFollowPipeline(fit=..., view=None)", "plain"),
                       ("view_msg(): the 921 600 bytes to the host", "view_msg_ms")):
        lines.append("| %s | %.3f | %.3f .. %.3f |" % (label, med(r[key]), min(r[key]), max(r[key])))
    lines += ["", "The view adds %.3f ms to a callback (median with it minus median without).  Both paths drew the same"
              % (med(r["view"]) - med(r["plain"])),
              "picture, bit for bit; its pixels per layer 0 .. 4: %s." % r["layers"], "", "## Raw lines", "", "```"]
    for e in m["kernel"]:
        for k, v in e.items():
            if isinstance(v, list) and k != "layer_share":
                lines.append("n=%d %s: %s" % (e["n"], k, " ".join("%.4f" % x for x in v)))
    for key in ("parent", "view", "plain", "view_msg_ms"):
        lines.append("callback %s: %s" % (key, " ".join("%.3f" % x for x in r[key])))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="lane_view.md")
    args = ap.parse_args()
    if args.step:
        measure()
        return 0
    p = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", "measure"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        print(p.stdout[-4000:])
        print("the measurement ended with status %d" % p.returncode)
        return p.returncode or 1
    result = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(_md(result, args.out))
    print("written " + args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
