#!/usr/bin/env python3
"""Cost of lane following on the device (unet_lane_detection_amd/follow.py): the HSV extractor, the scan-row centre and
one callback of `LaneFollowPipeline`.

  python tools/follow_timing.py --out profiles/r21/lane_follow.md

One measurement in a fresh child process under its own time limit.  Three parts:
  (a) extractor  unet_hsv_lanes_u8_batch on 64 resident frames of 480 x 640 and of 685 x 1055, box sizes (5,5) and
                 (1,1): a sample is LAUNCHES back-to-back launches between two HIP events, divided by LAUNCHES; median
                 of ITERS samples after WARMUP, the input rotating over three buffers.  Bytes per second over the
                 algorithmic 4 bytes a pixel (3 read, 1 written).  The yardstick is a device-to-device copy measured
                 the same way in the same run that moves the same bytes: 2 bytes a pixel read and 2 written.
  (b) centre     unet_lane_center_u8_batch on 64 masks of 685 x 1055, 1 and 64 scan rows, measured the same way.
  (c) callback   `LaneFollowPipeline.process` (model A, f16x3, and the "hsv" source) against `LanePipelineGPU.process`
                 plus the reference's centre on the host (np.where, np.mean) - the path there was before: wall clock
                 of one callback, message bytes in to centre out, median of CALLBACKS after 5 warm-ups.
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

BATCH = 64
SIZES = ((480, 640), (685, 1055))
KSIZES = ((5, 5), (1, 1))
WARMUP, ITERS, LAUNCHES, CALLBACKS = 3, 20, 10, 40
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


def _painted(n, h, w, seed):
    """frames with white patches on random colours, so that the morphology has work to do"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
    coarse = torch.rand((n, 1, h // 16 + 1, w // 16 + 1), device="cuda", generator=g) < 0.3
    field = torch.nn.functional.interpolate(coarse.float(), size=(h, w), mode="nearest")[:, 0] > 0
    field ^= torch.rand((n, h, w), device="cuda", generator=g) < 0.05
    frames[field] = 230
    return frames


def measure():
    import ctypes as C

    import numpy as np
    import torch
    from unet_lane_detection_amd import _lib, follow as F, ros_bridge as RB, state as S
    from unet_lane_detection_amd.model import UNetHIP

    lib = _lib.load()
    lower, upper = np.array([0, 0, 185], dtype=np.uint8), np.array([180, 40, 255], dtype=np.uint8)

    ptr = _lib.ptr

    def hsv_launch(frames, kc, ko, mask):   # the entry point itself on preallocated buffers: no allocation in the timed loop
        n, h, w = frames.shape[:3]
        rc = lib.unet_hsv_lanes_u8_batch(0, ptr(frames), n, h, w, 1, lower.ctypes.data_as(C.c_void_p),
                                         upper.ctypes.data_as(C.c_void_p), kc, ko, ptr(mask),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "unet_hsv_lanes_u8_batch")

    def center_launch(masks, rows, sums):
        n, h, w = masks.shape
        rc = lib.unet_lane_center_u8_batch(0, ptr(masks), n, h, w, rows, len(rows), 127, ptr(sums),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "unet_lane_center_u8_batch")

    out = {"extractor": [], "center": [], "callback": {}}
    for h, w in SIZES:
        px = BATCH * h * w
        inputs = [_painted(BATCH, h, w, seed) for seed in (1, 2, 3)]
        src = [torch.randint(0, 256, (2 * px,), dtype=torch.uint8, device="cuda") for _ in range(3)]
        dst = torch.empty(2 * px, dtype=torch.uint8, device="cuda")
        copy_ms = _events_ms(lambda i: dst.copy_(src[i % 3]))
        for kc, ko in KSIZES:
            mask = torch.empty((BATCH, h, w), dtype=torch.uint8, device="cuda")
            hsv_launch(inputs[0], kc, ko, mask)
            assert torch.equal(mask, F.HSVLaneExtractor(close_ksize=kc, open_ksize=ko).extract(inputs[0]))
            share = float((mask == 255).float().mean())
            ms = _events_ms(lambda i: hsv_launch(inputs[i % 3], kc, ko, mask))
            out["extractor"].append({"h": h, "w": w, "kc": kc, "ko": ko, "ms": ms, "bytes": 4 * px, "share": share})
        copy_again = _events_ms(lambda i: dst.copy_(src[i % 3]))          # the yardstick's own spread: before and after
        out["extractor"].append({"h": h, "w": w, "copy": True, "ms": copy_ms, "ms_again": copy_again, "bytes": 4 * px})
        if (h, w) == SIZES[-1]:
            masks = [F.HSVLaneExtractor().extract(f) for f in inputs]
            for rows in ([int(h * 0.7)], [int(r) for r in np.linspace(0, h - 1, 64)]):
                arr = (C.c_int * len(rows))(*rows)
                sums = torch.empty((BATCH, len(rows), 2), dtype=torch.int32, device="cuda")
                ms = _events_ms(lambda i: center_launch(masks[i % 3], arr, sums))
                out["center"].append({"rows": len(rows), "ms": ms, "bytes": BATCH * len(rows) * w})
        del inputs, src, dst

    # (c) one callback
    model = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    img = _painted(1, 480, 640, 9)[0].cpu().numpy()
    msg = RB.ImageMsg(height=480, width=640, encoding="bgr8", data=img.tobytes())
    plain = RB.LanePipelineGPU(model, precision="f16x3")
    follow = F.LaneFollowPipeline(model, source="unet", precision="f16x3")
    hsv = F.LaneFollowPipeline(model, source="hsv")

    def parent():
        m = plain.process(msg)
        mask = np.frombuffer(m.data, dtype=np.uint8).reshape(m.height, m.width)
        xs = np.where(mask[int(mask.shape[0] * 0.7), :] > 127)[0]
        return int(np.mean(xs)) if len(xs) > 10 else None

    def wall(fn):
        for _ in range(5):
            got = fn()
        ts = []
        for _ in range(CALLBACKS):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts, got
    # alternating rounds, so that a drifting host shows in both
    res = {"parent": [], "follow": [], "hsv": []}
    for _ in range(2):
        for key, fn in (("parent", parent), ("follow", lambda: follow.process(msg)[0]), ("hsv", lambda: hsv.process(msg)[0])):
            ts, got = wall(fn)
            res[key] += ts
            res[key + "_centre"] = got
    assert res["parent_centre"] == res["follow_centre"], (res["parent_centre"], res["follow_centre"])
    assert model.device_error() == 0
    out["callback"] = res
    model.release()
    print("RESULT " + json.dumps(out))


def _md(m, out_path):
    med = statistics.median
    lines = ["# Lane following on the device: extractor, scan-row centre, one callback", "",
             "Produced by `python tools/follow_timing.py --out %s` on one MI355X, one process." % out_path, "",
             "## (a) `unet_hsv_lanes_u8_batch`, %d frames a launch" % BATCH, "",
             "A sample is %d back-to-back launches between two HIP events, divided by %d; median of %d samples after %d"
             % (LAUNCHES, LAUNCHES, ITERS, WARMUP),
             "warm-ups; the input rotates over three buffers.  GB/s is over the 4 bytes a pixel the algorithm has to move",
             "(3 read, 1 written).  The yardstick is `Tensor.copy_` of 2 bytes a pixel, device to device (2 read, 2 written:",
             "the same bytes), measured the same way before and after the extractor's rows.", "",
             "| frames | what | ms a launch | min .. max | GB/s | share of the copy's rate | lane share of the output |",
             "|---|---|---|---|---|---|---|"]
    copies = {(e["h"], e["w"]): e for e in m["extractor"] if e.get("copy")}
    for e in m["extractor"]:
        c = copies[(e["h"], e["w"])]
        copy_ms = med(c["ms"] + c["ms_again"])
        if e.get("copy"):
            for label, key in (("copy, before", "ms"), ("copy, after", "ms_again")):
                d = med(e[key])
                lines.append("| %d x %d | %s | %.4f | %.4f .. %.4f | %.0f | | |" % (e["h"], e["w"], label, d, min(e[key]), max(e[key]),
                                                                                   e["bytes"] / d / 1e6))
        else:
            d = med(e["ms"])
            lines.append("| %d x %d | close %d, open %d | %.4f | %.4f .. %.4f | %.0f | %.2f | %.3f |" % (
                e["h"], e["w"], e["kc"], e["ko"], d, min(e["ms"]), max(e["ms"]), e["bytes"] / d / 1e6, copy_ms / d, e["share"]))
    lines += ["", "## (b) `unet_lane_center_u8_batch`, %d masks of %d x %d" % (BATCH, SIZES[-1][0], SIZES[-1][1]), "",
              "Measured the same way; bytes are the scan rows read.", "",
              "| scan rows | ms a launch | min .. max | GB/s |", "|---|---|---|---|"]
    for e in m["center"]:
        d = med(e["ms"])
        lines.append("| %d | %.4f | %.4f .. %.4f | %.1f |" % (e["rows"], d, min(e["ms"]), max(e["ms"]), e["bytes"] / d / 1e6))
    r = m["callback"]
    lines += ["", "## (c) One callback: a 480 x 640 bgr8 message in, the lane centre out", "",
              "Wall clock on the host, model A on the f16x3 tier at 224 x 224, warp to 1055 x 685; %d callbacks each in two"
              % CALLBACKS,
              "alternating rounds after 5 warm-ups.  \"before\" is `LanePipelineGPU.process` (the 722 KB mask comes to the host)",
              "followed by the reference's `np.where` / `np.mean` on the scan row.", "",
              "| path | ms a callback, median | min .. max |", "|---|---|---|"]
    for label, key in (("before: process + centre on the host", "parent"), ("LaneFollowPipeline, source \"unet\"", "follow"),
                       ("LaneFollowPipeline, source \"hsv\"", "hsv")):
        lines.append("| %s | %.3f | %.3f .. %.3f |" % (label, med(r[key]), min(r[key]), max(r[key])))
    lines += ["", "Centres: before %s, \"unet\" %s, \"hsv\" %s." % (r["parent_centre"], r["follow_centre"], r["hsv_centre"]),
              "", "## Raw lines", "", "```"]
    for e in m["extractor"] + m["center"]:
        head = " ".join("%s=%s" % (k, v) for k, v in e.items() if not isinstance(v, list))
        for k, v in e.items():
            if isinstance(v, list):
                lines.append("%s %s: %s" % (head, k, " ".join("%.4f" % x for x in v)))
    for key in ("parent", "follow", "hsv"):
        lines.append("callback %s: %s" % (key, " ".join("%.3f" % x for x in r[key])))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="lane_follow.md")
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
