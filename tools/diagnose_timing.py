#!/usr/bin/env python3
"""Cost of the diagnostics on the device (unet_lane_detection_amd/diagnose.py): the frame statistics, the probability
statistics and one callback of `LaneFollowPipeline` with `diagnose` on and off.

  python tools/diagnose_timing.py --out profiles/r22/diagnose.md

One measurement in a fresh child process under its own time limit.  Three parts:
  (a) frames     unet_frame_stats_u8_batch on 64 resident frames of 480 x 640, dense and in rows of 3 * 640 + 16 bytes,
                 and on one frame: a sample is LAUNCHES back-to-back calls (each the record-setting launch and the
                 kernel) between two HIP events, divided by LAUNCHES; median of ITERS samples after WARMUP, the input
                 rotating over three buffers.  Bytes per second over the 3 bytes a pixel the call has to read.  The
                 yardstick is a device-to-device copy of the same bytes (3 read and 3 written a pixel), measured the
                 same way in the same run, before and after.
  (b) planes     unet_prob_stats_f32_batch on 256 planes of 224 x 224 floats, beside a copy of those bytes.
  (c) callback   `LaneFollowPipeline.process` on a 480 x 640 bgr8 message, sources "hsv" and "unet" (model A, f16x3),
                 with diagnose=False - the path as it was - and diagnose=True: wall clock of one callback, message bytes
                 in to centres (and statistics) out, median of CALLBACKS after 5 warm-ups, in alternating rounds.
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

BATCH, H, W, PAD = 64, 480, 640, 16
PLANES, PLANE = 256, 224 * 224
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


def measure():
    import ctypes as C

    import numpy as np
    import torch
    from unet_lane_detection_amd import _lib, diagnose as D, follow as F, ros_bridge as RB, state as S
    from unet_lane_detection_amd.model import UNetHIP

    lib = _lib.load()

    ptr = _lib.ptr

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def frames_launch(buf, n, stride, rec):   # the entry point itself on preallocated buffers
        _lib.check(lib.unet_frame_stats_u8_batch(0, ptr(buf), n, H, W, stride, 1, ptr(rec), stream()),
                   "unet_frame_stats_u8_batch")

    def planes_launch(buf, rec):
        _lib.check(lib.unet_prob_stats_f32_batch(0, ptr(buf), PLANES, PLANE, 0.5, ptr(rec), stream()),
                   "unet_prob_stats_f32_batch")

    out = {"frames": [], "planes": [], "callback": {}}
    g = torch.Generator(device="cuda").manual_seed(1)

    # (a) frames
    nbytes = BATCH * H * W * 3
    src = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(3)]
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rec = torch.empty((BATCH, 8), dtype=torch.int64, device="cuda")
    copy_ms = _events_ms(lambda i: dst.copy_(src[i % 3]))
    frames_launch(src[0], BATCH, 0, rec)
    assert np.array_equal(rec.cpu().numpy(), D.frame_records(src[0], BATCH, H, W).cpu().numpy())
    ms = _events_ms(lambda i: frames_launch(src[i % 3], BATCH, 0, rec))
    out["frames"].append({"what": "%d frames, dense" % BATCH, "ms": ms, "bytes": nbytes})
    stride = 3 * W + PAD
    padded = [torch.randint(0, 256, (BATCH * H * stride,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(3)]
    ms = _events_ms(lambda i: frames_launch(padded[i % 3], BATCH, stride, rec))
    out["frames"].append({"what": "%d frames, rows of %d bytes" % (BATCH, stride), "ms": ms, "bytes": nbytes})
    ms = _events_ms(lambda i: frames_launch(src[i % 3], 1, 0, rec))
    out["frames"].append({"what": "1 frame, dense", "ms": ms, "bytes": nbytes // BATCH})
    copy_again = _events_ms(lambda i: dst.copy_(src[i % 3]))
    out["frames"].append({"what": "copy", "copy": True, "ms": copy_ms, "ms_again": copy_again, "bytes": 2 * nbytes})
    del src, dst, padded

    # (b) probability planes
    planes = [torch.rand((PLANES, PLANE), dtype=torch.float32, device="cuda", generator=g) for _ in range(3)]
    pdst = torch.empty_like(planes[0])
    prec = torch.empty((PLANES, 4), dtype=torch.int64, device="cuda")
    pcopy = _events_ms(lambda i: pdst.copy_(planes[i % 3]))
    ms = _events_ms(lambda i: planes_launch(planes[i % 3], prec))
    pcopy_again = _events_ms(lambda i: pdst.copy_(planes[i % 3]))
    out["planes"].append({"what": "%d planes of 224 x 224" % PLANES, "ms": ms, "bytes": PLANES * PLANE * 4})
    out["planes"].append({"what": "copy", "copy": True, "ms": pcopy, "ms_again": pcopy_again, "bytes": 2 * PLANES * PLANE * 4})
    del planes, pdst

    # (c) one callback
    model = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g).cpu().numpy()
    msg = RB.ImageMsg(height=H, width=W, encoding="bgr8", data=img.tobytes())
    pipes = {"hsv_off": F.LaneFollowPipeline(None, source="hsv"),
             "hsv_on": F.LaneFollowPipeline(None, source="hsv", diagnose=True),
             "unet_off": F.LaneFollowPipeline(model, source="unet", precision="f16x3"),
             "unet_on": F.LaneFollowPipeline(model, source="unet", precision="f16x3", diagnose=True)}

    def wall(fn):
        for _ in range(5):
            got = fn()
        ts = []
        for _ in range(CALLBACKS):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts, got
    res = {k: [] for k in pipes}
    got = {}
    for _ in range(2):   # alternating rounds, so that a drifting host shows in both
        for key, pipe in pipes.items():
            ts, got[key] = wall(lambda: pipe.process(msg))
            res[key] += ts
    assert got["hsv_on"][0] == got["hsv_off"] and got["unet_on"][0] == got["unet_off"]
    assert np.array_equal(got["hsv_on"][1].words, got["unet_on"][1].words)
    assert model.device_error() == 0
    res["report"] = got["hsv_on"][1].report(0)
    out["callback"] = res
    model.release()
    print("RESULT " + json.dumps(out))


def _table(lines, entries):
    med = statistics.median
    copy = [e for e in entries if e.get("copy")][0]
    copy_ms = med(copy["ms"] + copy["ms_again"])
    lines += ["| what | ms a call | min .. max | GB/s | the copy's time over the call's |", "|---|---|---|---|---|"]
    for e in entries:
        if e.get("copy"):
            for label, key in (("copy of those bytes, before", "ms"), ("copy of those bytes, after", "ms_again")):
                d = med(e[key])
                lines.append("| %s | %.4f | %.4f .. %.4f | %.0f (read + written) | |" % (label, d, min(e[key]), max(e[key]),
                                                                                        e["bytes"] / d / 1e6))
        else:
            d = med(e["ms"])
            ratio = ("%.2f" % (copy_ms / d)) if e["bytes"] * 2 == copy["bytes"] else ""
            lines.append("| %s | %.4f | %.4f .. %.4f | %.0f (read) | %s |" % (e["what"], d, min(e["ms"]), max(e["ms"]),
                                                                             e["bytes"] / d / 1e6, ratio))


def _md(m, out_path):
    med = statistics.median
    lines = ["# Diagnostics on the device: frame statistics, probability statistics, one callback", "",
             "Produced by `python tools/diagnose_timing.py --out %s` on one MI355X, one process." % out_path, "",
             "## (a) `unet_frame_stats_u8_batch`, frames of %d x %d" % (H, W), "",
             "A sample is %d back-to-back calls between two HIP events, divided by %d; median of %d samples after %d warm-ups;"
             % (LAUNCHES, LAUNCHES, ITERS, WARMUP),
             "the input rotates over three buffers.  A call is two launches: the one that sets the records and the kernel.",
             "GB/s is over the 3 bytes a pixel the call reads.  The yardstick is `Tensor.copy_` of the 64 frames' bytes, device",
             "to device (it reads and writes them), measured the same way before and after.", ""]
    _table(lines, m["frames"])
    lines += ["", "## (b) `unet_prob_stats_f32_batch`", "", "Measured the same way; the copy moves the planes' bytes.", ""]
    _table(lines, m["planes"])
    r = m["callback"]
    lines += ["", "## (c) One callback: a %d x %d bgr8 message in, the lane centres out" % (H, W), "",
              "Wall clock on the host, warp to 1055 x 685; %d callbacks each in two alternating rounds after 5 warm-ups."
              % CALLBACKS,
              "`diagnose=False` is the path as it was; with `diagnose=True` the message's rows are measured on the device and",
              "64 more bytes are read back.", "",
              "| path | ms a callback, median | min .. max |", "|---|---|---|"]
    for label, key in (("source \"hsv\", diagnose=False", "hsv_off"), ("source \"hsv\", diagnose=True", "hsv_on"),
                       ("source \"unet\" (model A, f16x3), diagnose=False", "unet_off"),
                       ("source \"unet\" (model A, f16x3), diagnose=True", "unet_on")):
        lines.append("| %s | %.3f | %.3f .. %.3f |" % (label, med(r[key]), min(r[key]), max(r[key])))
    lines += ["", "Difference of the medians: \"hsv\" %+.3f ms, \"unet\" %+.3f ms." % (
        med(r["hsv_on"]) - med(r["hsv_off"]), med(r["unet_on"]) - med(r["unet_off"])), "",
        "The message's report (uniformly random bytes):", "", "```"] + r["report"] + ["```", "", "## Raw lines", "", "```"]
    for e in m["frames"] + m["planes"]:
        for k, v in e.items():
            if isinstance(v, list):
                lines.append("%s %s: %s" % (e["what"], k, " ".join("%.4f" % x for x in v)))
    for key in ("hsv_off", "hsv_on", "unet_off", "unet_on"):
        lines.append("callback %s: %s" % (key, " ".join("%.3f" % x for x in r[key])))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="diagnose.md")
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
