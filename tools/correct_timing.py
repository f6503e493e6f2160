#!/usr/bin/env python3
"""Cost and effect of the frame correction on the device (unet_lane_detection_amd/correct.py).

  python tools/correct_timing.py --out profiles/r26/correct.md [--parent PATH]

Every measurement runs in a fresh child process under its own time limit.  Three parts:
  (a) the call   unet_correct_u8_batch on 64 resident frames of 480 x 640 and on one frame, every stage alone, all of
                 them, none of them (the histograms, the plan and the table pass still run), and all of them in rows
                 of 3 * 640 + 5 bytes (the byte path of the apply pass): a sample is LAUNCHES back-to-back calls
                 between two HIP events, divided by LAUNCHES; median of ITERS samples after WARMUP, the input rotating
                 over three buffers.  The yardstick is a device-to-device copy of the same bytes (the call also reads
                 and writes every byte once, and reads them once or twice more for the histograms), measured the same
                 way in the same process, before and after.  The frames are a ramp with blocks and noise, not uniform
                 noise: the histogram passes count into LDS, and how many lanes of a wave meet in one counter depends on
                 the content.  A flat frame - all lanes in one counter - is measured too.
  (b) callback   `LaneFollowPipeline.process` on a 480 x 640 bgr8 message, sources "hsv" and "unet" (model A, f16x3):
                 correct=None, gray world alone, and every stage.  Wall clock of one callback, median of CALLBACKS after
                 5 warm-ups, in alternating rounds.  With --parent PATH (a checkout of the parent commit with its library
                 built) the same callback without the argument is measured from that checkout in a process of its own,
                 right after.
  (c) effect     `HSVLaneExtractor.evaluate` (IoU against the painted markings) on synthetic tracks: as painted, under a
                 blue-deficient cast (blue * 0.7), and the cast frames after the gray-world correction.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH, H, W, PAD = 64, 480, 640, 5
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


def _scene(n, seed):
    """(n, H, W, 3) uint8 on the host: a cast, a brightness ramp, blocks, noise"""
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((n, H, W, 3), dtype=np.uint8)
    for i in range(n):
        img = np.zeros((H, W, 3), dtype=np.int64)
        for c, base in enumerate((50, 100, 140)):
            img[..., c] = base + (xx * 70) // (W - 1) + (yy * 35) // (H - 1) + rng.integers(-12, 13, (H, W))
        for _ in range(6):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            img[y0:y0 + H // 4, x0:x0 + W // 4] += int(rng.integers(-60, 90))
        out[i] = np.clip(img, 0, 255)
    return out


def _tracks(n):
    """(frames (n,H,W,3) uint8 BGR, targets (n,H,W) uint8): a gray surface (100 +- 6) with two white markings (240 +- 6)
    whose position and width change from frame to frame"""
    import numpy as np
    rng = np.random.default_rng(7)
    frames = np.empty((n, H, W, 3), dtype=np.uint8)
    targets = np.zeros((n, H, W), dtype=np.uint8)
    for i in range(n):
        shift, half_w = int(rng.integers(-60, 61)), int(rng.integers(8, 15))
        for y in range(H):
            half = W // 10 + (W // 4) * y // H
            for centre in (W // 2 + shift - half, W // 2 + shift + half):
                targets[i, y, max(centre - half_w, 0):max(centre + half_w, 0)] = 1
        level = np.where(targets[i] > 0, 240, 100)[..., None] + rng.integers(-6, 7, (H, W, 1))
        frames[i] = np.clip(level, 0, 255)
    return frames, targets


def measure_call():
    import ctypes as C

    import numpy as np
    import torch
    from unet_lane_detection_amd import _lib, correct as K

    lib = _lib.load()

    ptr = _lib.ptr

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    configs = [("no stage (histograms, plan, table pass)", K.CorrectConfig(white_balance=None)),
               ("white balance", K.CorrectConfig()),
               ("stretch 1 % / 1 %", K.CorrectConfig(white_balance=None, stretch=(1.0, 1.0))),
               ("tone (gamma 0.8)", K.CorrectConfig(white_balance=None, gamma=0.8)),
               ("CLAHE 2.0, 8 x 8", K.CorrectConfig(white_balance=None, clahe=K.Clahe())),
               ("all four", K.CorrectConfig(stretch=(1.0, 1.0), gamma=0.8, clahe=K.Clahe()))]
    nbytes = BATCH * H * W * 3
    base = _scene(4, 3)
    host = np.stack([base[i % 4] for i in range(BATCH)])
    src = [torch.from_numpy(np.roll(host, k, axis=0).copy()).cuda().view(-1) for k in range(3)]
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    work = torch.empty(lib.unet_correct_work_bytes(BATCH, 8, 8), dtype=torch.uint8, device="cuda")

    def launch(cfg, buf, n, stride=0, out=None):
        _lib.check(lib.unet_correct_u8_batch(0, ptr(buf), n, H, W, stride, 1, C.byref(cfg), ptr(dst if out is None else out),
                                             stride, ptr(work), work.numel(), stream()), "unet_correct_u8_batch")

    out = {"call": []}
    copy_ms = _events_ms(lambda i: dst.copy_(src[i % 3]))
    one = [s[:nbytes // BATCH] for s in src]
    copy1_ms = _events_ms(lambda i: dst[:nbytes // BATCH].copy_(one[i % 3]))
    for label, config in configs:
        cfg = config.struct()
        ms = _events_ms(lambda i: launch(cfg, src[i % 3], BATCH))
        out["call"].append({"what": label, "n": BATCH, "ms": ms})
        ms = _events_ms(lambda i: launch(cfg, src[i % 3], 1))
        out["call"].append({"what": label, "n": 1, "ms": ms})
    cfg = configs[-1][1].struct()
    stride = 3 * W + PAD
    rows = torch.zeros((BATCH, H, stride), dtype=torch.uint8, device="cuda")
    rows[:, :, :3 * W] = src[0].view(BATCH, H, 3 * W)
    rows_out = torch.empty_like(rows)
    ms = _events_ms(lambda i: launch(cfg, rows, BATCH, stride, rows_out))
    out["call"].append({"what": "all four, rows of %d bytes (byte path)" % stride, "n": BATCH, "ms": ms})
    launch(cfg, src[0], BATCH)
    torch.cuda.synchronize()
    assert torch.equal(rows_out[:, :, :3 * W].reshape(-1), dst), "the two paths of the apply pass differ"
    ms = _events_ms(lambda i: launch(cfg, src[0], BATCH, 0, src[0]))
    out["call"].append({"what": "all four, in place (the same frames again and again)", "n": BATCH, "ms": ms})
    flat = torch.full((nbytes,), 93, dtype=torch.uint8, device="cuda")
    ms = _events_ms(lambda i: launch(cfg, flat, BATCH))
    out["call"].append({"what": "all four, flat frames (every lane in one counter)", "n": BATCH, "ms": ms})
    out["copy"] = {"ms": copy_ms, "ms_again": _events_ms(lambda i: dst.copy_(src[i % 3])), "bytes": 2 * nbytes}
    out["copy1"] = {"ms": copy1_ms, "ms_again": _events_ms(lambda i: dst[:nbytes // BATCH].copy_(one[i % 3])),
                    "bytes": 2 * nbytes // BATCH}
    print("RESULT " + json.dumps(out))


def measure_callback(baseline):
    """baseline: only the callback without the argument, with nothing of this stage imported (a parent checkout)"""
    import torch
    from unet_lane_detection_amd import follow as F, ros_bridge as RB, state as S
    from unet_lane_detection_amd.model import UNetHIP

    model = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    img = _scene(1, 11)[0]
    msg = RB.ImageMsg(height=H, width=W, encoding="bgr8", data=img.tobytes())
    pipes = {"hsv_plain": F.LaneFollowPipeline(None, source="hsv"),
             "unet_plain": F.LaneFollowPipeline(model, source="unet", precision="f16x3")}
    if not baseline:
        from unet_lane_detection_amd import correct as K
        every = K.CorrectConfig(stretch=(1.0, 1.0), gamma=0.8, clahe=K.Clahe())
        pipes.update({"hsv_none": F.LaneFollowPipeline(None, source="hsv", correct=None),
                      "hsv_wb": F.LaneFollowPipeline(None, source="hsv", correct=K.CorrectConfig()),
                      "hsv_all": F.LaneFollowPipeline(None, source="hsv", correct=every),
                      "unet_none": F.LaneFollowPipeline(model, source="unet", precision="f16x3", correct=None),
                      "unet_wb": F.LaneFollowPipeline(model, source="unet", precision="f16x3", correct=K.CorrectConfig()),
                      "unet_all": F.LaneFollowPipeline(model, source="unet", precision="f16x3", correct=every)})
        del pipes["hsv_plain"], pipes["unet_plain"]

    def wall(fn):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(CALLBACKS):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts
    res = {k: [] for k in pipes}
    for _ in range(2):   # alternating rounds, so that a drifting host shows in all
        for key, pipe in pipes.items():
            res[key] += wall(lambda: pipe.process(msg))
    assert model.device_error() == 0
    torch.cuda.synchronize()
    model.release()
    print("RESULT " + json.dumps(res))


def measure_effect():
    import numpy as np
    import torch
    from unet_lane_detection_amd import correct as K, follow as F

    frames, targets = _tracks(16)
    cast = frames.copy()
    cast[..., 0] = np.floor(frames[..., 0] * 0.7 + 0.5).astype(np.uint8)
    fc = K.FrameCorrector(K.CorrectConfig())
    fixed = fc.correct(torch.from_numpy(cast).cuda()).cpu().numpy()
    plan = fc.plan()
    ex = F.HSVLaneExtractor()
    out = {}
    for key, f in (("as painted", frames), ("blue * 0.7", cast), ("blue * 0.7, gray-world correction", fixed)):
        out[key] = ex.evaluate(f, targets, batch=8).at(0.5)
    out["gains"] = [float(g) for g in plan.gains.mean(axis=0)]
    print("RESULT " + json.dumps(out))


def _child(step, root):
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", step, "--root", root]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        print(p.stdout[-4000:])
        print("step %s ended with status %d" % (step, p.returncode))
        return None, p.returncode or 1
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]), 0


def _md(call, cb, parent, effect, cmdline):
    med = statistics.median
    copy = med(call["copy"]["ms"] + call["copy"]["ms_again"])
    copy1 = med(call["copy1"]["ms"] + call["copy1"]["ms_again"])
    px = H * W
    lines = ["# Frame correction on the device: the call, one callback, the effect on the HSV baseline", "",
             "Produced by `%s` on one MI355X, every part in a process of its own." % cmdline, "",
             "## (a) `unet_correct_u8_batch`, frames of %d x %d" % (H, W), "",
             "A sample is %d back-to-back calls between two HIP events, divided by %d; median of %d samples after %d"
             % (LAUNCHES, LAUNCHES, ITERS, WARMUP),
             "warm-ups; the input rotates over three buffers.  A call is four launches without CLAHE and six with it.",
             "The yardstick is `Tensor.copy_` of the same frames' bytes, device to device, measured the same way before",
             "and after in the same process: %.4f ms for 64 frames (%.0f GB/s read + written), %.4f ms for one frame."
             % (copy, call["copy"]["bytes"] / copy / 1e6, copy1), "",
             "| stages | frames | ms a call | min .. max | us a frame | the call's time over the copy's |", "|---|---|---|---|---|---|"]
    for e in call["call"]:
        d = med(e["ms"])
        lines.append("| %s | %d | %.4f | %.4f .. %.4f | %.2f | %.2f |" % (
            e["what"], e["n"], d, min(e["ms"]), max(e["ms"]), d * 1e3 / e["n"], d / (copy if e["n"] == BATCH else copy1)))
    full = med([e for e in call["call"] if e["what"] == "all four" and e["n"] == BATCH][0]["ms"])
    lines += ["", "All four stages on 64 frames: %.1f ps a pixel." % (full * 1e9 / (BATCH * px)), "",
              "## (b) One callback: a %d x %d bgr8 message in, the lane centres out" % (H, W), "",
              "Wall clock on the host, warp to 1055 x 685; %d callbacks each in two alternating rounds after 5 warm-ups."
              % CALLBACKS, "", "| path | ms a callback, median | min .. max |", "|---|---|---|"]
    labels = (("hsv", "source \"hsv\""), ("unet", "source \"unet\" (model A, f16x3)"))
    for key, name in labels:
        for suffix, what in (("none", "correct=None"), ("wb", "gray world"), ("all", "all four stages")):
            r = cb[key + "_" + suffix]
            lines.append("| %s, %s | %.3f | %.3f .. %.3f |" % (name, what, med(r), min(r), max(r)))
        if parent:
            r = parent[key + "_plain"]
            lines.append("| %s, the parent commit's checkout, no argument | %.3f | %.3f .. %.3f |" % (name, med(r), min(r), max(r)))
    lines.append("")
    for key, name in labels:
        text = "%s: gray world %+.3f ms, all four %+.3f ms over correct=None" % (
            name, med(cb[key + "_wb"]) - med(cb[key + "_none"]), med(cb[key + "_all"]) - med(cb[key + "_none"]))
        if parent:
            text += "; correct=None against the parent commit %+.3f ms" % (med(cb[key + "_none"]) - med(parent[key + "_plain"]))
        lines.append(text + ".")
    if not parent:
        lines.append("The parent commit was not measured in this run (no --parent).")
    lines += ["", "## (c) The HSV baseline under a blue-deficient cast", "",
              "`HSVLaneExtractor.evaluate` on 16 synthetic tracks of %d x %d (gray surface 100 +- 6, two white markings" % (H, W),
              "240 +- 6), against the painted markings.  Mean gains of the correction (B, G, R): %s." %
              ", ".join("%.3f" % g for g in effect["gains"]), "",
              "| frames | IoU | precision | recall | tp | fp | fn |", "|---|---|---|---|---|---|---|"]
    for key, m in effect.items():
        if key != "gains":
            lines.append("| %s | %.4f | %.4f | %.4f | %d | %d | %d |" % (key, m["iou"], m["precision"], m["recall"],
                                                                       m["tp"], m["fp"], m["fn"]))
    lines += ["", "## Raw lines", "", "```"]
    for e in call["call"]:
        lines.append("%s, %d: %s" % (e["what"], e["n"], " ".join("%.4f" % x for x in e["ms"])))
    for k in ("copy", "copy1"):
        for kk in ("ms", "ms_again"):
            lines.append("%s %s: %s" % (k, kk, " ".join("%.4f" % x for x in call[k][kk])))
    for k, v in list(cb.items()) + [("parent " + k, v) for k, v in (parent or {}).items()]:
        lines.append("callback %s: %s" % (k, " ".join("%.3f" % x for x in v)))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--root", default=HERE_ROOT, help="the checkout the package is imported from")
    ap.add_argument("--parent", default="", help="a checkout of the parent commit, its library built")
    ap.add_argument("--out", default="correct.md")
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, os.path.abspath(args.root))
        {"call": measure_call, "callback": lambda: measure_callback(False), "baseline": lambda: measure_callback(True),
         "effect": measure_effect}[args.step]()
        return 0
    results = []
    steps = [("call", HERE_ROOT), ("callback", HERE_ROOT)] + ([("baseline", args.parent)] if args.parent else []) + \
        [("effect", HERE_ROOT)]
    for step, root in steps:   # a step that fails ends the run: nothing more is started on the device
        r, rc = _child(step, root)
        if rc:
            return rc
        results.append(r)
    call, cb = results[0], results[1]
    parent = results[2] if args.parent else None
    cmdline = "python tools/correct_timing.py --out %s" % args.out + (" --parent <parent checkout>" if args.parent else "")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(_md(call, cb, parent, results[-1], cmdline))
    print("written " + args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
