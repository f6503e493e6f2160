#!/usr/bin/env python3
"""Cost of the lane fit on the device (unet_lane_detection_amd/lanefit.py): the kernel, one frame on its own, and one
callback of `LaneFollowPipeline` with the fit on and off.

  python tools/lane_fit_timing.py --out profiles/r23/lane_fit.md

One measurement in a fresh child process under its own time limit.  Three parts:
  (a) kernel    unet_lane_fit_u8_batch on 1 and on 64 resident masks of 685 x 1055 and of 480 x 640, window mode and
                prior mode (the table made from the same masks' fits): a sample is LAUNCHES back-to-back launches
                between two HIP events, divided by LAUNCHES; median of ITERS samples after WARMUP, the input rotating
                over three buffers.  Beside each, measured the same way in the same run, `Tensor.copy_` of the same
                n * h * w bytes, device to device (it reads them once and writes them once).
  (b) one frame the n = 1 launch again, one launch per sample (what a caller who waits for every frame sees), since one
                workgroup serves a frame and 255 of 256 CUs idle.
  (c) callback  `LaneFollowPipeline.process` (model A, f16x3) with fit=FitConfig() and with fit=None, against the path
                there was before for the same answer: `process(return_mask=True)` - the 722 KB mask comes to the host -
                plus the numpy model of the fit (tests/lanefit_model.py) on it.  Wall clock of one callback, message
                bytes in to coefficients out, median of CALLBACKS after 5 warm-ups, alternating rounds.
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

SIZES = ((685, 1055), (480, 640))
BATCHES = (1, 64)
WARMUP, ITERS, LAUNCHES, CALLBACKS = 3, 20, 10, 30
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

    import lanefit_model as LM
    from unet_lane_detection_amd import _lib, follow as F, lanefit as LF, ros_bridge as RB, state as S
    from unet_lane_detection_amd.model import UNetHIP

    lib = _lib.load()
    cfg = LF.FitConfig()

    ptr = _lib.ptr

    def launch(masks, prior, out):     # the entry point itself on preallocated buffers: no allocation in the timed loop
        n, h, w = masks.shape
        rc = lib.unet_lane_fit_u8_batch(0, ptr(masks), n, h, w, cfg.level, cfg.n_windows, cfg.margin, cfg.min_pixels,
                                        ptr(prior), ptr(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "unet_lane_fit_u8_batch")

    out = {"kernel": [], "single": [], "callback": {}}
    for h, w in SIZES:
        painted = torch.from_numpy(LM.painted_lanes(11, 9, h, w)[:8]).cuda()      # 8 frames with both markings
        assert np.array_equal(LF.lane_fit_records(painted[:2], cfg).cpu().numpy().view(np.uint64),
                              LM.records(painted[:2].cpu().numpy(), cfg.level, cfg.n_windows, cfg.margin, cfg.min_pixels))
        for n in BATCHES:
            inputs = [torch.roll(painted[(torch.arange(n) + r) % 8], shifts=3 * r, dims=2).contiguous() for r in range(3)]
            fits = [LF.lane_fits(m, cfg) for m in inputs]
            tables = [torch.from_numpy(LF.prior_table(f, h)).cuda() for f in fits]
            found = float(np.mean([lane.coeffs is not None for f in fits for frame in f for lane in frame.lanes]))
            rec = torch.empty((n, 2, 16), dtype=torch.int64, device="cuda")
            src = [torch.randint(0, 256, (n * h * w,), dtype=torch.uint8, device="cuda") for _ in range(3)]
            dst = torch.empty(n * h * w, dtype=torch.uint8, device="cuda")
            copy_ms = _events_ms(lambda i: dst.copy_(src[i % 3]))
            window_ms = _events_ms(lambda i: launch(inputs[i % 3], None, rec))
            prior_ms = _events_ms(lambda i: launch(inputs[i % 3], tables[i % 3], rec))
            copy_again = _events_ms(lambda i: dst.copy_(src[i % 3]))      # the yardstick's own spread: before and after
            share = float((inputs[0] > cfg.level).float().mean())
            out["kernel"].append({"h": h, "w": w, "n": n, "bytes": n * h * w, "window": window_ms, "prior": prior_ms,
                                  "copy": copy_ms, "copy_again": copy_again, "on_share": share, "lanes_found": found})
            if n == 1:
                out["single"].append({"h": h, "w": w,
                                      "window": _events_ms(lambda i: launch(inputs[i % 3], None, rec), launches=1),
                                      "prior": _events_ms(lambda i: launch(inputs[i % 3], tables[i % 3], rec), launches=1),
                                      "copy": _events_ms(lambda i: dst.copy_(src[i % 3]), launches=1)})
            del inputs, tables, src, dst

    # (c) one callback
    model = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 256, (480, 640, 3), dtype=torch.uint8, generator=g).numpy()
    img[:, 150:170] = 240
    img[:, 470:490] = 240
    msg = RB.ImageMsg(height=480, width=640, encoding="bgr8", data=img.tobytes())
    plain = F.LaneFollowPipeline(model, source="unet", precision="f16x3")
    fitted = F.LaneFollowPipeline(model, source="unet", precision="f16x3", fit=cfg)
    host_tracker = LM.Tracker(cfg.level, cfg.n_windows, cfg.margin, cfg.min_pixels)

    def parent():
        centres, m = plain.process(msg, return_mask=True)
        mask = np.frombuffer(m.data, dtype=np.uint8).reshape(m.height, m.width)
        mode, rec = host_tracker.update(mask)
        return [LM.coeffs_of(wd) for wd in rec[0]], rec

    def device():
        centres, fits = fitted.process(msg)
        return [lane.coeffs for lane in fits[0].lanes], fits.words

    def wall(fn):
        for _ in range(5):
            got = fn()
        ts = []
        for _ in range(CALLBACKS):
            t0 = time.perf_counter()
            got = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts, got
    res = {"parent": [], "fit": [], "plain": []}
    for _ in range(2):     # alternating rounds, so that a drifting host shows in all three
        for key, fn in (("parent", parent), ("fit", device), ("plain", lambda: (plain.process(msg), None))):
            ts, got = wall(fn)
            res[key] += ts
            res[key + "_got"] = got
    # both paths fit the same mask with the same tracker logic: the same records at every step
    assert np.array_equal(res["parent_got"][1], res["fit_got"][1])
    assert res["parent_got"][0] == res["fit_got"][0]
    res["coeffs"] = [list(c) if c is not None else None for c in res["fit_got"][0]]
    res["modes"] = sorted(set(fitted.tracker.modes))
    for key in ("parent_got", "fit_got", "plain_got"):
        del res[key]
    assert model.device_error() == 0
    out["callback"] = res
    model.release()
    print("RESULT " + json.dumps(out))


def _md(m, out_path):
    med = statistics.median
    lines = ["# Lane fit on the device: the kernel, one frame on its own, one callback", "",
             "Produced by `python tools/lane_fit_timing.py --out %s` on one MI355X, one process." % out_path, "",
             "## (a) `unet_lane_fit_u8_batch`: 9 windows, margin 100, min_pixels 50, level 127", "",
             "A sample is %d back-to-back launches between two HIP events, divided by %d; median of %d samples after %d"
             % (LAUNCHES, LAUNCHES, ITERS, WARMUP),
             "warm-ups; the input rotates over three buffers of painted masks (two curved markings, one dashed, 1 - 3 % noise).",
             "GB/s is over the n h w mask bytes.  The yardstick is `Tensor.copy_` of the same n h w bytes, device to device",
             "(read once, written once), measured the same way before and after the kernel's rows.  One workgroup serves a",
             "frame: a launch of n masks occupies n of the 256 CUs.", "",
             "| masks | what | ms a launch | min .. max | GB/s | time / copy's time |", "|---|---|---|---|---|---|"]
    for e in m["kernel"]:
        copy_ms = med(e["copy"] + e["copy_again"])
        head = "%d of %d x %d" % (e["n"], e["h"], e["w"])
        for label, key in (("copy, before", "copy"), ("window mode", "window"), ("prior mode", "prior"), ("copy, after", "copy_again")):
            d = med(e[key])
            ratio = "" if key.startswith("copy") else "%.2f" % (d / copy_ms)
            lines.append("| %s | %s | %.4f | %.4f .. %.4f | %.1f | %s |" % (head, label, d, min(e[key]), max(e[key]),
                                                                          e["bytes"] / d / 1e6, ratio))
    lines += ["", "Share of ON pixels in the masks: %s; lanes with coefficients: %s." % (
        ", ".join("%.3f" % e["on_share"] for e in m["kernel"]), ", ".join("%.2f" % e["lanes_found"] for e in m["kernel"])),
        "", "## (b) One frame on its own", "",
        "n = 1, one launch per sample (two events around a single launch, so the figure includes what a lone launch costs",
        "between events); the copy of the same bytes the same way.", "",
        "| mask | what | ms | min .. max |", "|---|---|---|---|"]
    for e in m["single"]:
        for label, key in (("window mode", "window"), ("prior mode", "prior"), ("copy", "copy")):
            lines.append("| %d x %d | %s | %.4f | %.4f .. %.4f |" % (e["h"], e["w"], label, med(e[key]), min(e[key]), max(e[key])))
    r = m["callback"]
    lines += ["", "## (c) One callback: a 480 x 640 bgr8 message in, both lanes' coefficients out", "",
              "Wall clock on the host, model A on the f16x3 tier at 224 x 224, warp to 1055 x 685; %d callbacks each in two"
              % CALLBACKS,
              "alternating rounds after 5 warm-ups.  \"before\" is `LaneFollowPipeline.process(return_mask=True)` - the 722 KB",
              "mask comes to the host - followed by the numpy model of the fit (tests/lanefit_model.py: loops over rows,",
              "Python integers, Fractions) with the same tracker logic; it is the only host implementation there is, not a tuned one.", "",
              "| path | ms a callback, median | min .. max |", "|---|---|---|"]
    for label, key in (("before: process(return_mask=True) + the fit on the host", "parent"),
                       ("LaneFollowPipeline(fit=FitConfig())", "fit"), ("LaneFollowPipeline(fit=None): centres only", "plain")):
        lines.append("| %s | %.3f | %.3f .. %.3f |" % (label, med(r[key]), min(r[key]), max(r[key])))
    lines += ["", "The fit adds %.3f ms to a callback (median with it minus median without)." % (med(r["fit"]) - med(r["plain"])),
              "Both paths returned the same records and coefficients: %s; modes that ran: %s." % (r["coeffs"], ", ".join(r["modes"])),
              "", "## Raw lines", "", "```"]
    for e in m["kernel"] + m["single"]:
        head = " ".join("%s=%s" % (k, v) for k, v in e.items() if not isinstance(v, list))
        for k, v in e.items():
            if isinstance(v, list):
                lines.append("%s %s: %s" % (head, k, " ".join("%.4f" % x for x in v)))
    for key in ("parent", "fit", "plain"):
        lines.append("callback %s: %s" % (key, " ".join("%.3f" % x for x in r[key])))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="lane_fit.md")
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
