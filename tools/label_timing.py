#!/usr/bin/env python3
"""Cost of the component labelling on the device (unet_lane_detection_amd/instances.py): the two calls, one frame on
its own, and one callback of `LaneFollowPipeline` with the clean-up on and off.

  python tools/label_timing.py --out profiles/r24/label.md

One measurement in a fresh child process under its own time limit.  Three parts:
  (a) calls     unet_label_u8_batch (8-connected, cap 1024) and unet_keep_components_u8_batch (min_area 64) on 1 and on
                64 resident masks of 685 x 1055 and of 224 x 224, painted lanes with 1 % speckle and random masks of
                density 0.5: a sample is LAUNCHES back-to-back calls between two HIP events, divided by LAUNCHES; median
                of ITERS samples after WARMUP, the input rotating over three buffers.  Beside each, measured the same way
                in the same run, `Tensor.copy_` of the same n * h * w bytes, device to device, and
                unet_lane_fit_u8_batch on the same masks.
  (b) one frame the n = 1 calls again, one call per sample (what a caller who waits for every frame sees).
  (c) callback  `LaneFollowPipeline.process` (model A, f16x3) with clean=CleanConfig() and with clean=None, against the
                host route to the same mask: `process(return_mask=True)` - the 722 KB mask comes to the host - then
                scipy.ndimage.label and numpy (tests/label_model.py where scipy is not importable; the output says
                which).  Wall clock of one callback, median of CALLBACKS after 5 warm-ups, alternating rounds.

`--step phases-painted` (or `phases-random`) only issues the calls on one 685 x 1055 mask, for a kernel trace in a run
of its own, and `--trace` turns the two traces' databases into the table of kernels:
  rocprofv3 --kernel-trace --stats -d P -o t -- python tools/label_timing.py --step phases-painted
  rocprofv3 --kernel-trace --stats -d R -o t -- python tools/label_timing.py --step phases-random
  python tools/label_timing.py --trace P/t_results.db R/t_results.db --out profiles/r24/label_phases.md
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((685, 1055), (224, 224))
BATCHES = (1, 64)
WARMUP, ITERS, LAUNCHES, CALLBACKS = 3, 20, 10, 30
LIMIT = 420
CAP, MIN_AREA = 1024, 64


def _events_ms(fn, launches=LAUNCHES):
    """fn(i) enqueues call i; -> ITERS samples of milliseconds per call"""
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


class Calls:
    """the two entry points on preallocated buffers: no allocation in the timed loop"""

    def __init__(self, lib, n, h, w):
        import torch
        self.lib, self.shape = lib, (n, h, w)
        self.labels = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
        self.header = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        self.records = torch.empty((n, CAP, 16), dtype=torch.int64, device="cuda")
        self.work = torch.empty((lib.unet_label_work_bytes(n, h, w),), dtype=torch.uint8, device="cuda")
        self.keep = torch.empty((n, CAP), dtype=torch.uint8, device="cuda")
        self.out = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        self.fit = torch.empty((n, 2, 16), dtype=torch.int64, device="cuda")

    def label(self, masks):
        from unet_lane_detection_amd import _lib
        n, h, w = self.shape
        _lib.call("unet_label_u8_batch", masks.device, masks, n, h, w, 127, 8, self.labels, CAP, self.header, self.records,
                  self.work, self.work.numel())

    def keep_components(self):
        from unet_lane_detection_amd import _lib
        n, h, w = self.shape
        _lib.call("unet_keep_components_u8_batch", self.labels.device, self.labels, n, h, w, self.header, self.records, CAP,
                  MIN_AREA, 0, 0, 0, self.keep, self.out)

    def lane_fit(self, masks):
        from unet_lane_detection_amd import _lib
        n, h, w = self.shape
        _lib.call("unet_lane_fit_u8_batch", masks.device, masks, n, h, w, 127, 9, 100, 50, None, self.fit)


def _inputs(kind, n, h, w):
    """three (n, h, w) uint8 device tensors: painted lanes with 1 % speckle, or random at density 0.5"""
    import numpy as np
    import torch

    import label_model as M
    rng = np.random.default_rng(24 + n + h)
    out = []
    for r in range(3):
        if kind == "painted":
            base = [np.where(M._three_lanes(rng, h, w, 0.01), 255, 0).astype(np.uint8) for _ in range(min(n, 4))]
            frames = np.stack([np.roll(base[i % len(base)], 3 * (i // len(base)) + r, axis=1) for i in range(n)])
        else:
            frames = np.where(rng.random((n, h, w)) < 0.5, 255, 0).astype(np.uint8)
        out.append(torch.from_numpy(frames).cuda())
    return out


def measure():
    import numpy as np
    import torch

    import label_model as M
    from unet_lane_detection_amd import _lib, follow as F, instances as I, ros_bridge as RB, state as S
    from unet_lane_detection_amd.model import UNetHIP

    lib = _lib.load()
    out = {"calls": [], "single": [], "callback": {}}
    for h, w in SIZES:
        for kind in ("painted", "random"):
            for n in BATCHES:
                inputs = _inputs(kind, n, h, w)
                calls = Calls(lib, n, h, w)
                if n == 1:     # what is timed is what the tests check: the model's bytes
                    ref = M.label(inputs[0].cpu().numpy(), 127, 8, CAP)
                    calls.label(inputs[0])
                    calls.keep_components()
                    torch.cuda.synchronize()
                    assert np.array_equal(calls.labels.cpu().numpy(), ref[0])
                    assert np.array_equal(calls.records.cpu().numpy().view(np.uint64), ref[2])
                    assert np.array_equal(calls.out.cpu().numpy(), M.keep(*ref, CAP, min_area=MIN_AREA)[1])
                src = [torch.randint(0, 256, (n * h * w,), dtype=torch.uint8, device="cuda") for _ in range(3)]
                dst = torch.empty(n * h * w, dtype=torch.uint8, device="cuda")
                e = {"h": h, "w": w, "n": n, "kind": kind, "bytes": n * h * w}
                e["copy"] = _events_ms(lambda i: dst.copy_(src[i % 3]))
                e["label"] = _events_ms(lambda i: calls.label(inputs[i % 3]))
                e["keep"] = _events_ms(lambda i: calls.keep_components())
                e["lane_fit"] = _events_ms(lambda i: calls.lane_fit(inputs[i % 3]))
                e["copy_again"] = _events_ms(lambda i: dst.copy_(src[i % 3]))
                head = calls.header.cpu().numpy()
                e["components"] = float(head[:, 0].mean())
                e["on_share"] = float(head[:, 1].sum()) / (n * h * w)
                out["calls"].append(e)
                if n == 1:
                    out["single"].append({"h": h, "w": w, "kind": kind,
                                          "label": _events_ms(lambda i: calls.label(inputs[i % 3]), launches=1),
                                          "keep": _events_ms(lambda i: calls.keep_components(), launches=1),
                                          "lane_fit": _events_ms(lambda i: calls.lane_fit(inputs[i % 3]), launches=1),
                                          "copy": _events_ms(lambda i: dst.copy_(src[i % 3]), launches=1)})
                del inputs, calls, src, dst

    # (c) one callback
    try:
        from scipy import ndimage
        host_name = "scipy.ndimage.label + numpy"
    except ImportError:
        ndimage = None
        host_name = "tests/label_model.py (numpy, Python loops over runs)"
    model = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 256, (480, 640, 3), dtype=torch.uint8, generator=g).numpy()
    img[:, 150:170] = 240
    img[:, 470:490] = 240
    msg = RB.ImageMsg(height=480, width=640, encoding="bgr8", data=img.tobytes())
    cfg = I.CleanConfig(min_area=MIN_AREA)
    plain = F.LaneFollowPipeline(model, source="unet", precision="f16x3")
    cleaned = F.LaneFollowPipeline(model, source="unet", precision="f16x3", clean=cfg)

    def host():
        centres, m = plain.process(msg, return_mask=True)
        mask = np.frombuffer(m.data, dtype=np.uint8).reshape(m.height, m.width)
        if ndimage is not None:
            lab, k = ndimage.label(mask > cfg.level, structure=np.ones((3, 3), dtype=bool))
            area = np.bincount(lab.ravel(), minlength=k + 1)
            keep = area >= cfg.min_area
            keep[0] = False
            keep[cfg.max_components + 1:] = False
            return np.where(keep[lab], 255, 0).astype(np.uint8)
        ref = M.label(mask[None], cfg.level, cfg.connectivity, cfg.max_components)
        return M.keep(*ref, cfg.max_components, min_area=cfg.min_area)[1][0]

    def device():
        centres, m = cleaned.process(msg, return_mask=True)
        return np.frombuffer(m.data, dtype=np.uint8).reshape(m.height, m.width)

    def wall(fn):
        for _ in range(5):
            got = fn()
        ts = []
        for _ in range(CALLBACKS):
            t0 = time.perf_counter()
            got = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts, got
    res = {"host": [], "clean": [], "clean_centres": [], "plain": []}
    got = {}
    for _ in range(2):     # alternating rounds, so that a drifting host shows in all of them
        for key, fn in (("host", host), ("clean", device), ("clean_centres", lambda: cleaned.process(msg)),
                        ("plain", lambda: plain.process(msg))):
            ts, got[key] = wall(fn)
            res[key] += ts
    assert np.array_equal(got["host"], got["clean"])          # both routes end in the same mask
    res["host_name"] = host_name
    res["components"] = cleaned.last_components.count[0]
    res["kept"] = int((got["clean"] > 0).sum())
    assert model.device_error() == 0
    out["callback"] = res
    model.release()
    print("RESULT " + json.dumps(out))


def phases(kind):
    import torch

    from unet_lane_detection_amd import _lib
    lib = _lib.load()
    h, w = SIZES[0]
    inputs = _inputs(kind, 1, h, w)
    calls = Calls(lib, 1, h, w)
    for i in range(40):
        calls.label(inputs[i % 3])
        calls.keep_components()
    torch.cuda.synchronize()
    print("phases: 40 calls of each entry point issued on one %s mask" % kind)


def trace_table(painted_db, random_db, out_path):
    """the `kernels` view of two rocprofv3 databases -> a table of this feature's kernels, microseconds"""
    import sqlite3
    cols = []
    for path in (painted_db, random_db):
        db = sqlite3.connect(path)
        rows = db.execute("select name, count(*), avg(end - start) / 1e3, min(end - start) / 1e3, max(end - start) / 1e3 "
                          "from kernels where name like '%LabelArgs%' or name like '%KeepArgs%' group by name").fetchall()
        cols.append({re.search(r"(\w+_kernel)\(", r[0]).group(1): r[1:] for r in rows})
    names = sorted(cols[0], key=lambda k: -cols[0][k][1])
    lines = ["# Component labelling: the kernels of one 685 x 1055 mask", "",
             "Produced by `python tools/label_timing.py --trace ... --out %s` from two `rocprofv3 --kernel-trace` runs of" % out_path,
             "`--step phases-painted` and `--step phases-random`: %d calls of each entry point on one resident mask, runs of"
             % cols[0][names[0]][0],
             "their own.  Kernel durations from the trace, microseconds.", "",
             "| kernel | painted: mean | min .. max | random 0.5: mean | min .. max |", "|---|---|---|---|---|"]
    for k in names:
        a, b = cols[0][k], cols[1].get(k, (0, 0.0, 0.0, 0.0))
        lines.append("| `%s` | %.1f | %.1f .. %.1f | %.1f | %.1f .. %.1f |" % (k, a[1], a[2], a[3], b[1], b[2], b[3]))
    lines += ["| sum of the means | %.1f | | %.1f | |" % (sum(v[1] for v in cols[0].values()), sum(v[1] for v in cols[1].values())), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines))
    print("written " + out_path)


def _md(m, out_path):
    med = statistics.median
    lines = ["# Component labelling on the device: the calls, one frame on its own, one callback", "",
             "Produced by `python tools/label_timing.py --out %s` on one MI355X, one process." % out_path, "",
             "## (a) `unet_label_u8_batch` (8-connected, cap %d) and `unet_keep_components_u8_batch` (min_area %d)" % (CAP, MIN_AREA), "",
             "A sample is %d back-to-back calls between two HIP events, divided by %d; median of %d samples after %d"
             % (LAUNCHES, LAUNCHES, ITERS, WARMUP),
             "warm-ups; the input rotates over three buffers.  \"painted\" is three curved markings with 1 % speckle, \"random\"",
             "is density 0.5.  GB/s is over the n h w mask bytes (the label call also writes 4 n h w bytes of labels and reads",
             "and rewrites them in its later phases).  The yardstick is `Tensor.copy_` of the same n h w bytes, device to device,",
             "measured the same way before and after; `unet_lane_fit_u8_batch` (window mode) runs on the same masks.", "",
             "| masks | what | ms a call | min .. max | GB/s | time / copy's time |", "|---|---|---|---|---|---|"]
    for e in m["calls"]:
        copy_ms = med(e["copy"] + e["copy_again"])
        head = "%d of %d x %d, %s" % (e["n"], e["h"], e["w"], e["kind"])
        for label, key in (("copy, before", "copy"), ("label", "label"), ("keep", "keep"), ("lane fit", "lane_fit"),
                           ("copy, after", "copy_again")):
            d = med(e[key])
            ratio = "" if key.startswith("copy") else "%.1f" % (d / copy_ms)
            lines.append("| %s | %s | %.4f | %.4f .. %.4f | %.1f | %s |" % (head, label, d, min(e[key]), max(e[key]),
                                                                          e["bytes"] / d / 1e6, ratio))
    lines += ["", "Components a frame (mean) and share of ON pixels: " + "; ".join(
        "%d of %d x %d %s: %.0f, %.3f" % (e["n"], e["h"], e["w"], e["kind"], e["components"], e["on_share"]) for e in m["calls"]) + ".",
        "", "## (b) One frame on its own", "",
        "n = 1, one call per sample (two events around a single call); the copy of the same bytes the same way.", "",
        "| mask | what | ms | min .. max |", "|---|---|---|---|"]
    for e in m["single"]:
        for label, key in (("label", "label"), ("keep", "keep"), ("lane fit", "lane_fit"), ("copy", "copy")):
            lines.append("| %d x %d, %s | %s | %.4f | %.4f .. %.4f |" % (e["h"], e["w"], e["kind"], label, med(e[key]),
                                                                       min(e[key]), max(e[key])))
    r = m["callback"]
    lines += ["", "## (c) One callback: a 480 x 640 bgr8 message in, the cleaned 685 x 1055 mask out", "",
              "Wall clock on the host, model A on the f16x3 tier at 224 x 224, warp to 1055 x 685; %d callbacks each in two" % CALLBACKS,
              "alternating rounds after 5 warm-ups.  The host route is `LaneFollowPipeline.process(return_mask=True)` - the 722 KB",
              "mask comes to the host - followed by %s with the same rule (min_area %d, cap %d)." % (r["host_name"], MIN_AREA, CAP),
              "Both routes ended in the same mask: %d components in the frame, %d pixels kept." % (r["components"], r["kept"]), "",
              "| path | ms a callback, median | min .. max |", "|---|---|---|"]
    for label, key in (("host route: process(return_mask=True) + %s" % r["host_name"], "host"),
                       ("LaneFollowPipeline(clean=CleanConfig()), return_mask=True", "clean"),
                       ("LaneFollowPipeline(clean=CleanConfig()): centres only", "clean_centres"),
                       ("LaneFollowPipeline(clean=None): centres only", "plain")):
        lines.append("| %s | %.3f | %.3f .. %.3f |" % (label, med(r[key]), min(r[key]), max(r[key])))
    lines += ["", "The clean-up adds %.3f ms to a callback (median with it minus median without, centres only)."
              % (med(r["clean_centres"]) - med(r["plain"])), "", "## Raw lines", "", "```"]
    for e in m["calls"] + m["single"]:
        head = " ".join("%s=%s" % (k, v) for k, v in e.items() if not isinstance(v, list))
        for k, v in e.items():
            if isinstance(v, list):
                lines.append("%s %s: %s" % (head, k, " ".join("%.4f" % x for x in v)))
    for key in ("host", "clean", "clean_centres", "plain"):
        lines.append("callback %s: %s" % (key, " ".join("%.3f" % x for x in r[key])))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="label.md")
    ap.add_argument("--trace", nargs=2, metavar=("PAINTED_DB", "RANDOM_DB"), default=None)
    args = ap.parse_args()
    if args.trace:
        trace_table(args.trace[0], args.trace[1], args.out)
        return 0
    if args.step.startswith("phases-"):
        phases(args.step[7:])
        return 0
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
