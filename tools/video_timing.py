#!/usr/bin/env python3
"""Cost of the video path (unet_lane_detection_amd/video.py) per chunk of 64 frames of 480 x 640, on two tiers: int8
with model B and f16x3 with model A, network input 224 x 224.

  python tools/video_timing.py --out profiles/r19/video_pipeline.md

One measurement in a fresh child process under its own time limit.  Three parts:
  (a) kernels    HIP events around unet_resize_u8_batch and unet_overlay_u8_batch (with the full-size mask) on a resident
                 chunk, median of ITERS launches after WARMUP, and the bytes per second that implies from the bytes the
                 algorithm has to move;
  (b) pipeline   host-to-host frames/s of `FramePipeline.run` over CHUNKS chunks (wall clock from the first host array in
                 to the last host array out, median of ROUNDS), and the chunk's split into upload, resize, network,
                 overlay and download, each alone between HIP events;
  (c) parent     the same frames through what there was before the video path, a frame at a time: upload, CameraStage.resize,
                 run_u8, CameraStage.resize of the mask, download, colour table and blend in numpy.
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

CHUNK, HEIGHT, WIDTH, INPUT = 64, 480, 640, 224
WARMUP, ITERS, CHUNKS, ROUNDS, PARENT_FRAMES = 3, 20, 8, 3, 64
LIMIT = 480
FEATS_B = [32, 64, 128]


def kernel_bytes():
    """What one chunk has to move.  overlay: every frame byte read and every overlay byte written once, plus the
    full-size mask (the small masks stay in L2).  resize: every frame byte read once, the network's input written."""
    px = CHUNK * HEIGHT * WIDTH
    return {"overlay": px * 3 + px * 3 + px, "resize": px * 3 + CHUNK * INPUT * INPUT * 3}


def _events_ms(fn, warmup, iters):
    import torch
    ts = []
    for it in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ts.append(a.elapsed_time(b))
    return ts


def _blend_numpy(frame, mask, lut, alpha, beta, gamma):
    """applyColorMap + addWeighted of one frame on the host, in fp32 (tests/video_model.py states the same)"""
    import numpy as np
    f32 = np.float32
    v = frame.astype(f32) * f32(alpha) + lut[mask].astype(f32) * f32(beta) + f32(gamma)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def measure():
    import numpy as np
    import torch
    from unet_lane_detection_amd import quant, state as S, video as V
    from unet_lane_detection_amd.int8 import UNetInt8, calibrate
    from unet_lane_detection_amd.model import UNetHIP
    from unet_lane_detection_amd.ros_bridge import CameraStage

    frames = S.synthetic_frames(CHUNK, HEIGHT, WIDTH, seed=7)
    sdb = S.seeded_state_dict(FEATS_B, seed=0)
    fmb = UNetHIP(sdb, device=0)
    ranges = calibrate(fmb, torch.from_numpy(S.synthetic_frames(4, INPUT, INPUT, seed=1)), batch=4)
    fmb.release()
    tiers = (("int8, model B", UNetInt8(quant.quantize_model(sdb, ranges), device=0), {}),
             ("f16x3, model A", UNetHIP(S.seeded_state_dict(seed=0), device=0), {"precision": "f16x3"}))
    out = {"bytes": kernel_bytes(), "tiers": {}}
    stage = CameraStage(0)
    dev = torch.from_numpy(frames).cuda()
    pin_in = torch.from_numpy(frames).pin_memory()
    for name, model, kw in tiers:
        pipe = V.FramePipeline(model, input_size=(INPUT, INPUT), **kw)
        res = {}
        # (a) + the split of (b): every stage alone on a resident chunk
        small = pipe._resize(dev)
        mask_small = pipe._network(small)
        overlay = torch.empty_like(dev)
        mask = torch.empty(dev.shape[:3], dtype=torch.uint8, device="cuda")
        both = torch.empty(dev.numel() // 3 * 4, dtype=torch.uint8, device="cuda")
        pin_out = torch.empty(both.numel(), dtype=torch.uint8, pin_memory=True)
        up = torch.empty_like(dev)
        res["resize_ms"] = _events_ms(lambda: pipe._resize(dev), WARMUP, ITERS)
        res["network_ms"] = _events_ms(lambda: pipe._network(small), WARMUP, ITERS)
        res["overlay_ms"] = _events_ms(lambda: pipe._overlay(dev, mask_small, overlay, mask), WARMUP, ITERS)
        res["overlay_nomask_ms"] = _events_ms(lambda: pipe._overlay(dev, mask_small, overlay, None), WARMUP, ITERS)
        res["upload_ms"] = _events_ms(lambda: up.copy_(pin_in, non_blocking=True), WARMUP, ITERS)
        res["download_ms"] = _events_ms(lambda: pin_out.copy_(both, non_blocking=True), WARMUP, ITERS)
        # (b) host to host
        rates = []
        for r in range(ROUNDS + 1):   # the first round warms the staging buffers
            t0 = time.perf_counter()
            n = sum(len(o) for o, _ in pipe.run(frames for _ in range(CHUNKS)))
            dt = time.perf_counter() - t0
            if r:
                rates.append(n / dt)
        res["run_fps"] = rates
        # the same chunks through process(), one after another with host arrays in and out: no overlap
        t0 = time.perf_counter()
        for _ in range(CHUNKS):
            o, m = pipe.process(frames)
            o, m = o.cpu().numpy(), m.cpu().numpy()
        res["serial_fps"] = CHUNKS * CHUNK / (time.perf_counter() - t0)
        # (c) the parent's procedure, a frame at a time
        lut = V.jet_table()

        def parent(count):
            for i in range(count):
                rgb = np.ascontiguousarray(frames[i][..., ::-1])
                small1 = stage.resize(torch.from_numpy(rgb).cuda(), (INPUT, INPUT))
                m1 = model.run_u8(small1[None], return_mask=True, **kw)[-1]
                full = stage.resize(m1[0], (WIDTH, HEIGHT)).cpu().numpy()
                _blend_numpy(frames[i], full, lut, 0.7, 0.3, 0.0)

        parent(4)
        t0 = time.perf_counter()
        parent(PARENT_FRAMES)
        res["parent_fps"] = PARENT_FRAMES / (time.perf_counter() - t0)
        # ... and its device part alone (no numpy colouring), to show where the parent's time goes
        t0 = time.perf_counter()
        for i in range(PARENT_FRAMES):
            small1 = stage.resize(torch.from_numpy(frames[i]).cuda(), (INPUT, INPUT))
            m1 = model.run_u8(small1[None], return_mask=True, **kw)[-1]
            stage.resize(m1[0], (WIDTH, HEIGHT)).cpu()
        res["parent_device_only_fps"] = PARENT_FRAMES / (time.perf_counter() - t0)
        if hasattr(model, "device_error"):
            assert model.device_error() == 0
        out["tiers"][name] = res
        model.release()
    print("RESULT " + json.dumps(out))


def _md(m):
    med = statistics.median
    by = m["bytes"]
    lines = ["# The video path per chunk (%d frames of %d x %d, network input %d x %d)" % (CHUNK, HEIGHT, WIDTH, INPUT, INPUT), "",
             "Produced by `python tools/video_timing.py --out profiles/r19/video_pipeline.md` on one MI355X, one process.", "",
             "## (a) The two kernels", "",
             "HIP events around one launch on a resident chunk, median of %d after %d warm-ups.  Bytes are what the algorithm"
             % (ITERS, WARMUP),
             "has to move: overlay %.1f MB a chunk (frames read, overlay written, full-size mask written; without the mask %.1f MB),"
             % (by["overlay"] / 1e6, (by["overlay"] - CHUNK * HEIGHT * WIDTH) / 1e6),
             "resize %.1f MB (frames read, network input written)." % (by["resize"] / 1e6), "",
             "| tier | kernel | device ms | min .. max | GB/s |", "|---|---|---|---|---|"]
    for name, r in m["tiers"].items():
        for label, key, nbytes in (("unet_resize_u8_batch", "resize_ms", by["resize"]),
                                   ("unet_overlay_u8_batch, with mask", "overlay_ms", by["overlay"]),
                                   ("unet_overlay_u8_batch, no mask", "overlay_nomask_ms", by["overlay"] - CHUNK * HEIGHT * WIDTH)):
            d = med(r[key])
            lines.append("| %s | %s | %.4f | %.4f .. %.4f | %.0f |" % (name, label, d, min(r[key]), max(r[key]), nbytes / d / 1e6))
    lines += ["", "## (b) The pipeline, host array in to host array out", "",
              "`FramePipeline.run` over %d chunks, wall clock, median of %d rounds after one warm-up round; `process` is the same"
              % (CHUNKS, ROUNDS),
              "chunks one after another with a host array in and out (no overlap).  The split is each stage of one chunk alone",
              "between HIP events (upload and download from and to pinned memory).", "",
              "| tier | run frames/s | min .. max | process frames/s | upload ms | resize ms | network ms | overlay ms | download ms |",
              "|---|---|---|---|---|---|---|---|---|"]
    for name, r in m["tiers"].items():
        lines.append("| %s | %.0f | %.0f .. %.0f | %.0f | %.3f | %.3f | %.3f | %.3f | %.3f |" % (
            name, med(r["run_fps"]), min(r["run_fps"]), max(r["run_fps"]), r["serial_fps"], med(r["upload_ms"]),
            med(r["resize_ms"]), med(r["network_ms"]), med(r["overlay_ms"]), med(r["download_ms"])))
    lines += ["", "## (c) Against the procedure there was before", "",
              "The same frames, one at a time: upload, `CameraStage.resize`, `run_u8`, `CameraStage.resize` of the mask, download,",
              "colour table and blend in numpy (%d frames after 4 warm-ups, wall clock); the last column is that loop without the"
              % PARENT_FRAMES, "numpy colouring.", "",
              "| tier | run frames/s | frame at a time frames/s | ratio | frame at a time, device part only |", "|---|---|---|---|---|"]
    for name, r in m["tiers"].items():
        lines.append("| %s | %.0f | %.1f | %.1f x | %.1f |" % (name, med(r["run_fps"]), r["parent_fps"],
                                                              med(r["run_fps"]) / r["parent_fps"], r["parent_device_only_fps"]))
    lines += ["", "## Raw lines", "", "```"]
    for name, r in m["tiers"].items():
        for key, v in r.items():
            lines.append("%s %s: %s" % (name, key, " ".join("%.4f" % x for x in v) if isinstance(v, list) else "%.4f" % v))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="video_pipeline.md")
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
        f.write(_md(result))
    print("written " + args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
