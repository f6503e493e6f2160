#!/usr/bin/env python3
"""The three calibration algorithms on model B (seeded weights, synthetic frames): what each does to the int8 tier's
agreement with the float tier, and what the histogram pass costs beside the range pass.

  python tools/calibration_compare.py --out profiles/r15/calibration.md

One measurement in a fresh child process under its own time limit.  CALIB frames calibrate, EVAL other frames judge:
  per algorithm   `calibrate`, `quantize_model`, `UNetInt8`; `compare_outputs` (MAE of probabilities against the fp32
                  tier, the reference's acceptance check) and `evaluate` IoU / Dice against the fp32 tier's own masks;
                  how far each range was narrowed, and how many int8 activations sit on a clamp
  timing          HIP events on the stream around `minmax_pass` and `histogram_pass` over the same device-resident
                  calibration frames, alternated, medians of ITERS after WARMUP; the plain fp32 forward over the same
                  frames beside them; host seconds of `range_from_histogram` over all tensors
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

FEATS, SIZE, CALIB, EVAL, BATCH, BINS, WARMUP, ITERS = [32, 64, 128], 224, 96, 32, 8, 2048, 2, 7
LIMIT = 420


def _events_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def step_measure():
    import numpy as np
    import torch
    from unet_lane_detection_amd import int8 as I
    from unet_lane_detection_amd import quant, state as S
    from unet_lane_detection_amd.model import UNetHIP
    sd = S.seeded_state_dict(FEATS, seed=0)
    fm = UNetHIP(sd, device=0)
    calib = torch.from_numpy(S.synthetic_frames(CALIB, SIZE, SIZE, seed=1)).cuda()
    frames = torch.from_numpy(S.synthetic_frames(EVAL, SIZE, SIZE, seed=2)).cuda()
    masks = torch.cat([fm.run_u8(frames[i:i + BATCH], return_mask=True)[1] for i in range(0, EVAL, BATCH)])
    out = {"algorithms": {}, "lane_share": float((masks != 0).float().mean())}
    normal = None
    for algorithm in quant.ALGORITHMS:
        t0 = time.perf_counter()
        ranges = I.calibrate(fm, calib, batch=BATCH, algorithm=algorithm, bins=BINS)
        seconds = time.perf_counter() - t0
        normal = normal or ranges
        net = I.UNetInt8(quant.quantize_model(sd, ranges), device=0)
        cmp_ = I.compare_outputs(fm, net, frames, batch=BATCH)
        m = net.evaluate(frames, masks, batch=BATCH)
        net.run_u8(frames[:BATCH])
        clamp = {}
        for name, (c, level) in zip(quant.tensor_names(len(FEATS))[1:], quant.tensor_shapes(FEATS)[1:]):
            t = net.read_tensor(name, BATCH, SIZE >> level, SIZE >> level)
            clamp[name] = float(((t == 127) | (t == -128)).mean())
        net.release()
        out["algorithms"][algorithm] = {
            "mae_mean": cmp_.mean, "mae_max": cmp_.max, "grade": cmp_.grade, "iou": m.iou, "dice": m.f1,
            "calibrate_s": seconds, "clamped": clamp,
            "width": {k: (ranges[k][1] - ranges[k][0]) / (normal[k][1] - normal[k][0]) for k in ranges}}
    # the two device passes over the same resident frames, alternated; the plain forward beside them
    names = quant.tensor_names(len(FEATS))
    spans = np.array([(min(normal[k][0], 0.0), max(normal[k][1], 0.0)) for k in names], dtype=np.float32)
    legs = {"forward": lambda: [fm.run_u8(calib[i:i + BATCH]) for i in range(0, CALIB, BATCH)],
            "range pass": lambda: I.minmax_pass(fm, calib, BATCH),
            "histogram pass": lambda: I.histogram_pass(fm, calib, spans, BINS, BATCH),
            "histogram pass, 256 bins": lambda: I.histogram_pass(fm, calib, spans, 256, BATCH)}
    ms = {k: [] for k in legs}
    for it in range(WARMUP + ITERS):
        for k, fn in legs.items():
            t = _events_ms(fn)
            if it >= WARMUP:
                ms[k].append(t)
    out["pass_ms"] = ms
    hist = I.histogram_pass(fm, calib, spans, BINS, BATCH)[0].cpu().numpy().view(np.uint64)
    out["zero_share"] = {k: float(hist[i, BINS]) / float(hist[i].sum()) for i, k in enumerate(names)}
    host = {}
    for algorithm in ("mmse", "kl_divergence"):
        t0 = time.perf_counter()
        for i in range(len(names)):
            quant.range_from_histogram(hist[i], float(spans[i, 0]), float(spans[i, 1]), algorithm)
        host[algorithm] = time.perf_counter() - t0
    out["host_s"] = host
    assert fm.device_error() == 0
    fm.release()
    print("RESULT " + json.dumps(out))


def _md(m):
    med = statistics.median
    names = list(m["zero_share"])
    lines = ["# int8 calibration: 'normal', 'mmse' and 'kl_divergence' on model B", "",
             "Produced by `python tools/calibration_compare.py --out profiles/r15/calibration.md` on one MI355X, one process.", "",
             "Model B %s with seeded random weights; %d synthetic %d x %d frames calibrate, %d others judge (batch %d, %d bins)."
             % (FEATS, CALIB, SIZE, SIZE, EVAL, BATCH, BINS),
             "MAE: `compare_outputs`, mean absolute error of probabilities against the fp32 tier (the reference grades the mean:",
             "GOOD < 0.05, ACCEPTABLE < 0.10).  IoU / Dice: `UNetInt8.evaluate` against the fp32 tier's own masks (lane share of those",
             "masks: %.3f).  Seeded random weights are not a trained network: read the figures as what this model shows, not as what"
             % m["lane_share"],
             "the algorithms do for a trained one.", "",
             "| algorithm | MAE mean | MAE max | grade | IoU vs fp32 masks | Dice | calibrate() wall s |", "|---|---|---|---|---|---|---|"]
    for k, a in m["algorithms"].items():
        lines.append("| %s | %.6f | %.6f | %s | %.4f | %.4f | %.2f |" % (k, a["mae_mean"], a["mae_max"], a["grade"], a["iou"],
                                                                     a["dice"], a["calibrate_s"]))
    lines += ["", "## Range width against min/max, exact zeros, and activations on a clamp (first %d judged frames)" % BATCH, "",
              "| tensor | exact zeros | mmse width | kl width | clamped normal | clamped mmse | clamped kl |", "|---|---|---|---|---|---|---|"]
    al = m["algorithms"]
    for k in names:
        cl = [("%.4f %%" % (100 * al[a]["clamped"][k])) if k in al[a]["clamped"] else "-" for a in ("normal", "mmse", "kl_divergence")]
        lines.append("| %s | %.1f %% | %.3f | %.3f | %s | %s | %s |" % (k, 100 * m["zero_share"][k], al["mmse"]["width"][k],
                                                                      al["kl_divergence"]["width"][k], cl[0], cl[1], cl[2]))
    lines += ["", "## The device passes over the %d calibration frames (HIP events on the stream, frames resident)" % CALIB, "",
              "Legs alternated; median of %d after %d warm-ups.  The range pass reads its keys back after every batch; the"
              % (ITERS, WARMUP),
              "histogram pass leaves its counters on the device.", "", "| leg | ms (median) | min .. max | over the forward |", "|---|---|---|---|"]
    fwd = med(m["pass_ms"]["forward"])
    for k, ts in m["pass_ms"].items():
        lines.append("| %s | %.3f | %.3f .. %.3f | %+.3f |" % (k, med(ts), min(ts), max(ts), med(ts) - fwd))
    lines += ["", "Host time of `range_from_histogram` over the %d tensors: mmse %.2f s, kl_divergence %.2f s." %
              (len(names), m["host_s"]["mmse"], m["host_s"]["kl_divergence"]), "", "## Raw lines", "", "```"]
    for k, ts in m["pass_ms"].items():
        lines.append("%s: %s" % (k, " ".join("%.3f" % t for t in ts)))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="calibration.md")
    args = ap.parse_args()
    if args.step:
        step_measure()
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
