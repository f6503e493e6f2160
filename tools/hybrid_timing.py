#!/usr/bin/env python3
"""Hybrid quantisation of the int8 tier on model B (seeded weights, synthetic frames): what running units in fp16 costs
and gains.

  python tools/hybrid_timing.py --out profiles/r17/hybrid_timing.md

Configurations: pure int8, every unit hybrid, and the three units `int8.choose_hybrid` picks.  Timing follows the int8
leg of `bench.py --full`: batch 256 of 224 x 224 frames resident on the device, one warm-up forward, then STEPS forwards
between two HIP events on the stream; the configurations alternate and the median of ITERS rounds is reported.  MAE:
`compare_outputs`, mean absolute error of probabilities against the fp32 tier over EVAL other frames.  The
`int8.sensitivity` table (one unit hybrid at a time) over the same frames comes with it."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEATS, SIZE, BATCH, CALIB, EVAL, STEPS, ITERS = [32, 64, 128], 224, 256, 16, 16, 3, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="hybrid_timing.md")
    ap.add_argument("--batch", type=int, default=BATCH)
    args = ap.parse_args()
    import torch
    from unet_lane_detection_amd import int8 as I
    from unet_lane_detection_amd import quant, state as S
    from unet_lane_detection_amd.model import UNetHIP
    sd = S.seeded_state_dict(FEATS, seed=0)
    fm = UNetHIP(sd, device=0)
    ranges = I.calibrate(fm, torch.from_numpy(S.synthetic_frames(CALIB, SIZE, SIZE, seed=50)), batch=8)
    judge = torch.from_numpy(S.synthetic_frames(EVAL, SIZE, SIZE, seed=51)).cuda()
    rows = I.sensitivity(fm, sd, ranges, judge)
    best3 = I.choose_hybrid(fm, sd, ranges, judge, k=3)
    configs = {"pure int8": (), "all %d units hybrid" % len(rows): tuple(quant.unit_names(FEATS)),
               "choose_hybrid(k=3)": tuple(best3)}
    nets = {k: I.UNetInt8(quant.quantize_model(sd, ranges, hybrid=h), device=0) for k, h in configs.items()}
    mae = {k: I.compare_outputs(fm, n, judge) for k, n in nets.items()}
    frames = torch.from_numpy(S.synthetic_frames(32, SIZE, SIZE, seed=52)).cuda().repeat((args.batch + 31) // 32, 1, 1, 1)
    frames = frames[:args.batch].contiguous()
    ms = {k: [] for k in nets}
    for n in nets.values():
        n.run_u8(frames)                 # warm-up: plans the workspace
    torch.cuda.synchronize()
    for _ in range(ITERS):
        for k, n in nets.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(STEPS):
                n.run_u8(frames)
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / STEPS)
    assert fm.device_error() == 0
    med = statistics.median
    base = med(ms["pure int8"])
    lines = ["# Hybrid quantisation on model B: cost and gain", "",
             "Produced by `python tools/hybrid_timing.py` on one MI355X, one process.  Model B %s, seeded random weights," % FEATS,
             "ranges from %d synthetic %d x %d frames ('normal'); %d other frames judge.  Seeded random weights are not a" %
             (CALIB, SIZE, SIZE, EVAL),
             "trained network: read the figures as what this model shows.", "",
             "## Forward at batch %d (ms per forward: median of %d rounds of %d, min .. max)" % (args.batch, ITERS, STEPS), "",
             "| configuration | units | ms | min .. max | over pure int8 | frames/s | MAE mean | MAE max | grade |",
             "|---|---|---|---|---|---|---|---|---|"]
    for k, h in configs.items():
        t = med(ms[k])
        lines.append("| %s | %s | %.3f | %.3f .. %.3f | x %.2f | %.0f | %.6f | %.6f | %s |" % (
            k, ", ".join(h) if 0 < len(h) <= 3 else len(h), t, min(ms[k]), max(ms[k]), t / base, args.batch / t * 1e3,
            mae[k].mean, mae[k].max, mae[k].grade))
    lines += ["", "## `sensitivity`: one unit hybrid at a time (MAE against the fp32 tier; pure int8: %.6f)" % rows[0][2], "",
              "| unit | MAE with this unit hybrid | gain |", "|---|---|---|"]
    for u, m, b in rows:
        lines.append("| %s | %.6f | %+.6f |" % (u, m, b - m))
    lines += ["", "`choose_hybrid(k=3)` picked, in order: %s." % ", ".join(best3), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    for n in nets.values():
        n.release()
    fm.release()
    return 0


if __name__ == "__main__":
    sys.exit(main())
