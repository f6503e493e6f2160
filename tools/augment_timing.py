#!/usr/bin/env python3
"""Cost of the augmentation stage (augment.Augmenter.apply -> unet_augment_u8) per 64-frame 224 x 224 batch, beside one
training step on the batch it produced (model A).

  python tools/augment_timing.py --out profiles/r07/augment.md

One measurement in a fresh child process under its own time limit.  960 frames and masks are resident on the device
(the size of the reference's training set); every batch gathers 64 of them through a fresh permutation.  Three legs:
  all on    every operation forced on (p = 1 for flip, rotation, brightness / contrast, HSV and blur)
  all off   every probability 0: the pure gather, and the masks' targets
  default   the reference's probabilities (0.5, 0.5, 0.7, 0.7, 0.3)
per leg:
  device ms   HIP events around `apply` with a table drawn beforehand (the table's upload and the one launch), median
              of ITERS batches after WARMUP;
  host ms     wall time of `sample_params` for one batch (numpy, no device work), median;
  step ms     HIP events around `trainer.step` on the batch the leg produced, the legs alternated in PAIRS rounds.
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

BATCH, SIZE, RESIDENT, WARMUP, ITERS, STEP_ITERS, PAIRS = 64, 224, 960, 3, 20, 10, 3
LIMIT = 480
LEGS = (("all on", dict(p_flip=1.0, p_rotate=1.0, p_brightness_contrast=1.0, p_hsv=1.0, p_blur=1.0)),
        ("all off", dict(p_flip=0.0, p_rotate=0.0, p_brightness_contrast=0.0, p_hsv=0.0, p_blur=0.0)),
        ("default", {}))


def bytes_moved(with_masks=True):
    """What one batch has to move: every source frame and mask byte read once, every output byte written once."""
    px = BATCH * SIZE * SIZE
    return px * 3 + px * 3 + (px + px * 4 if with_masks else 0)


def _events_ms(fn, warmup, iters):
    import torch
    ts = []
    for it in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(it)
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ts.append(a.elapsed_time(b))
    return ts


def step_measure():
    import numpy as np
    import torch
    from unet_lane_detection_amd import augment as A
    from unet_lane_detection_amd import state as S
    from unet_lane_detection_amd.trainer import UNetTrainer
    frames = torch.from_numpy(S.synthetic_frames(BATCH, SIZE, SIZE, seed=3)).cuda().repeat(RESIDENT // BATCH, 1, 1, 1)
    masks = torch.from_numpy((S.synthetic_targets(BATCH, SIZE, SIZE, seed=3)[:, 0] * 255).astype(np.uint8)).cuda()
    ds = A.DeviceDataset(frames, masks.repeat(RESIDENT // BATCH, 1, 1), device=0)
    out = {"bytes": bytes_moved(), "legs": {}}
    batches = {}
    for name, kw in LEGS:
        aug = A.Augmenter(seed=1, **kw)
        order = np.random.default_rng(2)
        tables = [aug.sample_params(BATCH, RESIDENT, order.permutation(RESIDENT)[:BATCH]) for _ in range(WARMUP + ITERS)]
        host = []
        for _ in range(ITERS):
            t0 = time.perf_counter()
            aug.sample_params(BATCH, RESIDENT, np.arange(BATCH))
            host.append((time.perf_counter() - t0) * 1e3)
        buf = (torch.empty((BATCH, SIZE, SIZE, 3), dtype=torch.uint8, device="cuda"),
               torch.empty((BATCH, 1, SIZE, SIZE), dtype=torch.float32, device="cuda"))
        dev = _events_ms(lambda it: aug.apply(ds.images, ds.masks, tables[it], out=buf), WARMUP, ITERS)
        batches[name] = (buf[0].clone(), buf[1].clone())
        blur = np.concatenate([t["blur"] for t in tables[WARMUP:]])
        out["legs"][name] = {"device_ms": dev, "host_ms": host, "blurred_share": float((blur > 1).mean())}
    tr = UNetTrainer(S.seeded_state_dict(seed=0), device=0, lr=1e-4)
    rounds = []
    for _ in range(PAIRS):
        rounds.append({name: _events_ms(lambda it, b=batches[name]: tr.step(*b), 2, STEP_ITERS) for name, _ in LEGS})
    out["step_ms"] = rounds
    assert tr.device_error() == 0
    tr.release()
    print("RESULT " + json.dumps(out))


def _md(m):
    med = statistics.median
    steps = [med(r[name]) for r in m["step_ms"] for name, _ in LEGS]
    step = med(steps)
    lines = ["# The augmentation stage per batch (batch %d, %d x %d, %d frames resident), beside a training step of model A"
             % (BATCH, SIZE, SIZE, RESIDENT), "",
             "Produced by `python tools/augment_timing.py --out profiles/r07/augment.md` on one MI355X, one process.", "",
             "One launch per batch (`unet_augment_u8`): gather through the table's source index, flip / rotation, brightness /",
             "contrast, HSV, blur, and the masks' targets.  Device time is HIP events around `Augmenter.apply` with the table drawn",
             "beforehand - the 5 KB table's upload and the launch; host time is `sample_params` for one batch (numpy only).", "",
             "| leg | device ms (median of %d) | min .. max | share of the %.1f ms step | blurred samples | host ms to draw the table |"
             % (ITERS, step), "|---|---|---|---|---|---|"]
    for name, _ in LEGS:
        leg = m["legs"][name]
        d = med(leg["device_ms"])
        lines.append("| %s | %.4f | %.4f .. %.4f | %.2f %% | %.0f %% | %.3f |" % (
            name, d, min(leg["device_ms"]), max(leg["device_ms"]), 100.0 * d / step, 100 * leg["blurred_share"], med(leg["host_ms"])))
    mb = m["bytes"] / 1e6
    lines += ["", "Bytes one batch has to move (frames and masks read once, frames and fp32 targets written once): %.1f MB, which is"
              % mb, "%.1f us at the 6 TB/s a streaming copy reaches on this part; the rest of the device time is arithmetic, the launch and the\ntable's upload." % (m["bytes"] / 6e12 * 1e6), "",
              "## The training step on the batch each leg produced (HIP events around `step`)", "",
              "Legs alternated in %d rounds; median of %d steps after 2 warm-ups per leg and round." % (PAIRS, STEP_ITERS), "",
              "| round | " + " | ".join("%s ms" % n for n, _ in LEGS) + " |", "|---|" + "---|" * len(LEGS)]
    lines += ["| %d | " % (i + 1) + " | ".join("%.3f" % med(r[n]) for n, _ in LEGS) + " |" for i, r in enumerate(m["step_ms"])]
    lines += ["", "## Raw lines", "", "```"]
    for name, _ in LEGS:
        lines.append("%s device: %s" % (name, " ".join("%.4f" % x for x in m["legs"][name]["device_ms"])))
    for i, r in enumerate(m["step_ms"]):
        for name, _ in LEGS:
            lines.append("round %d step on %s: %s" % (i + 1, name, " ".join("%.3f" % x for x in r[name])))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="augment.md")
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
