#!/usr/bin/env python3
"""Cost of the general loss (mode 2) in a training step against the BCE + Dice loss it stands beside (model A, batch 64,
224 x 224), and its accuracy on the committed fixture.

  python tools/loss_timing.py --out profiles/r06/focal_loss.md

One measurement in a fresh child process under its own time limit:
  per launch  with per-launch profiling on, the `bce_dice_loss_grad` and `focal_loss_grad` records of a training step
              (three kernels each: partial sums, finalize, gradient), medians of five after two warm-ups; the focal
              record also for gamma = 3.5 (a powf per element) and gamma = 0 (no power);
  step        unprofiled wall time of a whole step (HIP events), `bce_dice` and `focal_dice` alternated in three pairs,
              median of ten steps after two warm-ups per leg;
  accuracy    unet_op_loss_grad on every case of tests/golden/focal.npz: worst |dx - dx64| against the bound of
              tests/test_focal_gpu.py, max(2 * E32, 2^-20 * max|dx64|).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, SIZE, WARMUP, ITERS, STEP_ITERS, PAIRS = 64, 224, 2, 5, 10, 3
LIMIT = 480


def _launch_ms(tr, frames, targets, label):
    import torch
    vals = []
    for it in range(WARMUP + ITERS):
        tr.profile(True)
        tr.step(frames, targets)
        torch.cuda.synchronize()
        recs = [r for r in tr.profile_records() if r[0] == label]
        assert len(recs) == 1, (label, len(recs))
        if it >= WARMUP:
            vals.append(recs[0][1])
    tr.profile(False)
    return vals


def _step_ms(tr, frames, targets):
    import torch
    ts = []
    for it in range(WARMUP + STEP_ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.step(frames, targets)
        b.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            ts.append(a.elapsed_time(b))
    return ts


def _accuracy():
    import numpy as np
    import torch
    from unet_lane_detection_amd import _lib
    lib = _lib.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", "focal.npz"))
    rows = []
    for case in (str(c) for c in g["cases"]):
        wb, wf, wd, pw, alpha, gamma, smooth = (float(v) for v in g[f"{case}/params"])
        x, t = torch.from_numpy(g[f"{case}/x"]).cuda(), torch.from_numpy(g[f"{case}/t"]).cuda()
        terms, dx = torch.zeros(4, device="cuda"), torch.zeros_like(x)
        cfg = _lib.LossConfig(2, wb, wf, wd, pw, alpha, gamma, smooth)
        rc = lib.unet_op_loss_grad(0, C.c_void_p(x.data_ptr()), C.c_void_p(t.data_ptr()), x.numel(), C.byref(cfg),
                                   C.c_void_p(terms.data_ptr()), C.c_void_p(dx.data_ptr()), None)
        _lib.check(rc, "unet_op_loss_grad")
        torch.cuda.synchronize()
        g64 = g[f"{case}/gx64"]
        e32 = float(np.abs(g[f"{case}/gx32"].astype(np.float64) - g64).max())
        gmax = float(np.abs(g64).max())
        bound = max(2 * e32, 2.0 ** -20 * gmax)
        worst = float(np.abs(dx.cpu().numpy().astype(np.float64) - g64).max())
        dterm = float(np.abs(terms.cpu().numpy().astype(np.float64) - g[f"{case}/terms64"]).max())
        rows.append({"case": case, "worst_over_bound": worst / bound, "worst_over_max": worst / gmax,
                     "ref32_over_max": e32 / gmax, "terms_worst": dterm})
    return rows


def step_measure():
    import torch
    from unet_lane_detection_amd import state as S
    from unet_lane_detection_amd.trainer import UNetTrainer
    out = {"accuracy": _accuracy()}
    tr = UNetTrainer(S.seeded_state_dict(seed=0), device=0, lr=1e-4)
    frames = torch.from_numpy(S.synthetic_frames(BATCH, SIZE, SIZE, seed=3)).cuda()
    targets = torch.from_numpy(S.synthetic_targets(BATCH, SIZE, SIZE, seed=3)).cuda()
    launches = {}
    tr.set_loss("bce_dice", 0.5, 0.5, 3.0)
    launches["bce_dice_loss_grad (bce_dice)"] = _launch_ms(tr, frames, targets, "bce_dice_loss_grad")
    for title, kw in (("focal_dice, gamma 2", {}), ("focal_dice, gamma 3.5", {"gamma": 3.5}), ("focal_dice, gamma 0", {"gamma": 0.0})):
        tr.set_loss("focal_dice", **kw)
        launches["focal_loss_grad (%s)" % title] = _launch_ms(tr, frames, targets, "focal_loss_grad")
    out["launch_ms"] = launches
    pairs = []
    for _ in range(PAIRS):
        tr.set_loss("bce_dice", 0.5, 0.5, 3.0)
        a = _step_ms(tr, frames, targets)
        tr.set_loss("focal_dice")
        b = _step_ms(tr, frames, targets)
        pairs.append({"bce_dice": a, "focal_dice": b})
    out["step_ms"] = pairs
    assert tr.device_error() == 0
    tr.release()
    print("RESULT " + json.dumps(out))


def _md(m):
    lines = ["# The general loss (BCE + focal + Dice) in a training step (model A, batch %d, %d x %d)" % (BATCH, SIZE, SIZE), "",
             "Produced by `tools/loss_timing.py` on one MI355X, one process.", "",
             "## Accuracy of `unet_op_loss_grad` on tests/golden/focal.npz", "",
             "Worst `|dx - dx64|` over the elements of a case, against the float64 run of the reference's loss classes; the bound of",
             "`tests/test_focal_gpu.py` is `max(2 * E32, 2^-20 * max|dx64|)`, `E32` the reference's own fp32 run.", "",
             "| case | worst / bound | worst / max\\|dx64\\| | reference fp32 / max\\|dx64\\| | worst loss-term error |", "|---|---|---|---|---|"]
    lines += ["| %s | %.3f | %.2e | %.2e | %.2e |" % (r["case"], r["worst_over_bound"], r["worst_over_max"], r["ref32_over_max"],
                                                     r["terms_worst"]) for r in m["accuracy"]]
    lines += ["", "## Per launch (profiling on: HIP events around the three kernels of the record)", "",
              "Medians of %d after %d warm-ups." % (ITERS, WARMUP), "", "| record | ms (median) | runs |", "|---|---|---|"]
    lines += ["| %s | %.4f | %s |" % (k, statistics.median(v), " ".join("%.4f" % x for x in v)) for k, v in m["launch_ms"].items()]
    lines += ["", "## Whole step (unprofiled, HIP events around `step`)", "",
              "`bce_dice` and `focal_dice` alternated; median of %d steps after %d warm-ups per leg." % (STEP_ITERS, WARMUP), "",
              "| pair | bce_dice ms | focal_dice ms |", "|---|---|---|"]
    lines += ["| %d | %.3f | %.3f |" % (i + 1, statistics.median(p["bce_dice"]), statistics.median(p["focal_dice"]))
              for i, p in enumerate(m["step_ms"])]
    a = [statistics.median(p["bce_dice"]) for p in m["step_ms"]]
    b = [statistics.median(p["focal_dice"]) for p in m["step_ms"]]
    lines += ["", "Spread of the three `bce_dice` legs: %.3f .. %.3f ms; the `focal_dice` legs: %.3f .. %.3f ms." %
              (min(a), max(a), min(b), max(b)), "", "## Raw lines", "", "```"]
    for i, p in enumerate(m["step_ms"]):
        for k in ("bce_dice", "focal_dice"):
            lines.append("pair %d %s: %s" % (i + 1, k, " ".join("%.3f" % x for x in p[k])))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="focal_loss.md")
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
