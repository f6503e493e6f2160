#!/usr/bin/env python3
"""Time of one validation batch against the train-mode forward it replaces, per launch (model A, batch 64, 224 x 224).

  python tools/validate_timing.py --out profiles/r05/validate_batch64.md

Two measurements, each in a fresh child process under its own time limit; the second only starts if the first ended
well:
  measure    with per-launch profiling on: one training step, the launches of its forward half (everything before the
             loss kernel) summed; then one validate() batch of the same shape in the same process.  Medians of five
             after two warm-ups, per launch and for the totals; plus the unprofiled wall time of both (HIP events).
  roundtrip  what validation cost without the eval pass, once: trainer.state_dict() to the host, a second UNetHIP
             from it (unet_load_param x 118 + unet_finalize).
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

BATCH, SIZE, WARMUP, ITERS = 64, 224, 2, 5
LIMITS = {"measure": 420, "roundtrip": 240}


def _trainer():
    import torch
    from unet_lane_detection_amd import state as S
    from unet_lane_detection_amd.trainer import UNetTrainer
    tr = UNetTrainer(S.seeded_state_dict(seed=0), device=0, lr=1e-4)
    frames = torch.from_numpy(S.synthetic_frames(BATCH, SIZE, SIZE, seed=3)).cuda()
    targets = torch.from_numpy(S.synthetic_targets(BATCH, SIZE, SIZE, seed=3)).cuda()
    return tr, frames, targets


def _table(runs):
    """runs: ITERS lists of (name, ms) with the same launch sequence -> [(name, median ms)]"""
    assert all([n for n, _ in r] == [n for n, _ in runs[0]] for r in runs), "the launch sequence changed between runs"
    return [(runs[0][i][0], statistics.median(r[i][1] for r in runs)) for i in range(len(runs[0]))]


def step_measure():
    import torch
    tr, frames, targets = _trainer()
    fwd_runs, val_runs = [], []
    for it in range(WARMUP + ITERS):
        tr.profile(True)
        tr.step(frames, targets)
        torch.cuda.synchronize()
        recs = tr.profile_records()
        cut = next(i for i, r in enumerate(recs) if r[0].startswith("bce_"))      # the loss kernel
        tr.profile(True)
        tr.validate([(frames, targets)])
        torch.cuda.synchronize()
        vrecs = tr.profile_records()
        if it >= WARMUP:
            fwd_runs.append([(r[0], r[1]) for r in recs[:cut]])
            val_runs.append([(r[0], r[1]) for r in vrecs])
    tr.profile(False)

    def wall(fn):
        ts = []
        for it in range(WARMUP + ITERS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if it >= WARMUP:
                ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    acc_wall = wall(lambda: tr.validate([(frames, targets)]))
    eval_wall = wall(lambda: tr.eval_logits(frames))
    step_wall = wall(lambda: tr.step(frames, targets))
    out = {"train_forward": _table(fwd_runs), "validate": _table(val_runs),
           "train_forward_totals": [sum(ms for _, ms in r) for r in fwd_runs],
           "validate_totals": [sum(ms for _, ms in r) for r in val_runs],
           "validate_wall_ms": acc_wall, "eval_forward_wall_ms": eval_wall, "train_step_wall_ms": step_wall}
    tr.release()
    print("RESULT " + json.dumps(out))


def step_roundtrip():
    import torch
    from unet_lane_detection_amd.model import UNetHIP
    tr, frames, targets = _trainer()
    tr.step(frames, targets)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sd = tr.state_dict()
    t1 = time.perf_counter()
    net = UNetHIP(sd, device=0)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    net.run_u8(frames)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    net.release()
    tr.release()
    print("RESULT " + json.dumps({"state_dict_s": t1 - t0, "unethip_load_finalize_s": t2 - t1,
                                  "first_forward_s": t3 - t2}))


def _md(m, r):
    lines = ["# One validation batch against the train-mode forward (model A, batch %d, %d x %d)" % (BATCH, SIZE, SIZE), "",
             "Produced by `tools/validate_timing.py` on one MI355X.  Per-launch profiling on (HIP events around every launch, side",
             "stream off), one process, medians of %d after %d warm-ups." % (ITERS, WARMUP), ""]
    tf, tv = statistics.median(m["train_forward_totals"]), statistics.median(m["validate_totals"])
    lines += ["| | sum of launches, ms (median) | runs |", "|---|---|---|",
              "| forward half of a training step (every launch before the loss kernel) | %.3f | %s |" %
              (tf, " ".join("%.3f" % v for v in m["train_forward_totals"])),
              "| eval-mode forward of one `validate` batch | %.3f | %s |" % (tv, " ".join("%.3f" % v for v in m["validate_totals"])),
              "", "Eval / train forward = %.3f.  Unprofiled wall time (HIP events around the calls, median of %d): "
              "`eval_logits` %.3f ms, `validate` of one batch (forward + metrics reduction + the host read of 16 numbers) "
              "%.3f ms, a whole training step %.3f ms." % (tv / tf, ITERS, m["eval_forward_wall_ms"], m["validate_wall_ms"],
                                                         m["train_step_wall_ms"]), ""]
    for title, key in (("Training step, forward half", "train_forward"), ("Validation batch (eval-mode forward)", "validate")):
        lines += ["## %s" % title, "", "| # | launch | ms |", "|---|---|---|"]
        lines += ["| %d | %s | %.4f |" % (i, n, ms) for i, (n, ms) in enumerate(m[key])]
        agg = {}
        for n, ms in m[key]:
            agg[n] = agg.get(n, 0.0) + ms
        lines += ["", "By label: " + ", ".join("%s %.3f" % (n, ms) for n, ms in sorted(agg.items(), key=lambda kv: -kv[1])), ""]
    lines += ["## The host round trip this replaces (measured once)", "",
              "| step | s |", "|---|---|",
              "| `trainer.state_dict()` (parameters and buffers to the host) | %.3f |" % r["state_dict_s"],
              "| second `UNetHIP` from it (`unet_load_param` x 118 + `unet_finalize`: host folding and packing) | %.3f |" % r["unethip_load_finalize_s"],
              "| its first `run_u8` of the batch (workspace allocation included) | %.3f |" % r["first_forward_s"], ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="validate_batch64.md")
    args = ap.parse_args()
    if args.step:
        {"measure": step_measure, "roundtrip": step_roundtrip}[args.step]()
        return 0
    results = {}
    for name in ("measure", "roundtrip"):      # chained: a failure ends the run
        p = subprocess.run(["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            print(p.stdout[-4000:])
            print("step %s ended with status %d: stopping" % (name, p.returncode))
            return p.returncode or 1
        results[name] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(_md(results["measure"], results["roundtrip"]))
    print("written " + args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
