#!/usr/bin/env python3
"""Cost of the multi-class path beside the single-class one it stands next to (model A, batch 64, 224 x 224).

  python tools/multiclass_timing.py --out profiles/r30/multiclass.md [--parent-root DIR]

Every measurement runs in a fresh child process under its own time limit; a child that ends on a signal or a time
limit ends the run.
  heads    per-launch records (HIP events around the launch) of one forward: `headk` (K = 2, 3, 8; fp32 tier) and
           `headk_f16x3` (planes) beside `head1x1` of a single-class model, and a device copy of the head's input bytes
           (64 channels x 4 bytes per pixel) timed in the same process; medians of five after two warm-ups
  train    per-launch records of a training step at K = 3 (`headk`, `class_loss_grad`, `headk_bwd`) and K = 1
           (`bce_dice_loss_grad`, `head_bwd` - the rank-1 form, which stores no dA), then the unprofiled step (HIP
           events), median of ten after two warm-ups
  step     the unprofiled K = 1 step of this tree and of the tree under --parent-root (a checkout of the parent commit,
           built), alternated in two pairs
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, SIZE, WARMUP, ITERS, STEP_ITERS = 64, 224, 2, 5, 10
LIMIT = 420


def _records(obj, run, labels):
    import torch
    vals = {name: [] for name in labels}
    for it in range(WARMUP + ITERS):
        obj.profile(True)
        run()
        torch.cuda.synchronize()
        recs = obj.profile_records()
        if it >= WARMUP:
            for name in labels:
                ms = [r[1] for r in recs if r[0] == name]
                if ms:
                    vals[name].append(sum(ms))
    obj.profile(False)
    return {name: statistics.median(v) for name, v in vals.items() if v}


def _events(run, iters):
    import torch
    ts = []
    for it in range(WARMUP + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            ts.append(a.elapsed_time(b))
    return ts


def worker_heads():
    import torch
    from unet_lane_detection_amd import state as S
    from unet_lane_detection_amd.model import UNetHIP
    frames = torch.from_numpy(S.synthetic_frames(BATCH, SIZE, SIZE, seed=1)).cuda()
    out = {}
    for k in (1, 2, 3, 8):
        m = UNetHIP(S.seeded_state_dict(seed=0, out_channels=k), device=0)
        if k == 1:
            out["head1x1"] = _records(m, lambda: m.run_u8(frames, return_probs=True, return_mask=True), ["head1x1"])["head1x1"]
        else:
            for tier, label in (("fp32", "headk"), ("f16x3", "headk_f16x3")):
                run = lambda: m.run_u8(frames, return_probs=True, return_labels=True, mask_class=1, precision=tier)
                out[f"{label}_k{k}"] = _records(m, run, [label])[label]
                run = lambda: m.run_u8(frames, precision=tier)
                out[f"{label}_k{k}_logits_only"] = _records(m, run, [label])[label]
        m.release()
    src = torch.empty(BATCH * SIZE * SIZE * 64, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    out["copy_input_bytes"] = statistics.median(_events(lambda: dst.copy_(src), 10))
    out["pixels"] = BATCH * SIZE * SIZE
    print(json.dumps(out))


def worker_train(k):
    import numpy as np
    import torch
    from unet_lane_detection_amd import state as S
    from unet_lane_detection_amd.trainer import UNetTrainer
    frames = torch.from_numpy(S.synthetic_frames(BATCH, SIZE, SIZE, seed=1)).cuda()
    tr = UNetTrainer(S.seeded_state_dict(seed=0, out_channels=k), device=0, lr=1e-4)
    if k == 1:
        tgt = torch.from_numpy(S.synthetic_targets(BATCH, SIZE, SIZE, seed=1)).cuda()
        tr.set_loss("bce_dice", 0.5, 0.5, 3.0)
        labels = ["bce_dice_loss_grad", "head_bwd", "head1x1"]
    else:
        rng = np.random.default_rng(1)
        tgt = torch.from_numpy(rng.integers(0, k, size=(BATCH, SIZE, SIZE)).astype(np.uint8)).cuda()
        tr.set_loss("ce_dice", smooth=1.0)
        labels = ["class_loss_grad", "headk_bwd", "headk"]
    out = _records(tr, lambda: tr.step(frames, tgt), labels)
    ts = _events(lambda: tr.step(frames, tgt), STEP_ITERS)
    out["step_ms"] = statistics.median(ts)
    out["step_min"], out["step_max"] = min(ts), max(ts)
    tr.release()
    print(json.dumps(out))


def worker_step():
    import torch
    from unet_lane_detection_amd import state as S
    from unet_lane_detection_amd.trainer import UNetTrainer
    frames = torch.from_numpy(S.synthetic_frames(BATCH, SIZE, SIZE, seed=1)).cuda()
    tgt = torch.from_numpy(S.synthetic_targets(BATCH, SIZE, SIZE, seed=1)).cuda()
    tr = UNetTrainer(S.seeded_state_dict(seed=0), device=0, lr=1e-4)
    ts = _events(lambda: tr.step(frames, tgt), STEP_ITERS)
    tr.release()
    print(json.dumps({"step_ms": statistics.median(ts), "step_min": min(ts), "step_max": max(ts)}))


def child(args, root=ROOT):
    """One worker in a fresh process importing the package under `root`; its JSON line, or SystemExit on a fault"""
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--root", root] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)} under {root}: exit status {r.returncode}; nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30", "multiclass.md"))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit, for the K = 1 step")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--worker", default=None, choices=["heads", "train", "step"])
    ap.add_argument("--k", type=int, default=3)
    a = ap.parse_args()
    if a.worker:
        sys.path.insert(0, a.root)
        {"heads": worker_heads, "train": lambda: worker_train(a.k), "step": worker_step}[a.worker]()
        return
    heads = child(["--worker", "heads"])
    t3 = child(["--worker", "train", "--k", "3"])
    t1 = child(["--worker", "train", "--k", "1"])
    steps = []
    if a.parent_root:
        for _ in range(2):
            steps.append(("this commit", child(["--worker", "step"])))
            steps.append(("parent", child(["--worker", "step"], root=os.path.abspath(a.parent_root))))
    px = heads["pixels"]
    gbs = lambda ms, bytes_per_px: px * bytes_per_px / (ms * 1e-3) / 1e9
    L = ["# Multi-class path: per-launch cost at batch 64, 224 x 224 (model A, one MI355X)", "",
         "Written by tools/multiclass_timing.py; per-launch figures are medians of five HIP-event records after two",
         "warm-ups, steps medians of ten.  The heads read 64 channels x 4 bytes per pixel and write at most 9 K + 2.", "",
         "## Heads", "", "| launch | outputs | ms | GB/s over the bytes it moves |", "|---|---|---|---|",
         f"| device copy of the input bytes (read + write 256 B/px) | - | {heads['copy_input_bytes']:.3f} | "
         f"{gbs(heads['copy_input_bytes'], 512):.0f} |",
         f"| head1x1 (K = 1, fp32) | logits, probs, mask | {heads['head1x1']:.3f} | {gbs(heads['head1x1'], 256 + 9):.0f} |"]
    for k in (2, 3, 8):
        for label, inb in (("headk", 256), ("headk_f16x3", 256)):
            L.append(f"| {label} K = {k} | logits, probs, labels, mask | {heads[f'{label}_k{k}']:.3f} | "
                     f"{gbs(heads[f'{label}_k{k}'], inb + 8 * k + 2):.0f} |")
            L.append(f"| {label} K = {k} | logits | {heads[f'{label}_k{k}_logits_only']:.3f} | "
                     f"{gbs(heads[f'{label}_k{k}_logits_only'], inb + 4 * k):.0f} |")
    L += ["", "## Training step", "", "| record | K = 1 | K = 3 |", "|---|---|---|",
          f"| head forward (ms) | {t1.get('head1x1', float('nan')):.3f} (head1x1; absent where it rides in the last unit) | {t3['headk']:.3f} (headk) |",
          f"| loss passes (ms) | {t1['bce_dice_loss_grad']:.3f} (bce_dice_loss_grad) | {t3['class_loss_grad']:.3f} (class_loss_grad) |",
          f"| head backward (ms) | {t1['head_bwd']:.3f} (head_bwd, rank-1: no dA stored) | {t3['headk_bwd']:.3f} (headk_bwd, dA stored) |",
          f"| step, unprofiled (ms) | {t1['step_ms']:.2f} ({t1['step_min']:.2f} .. {t1['step_max']:.2f}) | "
          f"{t3['step_ms']:.2f} ({t3['step_min']:.2f} .. {t3['step_max']:.2f}) |"]
    if steps:
        L += ["", "## K = 1 step, this commit against the parent commit (same session, alternated)", "",
              "| tree | median ms | min .. max |", "|---|---|---|"]
        for name, s in steps:
            L.append(f"| {name} | {s['step_ms']:.2f} | {s['step_min']:.2f} .. {s['step_max']:.2f} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
