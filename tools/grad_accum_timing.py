#!/usr/bin/env python3
"""Cost of gradient accumulation, the gradient record and the clipped optimiser step (csrc/grad_kernels.cpp,
adam_rec_kernel in csrc/train_kernels.h, UNetTrainer's accum_steps / max_grad_norm / skip_nonfinite).

  python tools/grad_accum_timing.py --out profiles/r28/grad_accum.md [--parent-root DIR] [--rehearsal FILE]

  (a) passes   at the flagship model's parameter count, in this one process: acc = acc + grads, grads = acc + grads
               with the record, the pure record pass, and - on a trainer, from its per-launch profile - adam_kernel
               against adam_rec_kernel.  A sample of a pass is LAUNCHES back-to-back calls between two HIP events,
               divided by LAUNCHES; median, smallest and largest of ITERS samples after WARMUP.  Beside each, measured
               the same way, a device-to-device copy that moves the same number of bytes (half of them read, half
               written).
  (b) steps    the batch-64 training step at 224 x 224 with the defaults, with clipping only and with accum_steps = 4
               (per micro-batch), each in a fresh child process, host clock around steps that end in the step's own
               wait.  With --parent-root (a checkout of the parent commit with its library built) the parent's step is
               timed the same way before and after, twice, which gives the session's run-to-run spread.
  --rehearsal  the output of tools/dp_accum_rehearsal.py, quoted at the end; without it the report says it was not run.
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
WARMUP, ITERS, LAUNCHES = 3, 15, 10
STEP_WARMUP, STEP_UPDATES = 6, 24
BATCH = 64


def events_ms(fn):
    import torch
    samples = []
    for it in range(WARMUP + ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            samples.append(a.elapsed_time(b) / LAUNCHES)
    return samples


def spread(samples):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(samples), min(samples), max(samples))


def copy_of(nbytes):
    """a device copy that moves nbytes in all: nbytes / 2 read, nbytes / 2 written"""
    import torch
    src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    return events_ms(lambda: dst.copy_(src))


def measure_passes():
    import torch
    sys.path.insert(0, ROOT)
    from unet_lane_detection_amd import _lib, state as S
    from unet_lane_detection_amd.trainer import UNetTrainer
    lib = _lib.load(build_if_missing=False)
    tr = UNetTrainer(S.seeded_state_dict(seed=0), device=0, lr=1e-4)
    P = tr.params.numel()
    tr.grads.normal_(0.0, 1e-3)
    acc = torch.zeros_like(tr.params)
    rec = tr.grad_record
    p, stream = _lib.ptr, lambda: _lib.stream(tr.device)

    def run(dst, a, b, with_record):
        rc = lib.unet_grad_accumulate_f32(0, p(dst), p(a), p(b), P, p(rec) if with_record else None,
                                          p(tr._grad_work) if with_record else None, stream())
        assert rc == 0, lib.unet_op_last_error()
    rows = []
    for name, fn, nbytes in (("acc = acc + grads", lambda: run(acc, acc, tr.grads, False), 12 * P),
                             ("acc = grads (first micro-batch)", lambda: run(acc, tr.grads, None, False), 8 * P),
                             ("grads = acc + grads, with the record", lambda: run(tr.grads, acc, tr.grads, True), 12 * P),
                             ("record only (pure reduction)", lambda: run(tr.grads, tr.grads, None, True), 4 * P)):
        acc.zero_()
        tr.grads.normal_(0.0, 1e-3)
        rows.append(dict(name=name, bytes=nbytes, kernel=events_ms(fn), copy=copy_of(nbytes)))
    # the two optimiser kernels, from the handle's per-launch profile (HIP events around each launch)
    tr.grads.normal_(0.0, 1e-3)
    run(tr.grads, tr.grads, None, True)
    tr.max_grad_norm = 1.0
    tr.profile(True)
    times = {"adam": [], "adam_rec": []}
    for it in range(WARMUP + ITERS):
        tr.optimizer_step(1.0)
        tr.optimizer_step_rec(1.0)
        torch.cuda.synchronize()
        for name, ms, _, _ in tr.profile_records():
            if name in times and it >= WARMUP:
                times[name].append(ms)
        tr.profile(True)          # clears the records
    tr.profile(False)
    copy = copy_of(28 * P)
    for name in ("adam", "adam_rec"):
        rows.append(dict(name="%s_kernel (profile record '%s')" % (name, name), bytes=28 * P, kernel=times[name], copy=copy))
    assert tr.device_error() == 0
    props = torch.cuda.get_device_properties(0)
    tr.release()
    return rows, P, "%s (%s)" % (props.name, getattr(props, "gcnArchName", "?").split(":")[0])


def child_steps(root, mode):
    """one fresh process: the package under `root`, STEP_UPDATES timed updates -> one JSON line"""
    sys.path.insert(0, root)
    import torch
    from unet_lane_detection_amd import state as S
    from unet_lane_detection_amd.trainer import UNetTrainer
    kw = {"clip": dict(max_grad_norm=1.0), "accum4": dict(accum_steps=4)}.get(mode, {})
    tr = UNetTrainer(S.seeded_state_dict(seed=0), device=0, lr=1e-4, **kw)
    x = torch.from_numpy(S.synthetic_frames(BATCH, seed=3)).cuda()
    t = torch.from_numpy(S.synthetic_targets(BATCH, seed=3)).cuda()
    micro = 4 if mode == "accum4" else 1
    samples = []
    for it in range(STEP_WARMUP + STEP_UPDATES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(micro):
            tr.step(x, t)
        torch.cuda.synchronize()
        if it >= STEP_WARMUP:
            samples.append((time.perf_counter() - t0) * 1e3 / micro)
    assert tr.device_error() == 0
    print(json.dumps({"mode": mode, "root": root, "ms": samples, "loss": float(tr.loss.item())}), flush=True)
    tr.release()


def measure_steps(parent_root):
    plan = [("new", ROOT, "defaults"), ("new", ROOT, "clip"), ("new", ROOT, "accum4")]
    if parent_root:
        plan = [("parent", parent_root, "defaults")] + plan + [("parent", parent_root, "defaults"), ("new", ROOT, "defaults")]
    out = []
    for who, root, mode in plan:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--child-root", root],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
        if p.returncode != 0 or line is None:
            raise SystemExit("step timing of %s/%s failed (exit %d):\n%s" % (who, mode, p.returncode, p.stdout[-2000:]))
        r = json.loads(line)
        r["who"] = who
        out.append(r)
    return out


def report(rows, P, device, steps, rehearsal):
    lines = ["# Gradient accumulation, the gradient record and the clipped optimiser step: what they cost", "",
             "`python tools/grad_accum_timing.py`, on %s.  %d parameters (%.1f MB a buffer)." % (device, P, 4 * P / 1e6), "",
             "## (a) passes over the flat buffers", "",
             "Milliseconds per call; a sample is %d back-to-back calls between two HIP events; median (smallest .. largest)"
             % LAUNCHES,
             "of %d samples after %d warm-up samples.  The copy beside each pass moves the same number of bytes, half read"
             % (ITERS, WARMUP),
             "and half written, in the same process.  The two optimiser kernels come from the handle's per-launch profile.",
             "", "| pass | bytes moved, MB | pass ms | GB/s | copy of the same bytes ms | pass / copy |", "|---|---|---|---|---|---|"]
    for r in rows:
        k, c = statistics.median(r["kernel"]), statistics.median(r["copy"])
        lines.append("| %s | %.0f | %s | %.0f | %s | %.2f |" % (r["name"], r["bytes"] / 1e6, spread(r["kernel"]),
                                                               r["bytes"] / k / 1e6, spread(r["copy"]), k / c))
    lines += ["", "## (b) the batch-%d training step at 224 x 224" % BATCH, "",
              "Each row is a fresh process: %d updates after %d warm-up updates, host clock around calls of `step` that end"
              % (STEP_UPDATES, STEP_WARMUP),
              "in a device synchronise; milliseconds per call of `step` (per micro-batch with accumulation), median",
              "(smallest .. largest), in the order they ran.", "", "| code | trainer | ms per step |", "|---|---|---|"]
    names = {"defaults": "defaults", "clip": "max_grad_norm = 1.0", "accum4": "accum_steps = 4, per micro-batch"}
    for r in steps:
        lines.append("| %s | %s | %s |" % ("parent commit" if r["who"] == "parent" else "this commit", names[r["mode"]],
                                           spread(r["ms"])))
    med = lambda who, mode: [statistics.median(r["ms"]) for r in steps if r["who"] == who and r["mode"] == mode]
    parent, new = med("parent", "defaults"), med("new", "defaults")
    if len(parent) == 2:
        lines += ["", "The parent commit timed twice differs from itself by %.2f ms (%.2f %%): the session's run-to-run spread."
                  % (abs(parent[0] - parent[1]), 100 * abs(parent[0] - parent[1]) / min(parent)),
                  "This commit with the defaults: %s ms; the parent: %s ms." % (
                      ", ".join("%.2f" % v for v in new), ", ".join("%.2f" % v for v in parent))]
    else:
        lines += ["", "The parent commit's step was not measured in this run (no --parent-root)."]
    lines += ["", "## The 2-rank rehearsal (`tools/dp_accum_rehearsal.py`)", ""]
    lines += ["```", rehearsal.strip(), "```"] if rehearsal else ["It was not run."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28", "grad_accum.md"))
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--rehearsal", default="", help="file holding the output of tools/dp_accum_rehearsal.py")
    ap.add_argument("--child", default="")
    ap.add_argument("--child-root", default=ROOT)
    args = ap.parse_args()
    if args.child:
        return child_steps(args.child_root, args.child)
    import torch
    if torch.cuda.device_count() < 1:       # does not initialise the device: the children come first
        raise SystemExit("grad_accum_timing needs a GPU: nothing here is measured without one")
    steps = measure_steps(os.path.abspath(args.parent_root) if args.parent_root else "")
    rows, P, device = measure_passes()
    rehearsal = open(args.rehearsal).read() if args.rehearsal and os.path.exists(args.rehearsal) else ""
    text = report(rows, P, device, steps, rehearsal)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
