#!/usr/bin/env python3
"""Cost of the ensemble combine and of the threshold sweep (csrc/ensemble_kernels.cpp) per batch of 64 frames of
224 x 224, beside what each is measured against.

  python tools/ensemble_sweep_timing.py --out profiles/r20/ensemble_sweep.md [--baseline-lib PATH]

One measurement in a fresh child process under its own time limit.  Two parts:
  (a) combine   unet_ensemble_combine for K = 3 (means and mask written) against the three member forwards alone (model A
                on f16x3, probabilities written), which an ensemble pays whatever combines them;
  (b) sweep     unet_score_sweep_accumulate with T = 19 in both bin-combining variants (unet_set_sweep_combine) on two
                inputs - lane-like logits (8.5 % confident positives, the rest confident negatives: every wave wants one
                counter) and logits spread uniformly over the bins - against unet_seg_metrics_accumulate on the same
                logits and targets, which counts at one threshold.  --baseline-lib names the library that call is taken
                from (a build of the commit before the sweep existed); without it the call comes from this build, whose
                validate_kernels.cpp is the same file.

Every figure is HIP events around REPS back-to-back launches, divided by REPS; median of ROUNDS rounds after WARMUP, the
configurations taking turns within a round.  Each launch of a round reads another of SETS copies of the inputs (more
bytes than the Infinity Cache holds), so the rates are rates from HBM and not from a cache that a repeated launch warmed.
Bytes are what the algorithm has to move.
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

FRAMES, SIDE, K, T = 64, 224, 3, 19
NUMEL = FRAMES * SIDE * SIDE
WARMUP, ROUNDS, REPS, SETS = 2, 9, 24, 24
FORWARD_ITERS = 5
LIMIT = 540
P_LANE = 0.085


def _events_ms(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for r in range(reps):
        fn(r)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(baseline_lib):
    import numpy as np
    import torch
    from unet_lane_detection_amd import _lib, ensemble as E, metrics as M, state as S
    from unet_lane_detection_amd.model import UNetHIP, _logit

    lib = _lib.load(build_if_missing=False)
    base = lib
    if baseline_lib:
        base = C.CDLL(os.path.abspath(baseline_lib))
        for name in ("unet_seg_metrics_accumulate", "unet_op_last_error"):
            fn = getattr(base, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"baseline_lib": os.path.basename(baseline_lib) if baseline_lib else "", "rows": {}}
    rng = np.random.default_rng(0)

    # ---- (a) combine ------------------------------------------------------------------------------------------
    sets = [[torch.rand(NUMEL, device="cuda") for _ in range(K)] for _ in range(SETS // 3)]
    probs_out = torch.empty(NUMEL, device="cuda")
    mask_out = torch.empty(NUMEL, dtype=torch.uint8, device="cuda")
    w = (C.c_float * K)(*E.normalise_weights([1, 2, 3], K))
    ptr_sets = [(C.c_void_p * K)(*[p.data_ptr() for p in ps]) for ps in sets]

    def combine(r, probs=True, mask=True):
        rc = lib.unet_ensemble_combine(0, ptr_sets[r % len(sets)], K, w, NUMEL, 0.5,
                                       C.c_void_p(probs_out.data_ptr() if probs else 0),
                                       C.c_void_p(mask_out.data_ptr() if mask else 0), stream)
        assert rc == 0, lib.unet_op_last_error()

    # ---- (b) sweep --------------------------------------------------------------------------------------------
    th = M.sweep_thresholds(M.DEFAULT_THRESHOLDS, "logit")
    assert th.size == T
    targets = S.synthetic_targets(FRAMES, SIDE, SIDE, seed=3, p=P_LANE).reshape(-1)
    lane = np.where(targets > 0, 6.0, -6.0).astype(np.float32) + rng.standard_normal(NUMEL).astype(np.float32) * 0.5
    u = rng.random(NUMEL)
    uniform = np.log(u / (1.0 - u)).astype(np.float32)
    inputs = {}
    for name, logits in (("lane-like", lane), ("uniform", uniform)):
        want = M.sweep_model(logits, targets, th)
        inputs[name] = {
            "want": want,
            "logits": [torch.from_numpy(logits).cuda().clone() for _ in range(SETS)],
            "float": [torch.from_numpy(targets).cuda().clone() for _ in range(SETS)],
            "bytes": [torch.from_numpy((targets * 255).astype(np.uint8)).cuda().clone() for _ in range(SETS)],
        }
    counts = torch.zeros(2 * (T + 1), dtype=torch.int64, device="cuda")
    acc = torch.zeros(M.NUM_ACCUMULATORS, dtype=torch.float64, device="cuda")
    thp = th.ctypes.data_as(C.POINTER(C.c_float))

    def sweep(r, inp, kind):
        d = inputs[inp]
        rc = lib.unet_score_sweep_accumulate(0, C.c_void_p(d["logits"][r % SETS].data_ptr()),
                                             C.c_void_p(d[kind][r % SETS].data_ptr()), int(kind == "bytes"), NUMEL, thp, T,
                                             C.c_void_p(counts.data_ptr()), stream)
        assert rc == 0, lib.unet_op_last_error()

    def seg(r, inp, kind):
        d = inputs[inp]
        rc = base.unet_seg_metrics_accumulate(0, C.c_void_p(d["logits"][r % SETS].data_ptr()),
                                              C.c_void_p(d[kind][r % SETS].data_ptr()), int(kind == "bytes"), NUMEL,
                                              _logit(0.5), 0, 1.0, 0.0, 1.0, 1e-6, C.c_void_p(acc.data_ptr()), stream)
        assert rc == 0, base.unet_op_last_error()

    # both variants count what the model counts, on both inputs and both target types, before anything is timed
    for variant in (1, 0):
        lib.unet_set_sweep_combine(variant)
        for inp in inputs:
            for kind in ("float", "bytes"):
                counts.zero_()
                sweep(0, inp, kind)
                assert np.array_equal(counts.cpu().numpy().reshape(2, T + 1), inputs[inp]["want"]), (variant, inp, kind)
    lib.unet_set_sweep_combine(1)

    configs = {"combine K=3, means + mask": (lambda r: combine(r), NUMEL * (4 * K + 4 + 1)),
               "combine K=3, mask only": (lambda r: combine(r, probs=False), NUMEL * (4 * K + 1)),
               "combine K=3, means only": (lambda r: combine(r, mask=False), NUMEL * (4 * K + 4))}
    for inp in inputs:
        for kind, per in (("float", 8), ("bytes", 5)):
            for variant, label in ((1, "wave-combined"), (0, "per-lane atomics")):
                def run(r, inp=inp, kind=kind, variant=variant):
                    if r == 0:
                        lib.unet_set_sweep_combine(variant)
                    sweep(r, inp, kind)
                configs["sweep T=19, %s, %s targets, %s" % (inp, kind, label)] = (run, NUMEL * per)
            configs["seg_metrics (one threshold), %s, %s targets" % (inp, kind)] = (
                lambda r, inp=inp, kind=kind: seg(r, inp, kind), NUMEL * per)
    times = {name: [] for name in configs}
    for rnd in range(WARMUP + ROUNDS):
        for name, (fn, _) in configs.items():
            ms = _events_ms(fn, REPS)
            if rnd >= WARMUP:
                times[name].append(ms)
    lib.unet_set_sweep_combine(1)
    for name, (_, nbytes) in configs.items():
        out["rows"][name] = {"ms": times[name], "bytes": nbytes}

    # ---- the member forwards alone ----------------------------------------------------------------------------
    del sets, inputs
    torch.cuda.empty_cache()
    frames = torch.from_numpy(S.synthetic_frames(FRAMES, SIDE, SIDE, seed=7)).cuda()
    models = [UNetHIP(S.seeded_state_dict(seed=s), device=0) for s in range(K)]
    ens = E.Ensemble(models)

    def forwards(_):
        for m in models:
            m.run_u8(frames, return_probs=True, precision="f16x3")
    out["forwards_ms"] = [_events_ms(forwards, 1) for _ in range(2 + FORWARD_ITERS)][2:]
    out["ensemble_ms"] = [_events_ms(lambda _: ens.run_u8(frames, return_mask=True), 1) for _ in range(2 + FORWARD_ITERS)][2:]
    assert ens.device_error() == 0
    for m in models:
        m.release()
    print("RESULT " + json.dumps(out))


def _md(m, cmd):
    med = statistics.median
    rows = m["rows"]
    fwd = med(m["forwards_ms"])
    lines = ["# Ensemble combine and threshold sweep per batch (%d frames of %d x %d = %d elements)" % (FRAMES, SIDE, SIDE, NUMEL), "",
             "Produced by `%s` on one MI355X, one process." % cmd, "",
             "HIP events around %d back-to-back launches, divided by %d; median of %d rounds after %d warm-up rounds, the"
             % (REPS, REPS, ROUNDS, WARMUP),
             "configurations taking turns within a round.  Consecutive launches read different copies of the inputs (%d copies,"
             % SETS,
             "more bytes than the Infinity Cache holds).  Bytes are what the algorithm has to move; GB/s is bytes over the",
             "median time per launch, launch gaps included.", "",
             "## (a) `unet_ensemble_combine`, K = %d" % K, "",
             "| call | bytes / element | ms | min .. max | GB/s | share of the %d member forwards |" % K, "|---|---|---|---|---|---|"]
    for name, r in rows.items():
        if name.startswith("combine"):
            d = med(r["ms"])
            lines.append("| %s | %d | %.4f | %.4f .. %.4f | %.0f | %.3f %% |" % (
                name, r["bytes"] // NUMEL, d, min(r["ms"]), max(r["ms"]), r["bytes"] / d / 1e6, 100.0 * d / fwd))
    lines += ["", "The %d member forwards alone (model A, f16x3, probabilities written): %.3f ms (%.3f .. %.3f, %d runs after 2);"
              % (K, fwd, min(m["forwards_ms"]), max(m["forwards_ms"]), len(m["forwards_ms"])),
              "`Ensemble.run_u8(..., return_mask=True)` on the same frames, forwards and combine: %.3f ms (%.3f .. %.3f)."
              % (med(m["ensemble_ms"]), min(m["ensemble_ms"]), max(m["ensemble_ms"])), "",
              "## (b) `unet_score_sweep_accumulate`, T = %d" % T, "",
              "Beside `unet_seg_metrics_accumulate` on the same logits and targets (one threshold, plus the loss terms), taken from "
              + ("`%s`, a build of the parent commit." % m["baseline_lib"] if m["baseline_lib"] else
                 "this build (its validate_kernels.cpp is the parent commit's)."), "",
              "| input | targets | call | ms | min .. max | GB/s | against seg_metrics | share of the %d member forwards |" % K,
              "|---|---|---|---|---|---|---|---|"]
    for inp in ("lane-like", "uniform"):
        for kind in ("float", "bytes"):
            ref = med(rows["seg_metrics (one threshold), %s, %s targets" % (inp, kind)]["ms"])
            for name, r in rows.items():
                if ", %s, %s targets" % (inp, kind) in name:
                    d = med(r["ms"])
                    call = name.split(",")[0] + ("" if name.startswith("seg") else "," + name.split(",")[-1])
                    lines.append("| %s | %s | %s | %.4f | %.4f .. %.4f | %.0f | %.2f x | %.3f %% |" % (
                        inp, kind, call, d, min(r["ms"]), max(r["ms"]), r["bytes"] / d / 1e6, d / ref, 100.0 * d / fwd))
    lines += ["", "lane-like: logits of +-6 with normal noise of sigma 0.5, %.1f %% positives; uniform: logits whose probabilities are uniform"
              % (100 * P_LANE), "over (0, 1), so every one of the 20 bins of both classes is hit in every wave.", "",
              "## Raw lines", "", "```"]
    for name, r in rows.items():
        lines.append("%s: %s" % (name, " ".join("%.4f" % x for x in r["ms"])))
    lines.append("forwards: " + " ".join("%.4f" % x for x in m["forwards_ms"]))
    lines.append("ensemble: " + " ".join("%.4f" % x for x in m["ensemble_ms"]))
    lines += ["```", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="ensemble_sweep.md")
    ap.add_argument("--baseline-lib", default="", help="a libunet_hip.so to take unet_seg_metrics_accumulate from")
    args = ap.parse_args()
    if args.step:
        measure(args.baseline_lib)
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", "measure"]
    if args.baseline_lib:
        cmd += ["--baseline-lib", args.baseline_lib]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        print(p.stdout[-4000:])
        print("the measurement ended with status %d" % p.returncode)
        return p.returncode or 1
    result = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    shown = "python tools/ensemble_sweep_timing.py --out " + args.out + (" --baseline-lib <parent build>" if args.baseline_lib else "")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(_md(result, shown))
    print("written " + args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
