#!/usr/bin/env python3
"""Cost of the int8 tier's K-class head beside the single-class one (model B = [32, 64, 128], batch 256, 224 x 224).

  python tools/int8_multiclass_timing.py --out profiles/r31/int8_multiclass.md [--parent-lib PATH]

HIP events around every measured call, median of ITERS after WARMUP.  One process measures at a time, each under its
own time limit; a child that ends on a signal or a time limit ends the run.
  (a) heads    the head alone (unet_i8_run_head on the tensor a forward left behind) for K = 2, 3, 8 with three output
               sets - logits, labels, all four - and the single-class head_i8_kernel with its three; beside each a
               device copy that moves as many bytes (the head reads 32 bytes per pixel and writes what the set holds)
  (b) forward  the whole K-class forward for labels alone against the single-class forward with return_mask
  (c) parent   the single-class forward through this tree's library and through --parent-lib (the parent commit's
               libunet_hip.so), alternated in PAIRS pairs of fresh processes
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATS, BATCH, SIZE, WARMUP, ITERS, PAIRS = [32, 64, 128], 256, 224, 3, 20, 3
LIMIT = 300
KS = (2, 3, 8)


def _events_ms(run):
    import torch
    ts = []
    for it in range(WARMUP + ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            ts.append(a.elapsed_time(b))
    return {"ms": statistics.median(ts), "min": min(ts), "max": max(ts)}


def _copy_ms(total_bytes):
    """a device copy that moves `total_bytes` in all: half of them read, half written"""
    import torch
    src = torch.empty(total_bytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return _events_ms(lambda: dst.copy_(src))["ms"]


def _quantised(k):
    """model B with K classes, calibrated on the device (fp32 tier) over a few small frames"""
    import torch
    from unet_lane_detection_amd import quant, state as S
    from unet_lane_detection_amd.int8 import calibrate
    from unet_lane_detection_amd.model import UNetHIP
    sd = S.seeded_state_dict(FEATS, seed=0, out_channels=k)
    fm = UNetHIP(sd, device=0)
    ranges = calibrate(fm, torch.from_numpy(S.synthetic_frames(4, 64, 64, seed=1)), batch=4)
    fm.release()
    return quant.quantize_model(sd, ranges)


def worker_heads(single_path):
    import torch
    from unet_lane_detection_amd import _lib, quant, state as S
    from unet_lane_detection_amd.int8 import UNetInt8
    frames = torch.from_numpy(S.synthetic_frames(BATCH, SIZE, SIZE, seed=1)).cuda()
    px = BATCH * SIZE * SIZE
    c = FEATS[0]
    out = {"pixels": px, "heads": [], "forward": {}}
    p = _lib.ptr
    for k in (1,) + KS:
        qm = _quantised(k)
        if k == 1:
            quant.save_quantized(single_path, qm)
        net = UNetInt8(qm, device=0)
        logits = torch.empty((BATCH, k, SIZE, SIZE), dtype=torch.float32, device="cuda")
        probs = torch.empty_like(logits)
        labels = torch.empty((BATCH, SIZE, SIZE), dtype=torch.uint8, device="cuda")
        mask = torch.empty_like(labels)
        if k == 1:
            net.run_u8(frames, return_mask=True)
            sets = [("logits", (logits, None, None, None), 4), ("mask", (None, None, None, mask), 1),
                    ("logits, probs, mask", (logits, probs, None, mask), 9)]
            out["forward"]["k1_mask"] = _events_ms(lambda: net.run_u8(frames, return_mask=True))
        else:
            net.predict_labels(frames)
            sets = [("logits", (logits, None, None, None), 4 * k), ("labels", (None, None, labels, None), 1),
                    ("logits, probs, labels, mask", (logits, probs, labels, mask), 8 * k + 2)]
            out["forward"][f"k{k}_labels"] = _events_ms(lambda: net.predict_labels(frames))
        for name, (lg, pr, lb, mk), written in sets:
            def run():
                rc = net._lib.unet_i8_run_head(net._h, p(lg), p(pr), p(lb), 1 if k > 1 else 0, p(mk), 0.0, _lib.stream(net.device))
                net._check(rc, "unet_i8_run_head")
            t = _events_ms(run)
            moved = px * (c + written)
            out["heads"].append({"k": k, "outputs": name, "bytes_per_px": c + written, "copy_ms": _copy_ms(moved), **t})
        net.release()
        del logits, probs, labels, mask
    print(json.dumps(out))


def worker_single(lib_path, single_path):
    """the single-class forward through the library at `lib_path`, by the C ABI alone (the parent's library lacks the
    new exports, so the package's loader cannot take it)"""
    import numpy as np
    import torch
    from unet_lane_detection_amd import _lib, quant, state as S
    lib = C.CDLL(lib_path)
    for name in ("unet_i8_create", "unet_i8_load", "unet_i8_finalize", "unet_i8_forward_u8", "unet_i8_destroy", "unet_i8_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    qm = quant.load_quantized(single_path)
    feats = (C.c_int * len(FEATS))(*FEATS)
    h = C.c_void_p()

    def check(rc, where):
        if rc:
            raise SystemExit(f"{where}: {rc} {lib.unet_i8_last_error(h)}")
    check(lib.unet_i8_create(len(FEATS), feats, 0, C.byref(h)), "create")
    for key, v in qm.items():
        if key != "features":
            a = np.ascontiguousarray(v)
            check(lib.unet_i8_load(h, key.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes), key)
    check(lib.unet_i8_finalize(h), "finalize")
    frames = torch.from_numpy(S.synthetic_frames(BATCH, SIZE, SIZE, seed=1)).cuda()
    logits = torch.empty((BATCH, 1, SIZE, SIZE), dtype=torch.float32, device="cuda")
    mask = torch.empty((BATCH, SIZE, SIZE), dtype=torch.uint8, device="cuda")
    p = _lib.ptr
    stream = _lib.stream(torch.device("cuda", 0))
    t = _events_ms(lambda: check(lib.unet_i8_forward_u8(h, p(frames), BATCH, SIZE, SIZE, p(logits), None, p(mask), 0.0, stream), "forward"))
    torch.cuda.synchronize()
    lib.unet_i8_destroy(h)
    print(json.dumps(t))


def child(args):
    """one worker in a fresh process; its JSON line, or SystemExit when it did not end cleanly"""
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)}: exit status {r.returncode}; nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31", "int8_multiclass.md"))
    ap.add_argument("--parent-lib", default=None, help="libunet_hip.so built from the parent commit, for (c)")
    ap.add_argument("--worker", default=None, choices=["heads", "single"])
    ap.add_argument("--lib", default=None)
    ap.add_argument("--single", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.worker == "heads":
        return worker_heads(a.single)
    if a.worker == "single":
        return worker_single(a.lib, a.single)
    from unet_lane_detection_amd.build import LIB
    with tempfile.TemporaryDirectory() as tmp:
        single = os.path.join(tmp, "single.npz")
        res = child(["--worker", "heads", "--single", single])
        pairs = []
        if a.parent_lib:
            for _ in range(PAIRS):
                pairs.append(("this commit", child(["--worker", "single", "--lib", LIB, "--single", single])))
                pairs.append(("parent", child(["--worker", "single", "--lib", os.path.abspath(a.parent_lib), "--single", single])))
    px = res["pixels"]
    gbs = lambda ms, b: px * b / (ms * 1e-3) / 1e9
    L = ["# int8 tier, K-class head: cost at batch %d, %d x %d (model B %s, one MI355X)" % (BATCH, SIZE, SIZE, FEATS), "",
         "Written by tools/int8_multiclass_timing.py: HIP events, medians of %d after %d warm-ups." % (ITERS, WARMUP), "",
         "## (a) The head alone", "",
         "The head reads 32 bytes per pixel (the last int8 tensor) and writes what the output set holds; the copy beside",
         "it moves the same number of bytes (half read, half written).", "",
         "| head | outputs | bytes / pixel | ms (min .. max) | GB/s | copy of as many bytes, ms | head / copy |", "|---|---|---|---|---|---|---|"]
    for r in res["heads"]:
        name = "head_i8_kernel (K = 1)" if r["k"] == 1 else "headk_i8 K = %d" % r["k"]
        L.append("| %s | %s | %d | %.3f (%.3f .. %.3f) | %.0f | %.3f | %.2f |" % (
            name, r["outputs"], r["bytes_per_px"], r["ms"], r["min"], r["max"], gbs(r["ms"], r["bytes_per_px"]), r["copy_ms"],
            r["ms"] / r["copy_ms"]))
    f = res["forward"]
    L += ["", "## (b) The whole forward", "", "| forward | ms (min .. max) | frames / s |", "|---|---|---|",
          "| single-class, logits + mask (run_u8(return_mask=True)) | %.3f (%.3f .. %.3f) | %.0f |" % (
              f["k1_mask"]["ms"], f["k1_mask"]["min"], f["k1_mask"]["max"], BATCH / f["k1_mask"]["ms"] * 1e3)]
    for k in KS:
        t = f["k%d_labels" % k]
        L.append("| K = %d, labels alone (predict_labels) | %.3f (%.3f .. %.3f) | %.0f |" % (k, t["ms"], t["min"], t["max"],
                                                                                       BATCH / t["ms"] * 1e3))
    if pairs:
        L += ["", "## (c) Single-class forward (logits + mask), this commit against the parent commit", "",
              "Fresh processes, alternated.", "", "| library | median ms | min .. max |", "|---|---|---|"]
        for name, t in pairs:
            L.append("| %s | %.3f | %.3f .. %.3f |" % (name, t["ms"], t["min"], t["max"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
