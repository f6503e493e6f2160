"""Regenerates tests/golden/train_sequence.json: the ordered profiler labels (names only) of one forward_backward and one
eval_logits of UNetTrainer per case.  Run it on the GPU when the launch sequence of the training handle is changed ON
PURPOSE, and review the diff of the lists.

    python tests/golden/make_golden_train_sequence.py [out.json]
    python tests/golden/make_golden_train_sequence.py --case NAME     (one case, as JSON on the last line of stdout)

tests/test_train_sequence_gpu.py replays the cases and requires equal lists.  The profiler forces the weight gradients
in line; the side-stream modes are tied to that order by test_side_stream_weight_gradients_are_bit_identical.  The cases
are the smallest shapes that reach each branch of the forward walk and of the backward pass (csrc/unet_train.inc):

  a  [64, 128] 2x32x32   planes mode, transposed convolution on f16x3, head in the last unit's pass, pooled planes from
                         the BatchNorm pass (train) or the convolution's epilogue (eval)
  b  [64, 128] 2x28x28   f16x3 units outside planes mode: one split pass per unit, fp32 weight gradient at the odd 7x7
                         bottleneck
  c  [32, 64]  2x32x32   mixed: narrow units exact-fp32, bottleneck units f16x3, head as a launch of its own
  d  [8, 16]   2x32x48   exact fp32 throughout
  e  as a, after unet_set_train_x3(0): the repack, then exact fp32

UNET_TRAIN_POOL_FUSED=0 and UNET_TRAIN_FUSED_STATS=0 are read once per process: case a under each of them is recorded in
a fresh child process (ENV_CASES)."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "train_sequence.json")

CASES = {
    "a": dict(feats=[64, 128], shape=(2, 32, 32)),
    "b": dict(feats=[64, 128], shape=(2, 28, 28)),
    "c": dict(feats=[32, 64], shape=(2, 32, 32)),
    "d": dict(feats=[8, 16], shape=(2, 32, 48)),
    "e": dict(feats=[64, 128], shape=(2, 32, 32), x3_off=True),
}
# name -> (case, environment of the child process)
ENV_CASES = {
    "a_pool_unfused": ("a", {"UNET_TRAIN_POOL_FUSED": "0"}),
    "a_stats_unfused": ("a", {"UNET_TRAIN_FUSED_STATS": "0"}),
}


def record(case):
    """-> {"train": [label, ...], "eval": [label, ...]} of one tiny step in this process"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    from unet_lane_detection_amd import _lib
    from unet_lane_detection_amd import state as S
    from unet_lane_detection_amd.trainer import UNetTrainer
    spec = CASES[case]
    n, hh, ww = spec["shape"]
    frames = torch.from_numpy(S.synthetic_frames(n, hh, ww, seed=3))
    tgt = torch.from_numpy(S.synthetic_targets(n, hh, ww, seed=3))
    lib = _lib.load(build_if_missing=False)
    tr = UNetTrainer(S.seeded_state_dict(spec["feats"], seed=0), device=0, lr=1e-4)
    prev = lib.unet_set_train_x3(0) if spec.get("x3_off") else None
    out = {}
    try:
        for key, run in (("train", lambda: tr.forward_backward(frames, tgt)), ("eval", lambda: tr.eval_logits(frames))):
            tr.profile(True)          # clears the records
            run()
            torch.cuda.synchronize()
            assert tr.device_error() == 0, (case, key)
            out[key] = [r[0] for r in tr.profile_records()]
        tr.profile(False)
    finally:
        if prev is not None:
            lib.unet_set_train_x3(prev)
        tr.release()
    return out


def record_in_child(name, timeout=300):
    """one of ENV_CASES in a fresh process with its environment; raises when the child fails"""
    case, env = ENV_CASES[name]
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], env={**os.environ, **env},
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{name}: child exited with {p.returncode}\n{p.stdout[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def dump(table, path):
    """one line per list: the file is data for a test, and a changed launch shows as one changed line"""
    rows = []
    for name, rec in table.items():
        rows.append('"%s":{\n"train":%s,\n"eval":%s}' % (name, json.dumps(rec["train"], separators=(",", ":")),
                                                       json.dumps(rec["eval"], separators=(",", ":"))))
    with open(path, "w") as f:
        f.write('{"cases":{\n' + ",\n".join(rows) + "}}\n")


def main(out):
    table = {case: record(case) for case in CASES}
    for name in ENV_CASES:            # one after the other; the first failure ends the run
        table[name] = record_in_child(name)
    dump(table, out)
    print("wrote", out, {k: (len(v["train"]), len(v["eval"])) for k, v in table.items()})


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        print(json.dumps(record(sys.argv[2]), separators=(",", ":")))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else TABLE)
