#!/usr/bin/env python3
"""Gradient accumulation and clipping under data parallelism, world_size 2, by hand (the suite's own 2-rank rehearsal,
tests/dp_rehearsal.py, is started by tests/conftest.py and covers the plain step).

  python tools/dp_accum_rehearsal.py [--updates 2] [--out FILE]

Run from a FRESH process: it starts two rank processes (gloo, both on GPU 0, as tests/dp_rehearsal.py does) that train
with accum_steps = 2 and max_grad_norm set low enough to clip, and prints one JSON line.  After every update:
  * both ranks hold bit-identical parameters and Adam moments, the same grad_norm and the same step count;
  * they equal, bit for bit, a single-process replay on one trainer that forms the same sums in the same order: per
    rank (g(micro 1) + g(micro 2)) in fp32, the two ranks' sums added (one fp32 addition: the order of two does not
    matter), the record taken from that bucket, and ONE unet_train_adam_step with the coefficient computed on the host
    from the record as grad_scale (scale 1 / (2 * 2));
  * rank 0's BatchNorm running statistics equal the replay's (rank 0's buffers win every broadcast).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FEATS = [16, 32, 64]
PER_RANK, SIZE, MICRO, MAX_NORM = 3, 64, 2, 0.05


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(args):
    env = dict(os.environ)
    env.update({"WORLD_SIZE": "2", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(free_port()),
                "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")})
    procs = []
    for r in range(2):
        e = dict(env)
        e.update({"RANK": str(r), "LOCAL_RANK": str(r)})
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=e))
    deadline = time.time() + args.timeout
    rc = 0
    while any(p.poll() is None for p in procs):
        if time.time() > deadline or any(p.poll() not in (None, 0) for p in procs):
            rc = 1
            break
        time.sleep(0.2)
    for p in procs:
        if p.poll() is None:
            p.kill()
        rc = rc or (p.returncode or 0)
    return rc


def worker(args):
    import torch
    import torch.distributed as dist

    from unet_lane_detection_amd import dp, state as S
    from unet_lane_detection_amd.trainer import UNetTrainer

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    device = rank % torch.cuda.device_count()
    torch.cuda.set_device(device)
    sd = S.seeded_state_dict(FEATS, seed=5)
    per_micro = PER_RANK * world
    total = per_micro * MICRO * args.updates
    frames = torch.from_numpy(S.synthetic_frames(total, SIZE, SIZE, seed=11))
    targets = torch.from_numpy(S.synthetic_targets(total, SIZE, SIZE, seed=11))

    def shard(update, micro, r):
        base = (update * MICRO + micro) * per_micro
        lo, hi = dp.shard_range(per_micro, r, world)
        return frames[base + lo:base + hi], targets[base + lo:base + hi]

    tr = UNetTrainer(sd, device=device, lr=1e-3, accum_steps=MICRO, max_grad_norm=MAX_NORM)
    ref = UNetTrainer(sd, device=device, lr=1e-3, max_grad_norm=MAX_NORM, process_group=dp.LOCAL) if rank == 0 else None
    result = {"world": world, "updates": args.updates, "accum_steps": MICRO, "max_grad_norm": MAX_NORM,
              "ranks_identical": True, "params_equal_replay": True, "moments_equal_replay": True,
              "bn_equal_replay": True, "bucket_equal_replay": True, "record_equal_replay": True,
              "max_param_diff_vs_replay": 0.0, "clipped": True, "grad_norm": [], "step_count": 0}
    for u in range(args.updates):
        for m in range(MICRO):
            tr.step(*shard(u, m, rank))
        torch.cuda.synchronize()
        flat = torch.cat([tr.params, tr.exp_avg, tr.exp_avg_sq,
                          torch.tensor([tr.grad_norm, tr.step_count], dtype=torch.float32, device=tr.device)]).cpu()
        gathered = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(gathered, flat)
        if rank == 0:
            result["grad_norm"].append(tr.grad_norm)
            result["clipped"] &= tr.grad_norm > MAX_NORM
            for g in gathered[1:]:
                result["ranks_identical"] &= bool(torch.equal(g, gathered[0]))
            sums = [None] * world
            for m in range(MICRO):            # in the order the ranks ran: every forward starts from rank 0's buffers
                bn0, bn_after0 = ref.bn.clone(), None
                for r in range(world):
                    ref.bn.copy_(bn0)
                    ref.forward_backward(*shard(u, m, r))
                    sums[r] = ref.grads.clone() if m == 0 else sums[r] + ref.grads
                    if r == 0:
                        bn_after0 = ref.bn.clone()
                ref.bn.copy_(bn_after0)
            ref.grads.copy_(sums[0] + sums[1])
            ref._grad_pass(ref.grads, ref.grads, None, record=True)
            torch.cuda.synchronize()
            sumsq = float(ref.grad_record[0].item())
            result["bucket_equal_replay"] &= bool(torch.equal(ref.grads, tr.grads))
            result["record_equal_replay"] &= bool(torch.equal(ref.grad_record, tr.grad_record))
            ref.optimizer_step(ref.clip_coefficient(1.0 / (MICRO * world), sumsq))
            torch.cuda.synchronize()
            result["max_param_diff_vs_replay"] = max(result["max_param_diff_vs_replay"],
                                                     float((ref.params - tr.params).abs().max().item()))
            result["params_equal_replay"] &= bool(torch.equal(ref.params, tr.params))
            result["moments_equal_replay"] &= bool(torch.equal(ref.exp_avg, tr.exp_avg) and
                                                   torch.equal(ref.exp_avg_sq, tr.exp_avg_sq))
            result["bn_equal_replay"] &= bool(torch.equal(ref.bn, tr.bn))
    ok = True
    if rank == 0:
        result["step_count"] = tr.step_count
        ok = all(result[k] for k in ("ranks_identical", "params_equal_replay", "moments_equal_replay", "bn_equal_replay",
                                     "clipped")) and tr.step_count == args.updates
        result["ok"] = ok
        line = json.dumps(result)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        ref.release()
    tr.release()
    dist.barrier()
    dist.destroy_process_group()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--timeout", type=float, default=300.0)
    args = ap.parse_args()
    if "RANK" not in os.environ:
        sys.exit(launch(args))
    sys.exit(worker(args))


if __name__ == "__main__":
    main()
