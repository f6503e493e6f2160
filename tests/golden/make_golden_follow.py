"""Generate tests/golden/lane_follow.npz from the REFERENCE's own `LineFollower` (README.md:4068-4126).

Runs only where the reference checkout is available.  It executes the class text with stub rospy, Twist, bridge and
publisher objects and records numeric arrays only (allow_pickle=False).  No reference text is stored.

  masks, scan_rows, centers   small masks, the scan row handed to `find_lane_center` (-1: its default, 70 % height) and
                              its answer (-1: None) - random rows of several densities, rows with exactly 0, 10 and 11
                              white pixels, rows of the values 127 and 128, and a non-default scan row
  traj_masks, traj_angular,   30 masks fed to `mask_callback` one after the other, and the Twist it published for
  traj_linear                 each (NaN where it published nothing): the PID's trajectory, state included

Usage:  python tests/golden/make_golden_follow.py --reference <reference checkout>
"""
import argparse
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CLASS_LINES = (4068, 4126)


class _Twist:
    def __init__(self):
        self.linear = types.SimpleNamespace(x=0.0, y=0.0, z=0.0)
        self.angular = types.SimpleNamespace(x=0.0, y=0.0, z=0.0)


class _Publisher:
    def __init__(self, *a, **k):
        self.sent = []

    def publish(self, msg):
        self.sent.append(msg)


class _Bridge:
    def imgmsg_to_cv2(self, msg, encoding):
        assert encoding == "mono8"
        return msg          # the "message" is the mask itself


def load_line_follower(ref_root):
    with open(os.path.join(ref_root, "README.md"), encoding="utf-8") as f:
        lines = f.read().split("\n")
    lo, hi = CLASS_LINES
    rospy = types.SimpleNamespace(init_node=lambda *a, **k: None, Publisher=_Publisher,
                                  Subscriber=lambda *a, **k: None, loginfo=lambda *a, **k: None)
    ns = {"rospy": rospy, "np": np, "Twist": _Twist, "CvBridge": _Bridge, "Image": object}
    exec(compile("\n".join(lines[lo - 1:hi]), "reference:README.md", "exec"), ns)  # noqa: S102 - the reference oracle
    return ns["LineFollower"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    follower = load_line_follower(args.reference)()
    rng = np.random.default_rng(21)
    h, w = 10, 97
    default = int(h * 0.7)
    masks, rows = [], []
    for i in range(32):                                   # random bytes, white share from 2 % to 90 %
        m = rng.integers(0, 256, (h, w), dtype=np.uint8)
        m[rng.random((h, w)) > (0.02 + 0.88 * i / 31)] = 0
        masks.append(m)
        rows.append(-1 if i % 4 else int(rng.integers(0, h)))
    for count in (0, 10, 11):                             # the "more than 10" rule
        m = np.zeros((h, w), dtype=np.uint8)
        m[default, rng.choice(w, count, replace=False)] = 255
        masks.append(m)
        rows.append(-1)
    for value in (127, 128):                              # the "above 127" rule
        m = np.full((h, w), value, dtype=np.uint8)
        masks.append(m)
        rows.append(-1)
    m = np.zeros((h, w), dtype=np.uint8)                  # a non-default scan row: the lane is only there
    m[3, 40:60] = 200
    masks += [m, m]
    rows += [3, -1]
    centers = []
    for m, r in zip(masks, rows):
        c = follower.find_lane_center(m) if r < 0 else follower.find_lane_center(m, scan_row=r)
        centers.append(-1 if c is None else int(c))

    tw = 64
    traj = np.zeros((30, h, tw), dtype=np.uint8)
    for t in range(30):
        if t in (7, 8, 19):                               # frames without a lane: nothing published, state kept
            continue
        x0 = int(np.clip(20 + 18 * np.sin(t / 4.0) + rng.integers(-3, 4), 0, tw - 14))
        traj[t, default, x0:x0 + 14] = 255
    angular, linear = [], []
    for t in range(30):
        before = len(follower.cmd_pub.sent)
        follower.mask_callback(traj[t])
        if len(follower.cmd_pub.sent) > before:
            cmd = follower.cmd_pub.sent[-1]
            angular.append(float(cmd.angular.z))
            linear.append(float(cmd.linear.x))
        else:
            angular.append(np.nan)
            linear.append(np.nan)
    out = os.path.join(HERE, "lane_follow.npz")
    np.savez_compressed(out, masks=np.stack(masks), scan_rows=np.asarray(rows, dtype=np.int64),
                        centers=np.asarray(centers, dtype=np.int64), traj_masks=traj,
                        traj_angular=np.asarray(angular, dtype=np.float64), traj_linear=np.asarray(linear, dtype=np.float64))
    print(out, os.path.getsize(out), "bytes;", sum(c >= 0 for c in centers), "of", len(centers), "rows have a centre;",
          int(np.isfinite(angular).sum()), "of 30 callbacks published")


if __name__ == "__main__":
    main()
