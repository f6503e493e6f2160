#!/usr/bin/env python3
"""Generate tests/golden/focal.npz and tests/golden/tiny_f4_8_focal2.npz from the REFERENCE's own loss classes.

Runs only where the reference checkout is available.  Like make_golden_val.py it extracts code blocks of the reference's
README as text at run time - `DiceLoss` (README.md:1781-1807), `BCEDiceLoss` (:1855-1893), `FocalLoss` (:1914-1939),
`get_sample_weights` (:2544-2553), `UNet` (:1418-1481) - executes them against torch-CPU and records numeric arrays
only (allow_pickle=False).  No reference source is written into this repository.  (`calculate_pos_weight`, :2514-2530,
reads its masks through cv2, which is not available here; tests/test_imbalance_cpu.py restates its three lines of
arithmetic instead.)

focal.npz - per case `<c>/`: `x` logits, `t` targets (float32), `params` = (bce_weight, focal_weight, dice_weight,
pos_weight, alpha, gamma, smooth), and from the reference classes run in float64 and in float32 `terms64` / `terms32` =
(total, bce, dice, focal) and `gx64` / `gx32` = d total / d x, with
    total = bce_weight * BCEWithLogits(pos_weight) + focal_weight * FocalLoss(alpha, gamma) + dice_weight * DiceLoss(smooth)
(the first and third through BCEDiceLoss, as the training script composes them).  Logits: 2048 values each of N(0, 1),
N(0, 4), N(0, 12) (standard deviations), then +-30, +-60, +-87, +-100, +-120, each with t = 0 and t = 1 - beyond the
range where exp(-|x|) underflows in fp32.  Targets: Bernoulli(0.085), the lane ratio the reference measures
(README.md:2534); the case `soft` maps them to 0.05 / 0.95.

tiny_f4_8_focal2.npz - two AdamW steps of the reference UNet([4, 8]) under 0.5 * FocalLoss(0.25, 2) + 0.5 * DiceLoss, made
the way make_golden.py --only adamw makes tiny_f4_8_adamw2.npz (same weights, inputs and (lr, weight_decay) pairs); and a
small uint8 mask set with `get_sample_weights`' output for the dataset that serves it (mask = (png > 127) as float,
README.md:2022).

Usage:  python tests/golden/make_golden_focal.py [--reference /root/reference]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import load_reference_bcedice, load_reference_unet, to_t  # noqa: E402
from unet_lane_detection_amd.state import seeded_state_dict  # noqa: E402

README_DICELOSS_LINES = (1781, 1807)       # `class DiceLoss(nn.Module):` .. `return 1 - dice`
README_FOCAL_LINES = (1914, 1939)          # `class FocalLoss(nn.Module):` .. `return focal_loss.mean()`
README_SAMPLE_WEIGHTS_LINES = (2544, 2553)  # `def get_sample_weights(dataset):` .. `return weights`

FIXED = (30.0, 60.0, 87.0, 100.0, 120.0)
SMOOTH = 1e-6
#        name            wb   wf   wd   pw   alpha gamma  soft
CASES = (("focal_a25_g2", 0.0, 1.0, 0.0, 1.0, 0.25, 2.0, False),
         ("focal_a50_g1", 0.0, 1.0, 0.0, 1.0, 0.50, 1.0, False),
         ("focal_a75_g35", 0.0, 1.0, 0.0, 1.0, 0.75, 3.5, False),
         ("focal_a25_g0", 0.0, 1.0, 0.0, 1.0, 0.25, 0.0, False),
         ("focal_dice", 0.0, 0.5, 0.5, 3.0, 0.25, 2.0, False),
         ("combo", 0.3, 0.3, 0.4, 3.0, 0.25, 2.0, False),
         ("dice", 0.0, 0.0, 1.0, 1.0, 0.25, 2.0, False),
         ("soft", 0.0, 0.5, 0.5, 3.0, 0.25, 2.0, True))


def _block(ref_root, span, ns, name):
    with open(os.path.join(ref_root, "README.md"), encoding="utf-8") as f:
        lines = f.read().split("\n")
    lo, hi = span
    exec(compile("\n".join(lines[lo - 1:hi]), "reference:README.md", "exec"), ns)  # noqa: S102 - the reference oracle
    return ns[name]


def load_reference_losses(ref_root):
    ns = {"torch": torch, "nn": torch.nn, "F": torch.nn.functional}
    dice = _block(ref_root, README_DICELOSS_LINES, dict(ns), "DiceLoss")
    focal = _block(ref_root, README_FOCAL_LINES, dict(ns), "FocalLoss")
    return dice, load_reference_bcedice(ref_root), focal


def load_reference_sample_weights(ref_root):
    return _block(ref_root, README_SAMPLE_WEIGHTS_LINES, {}, "get_sample_weights")


class _AsDtype:
    """The classes call target.float(); in the float64 run that cast must keep float64 (the targets are float32
    numbers, so nothing else changes)."""

    def __init__(self, t, dtype):
        self.t, self.dtype = t.to(dtype), dtype

    def float(self):
        return self.t

    def view(self, *a):
        return _AsDtype(self.t.view(*a), self.dtype)

    def __rsub__(self, other):
        return other - self.t

    def __mul__(self, other):
        return self.t * other

    __rmul__ = __mul__


def reference_terms(classes, x_np, t_np, wb, wf, wd, pw, alpha, gamma, dtype):
    DiceLoss, BCEDiceLoss, FocalLoss = classes
    x = torch.from_numpy(x_np).to(dtype).requires_grad_(True)
    t = torch.from_numpy(t_np).to(dtype)
    tt = t if dtype == torch.float32 else _AsDtype(t, dtype)
    bd = BCEDiceLoss(bce_weight=wb, dice_weight=wd, pos_weight=torch.tensor([pw], dtype=dtype), smooth=SMOOTH)
    total_bd, bce, dice = bd(x, tt)
    focal = FocalLoss(alpha=alpha, gamma=gamma)(x, tt)
    assert bce.dtype == dtype and dice.dtype == dtype and focal.dtype == dtype, (bce.dtype, dice.dtype, focal.dtype)
    dice_alone = DiceLoss(smooth=SMOOTH)(x, tt)
    assert abs(dice_alone.item() - dice.item()) <= 1e-6 * (1 if dtype == torch.float32 else 1e-6)
    total = total_bd + wf * focal
    total.backward()
    return (np.array([total.item(), bce.item(), dice.item(), focal.item()], dtype=np.float64),
            x.grad.detach().numpy().astype(np.float64))


def make_focal(ref_root):
    classes = load_reference_losses(ref_root)
    out = {"cases": np.array([c[0] for c in CASES]).astype("U16")}
    for ci, (name, wb, wf, wd, pw, alpha, gamma, soft) in enumerate(CASES):
        rng = np.random.default_rng(100 + ci)
        x = np.concatenate([rng.standard_normal(2048) * s for s in (1.0, 4.0, 12.0)])
        t = (rng.random(x.size) < 0.085).astype(np.float64)
        fx = np.array([sgn * v for v in FIXED for sgn in (1.0, -1.0) for _ in (0, 1)])
        ft = np.array([tv for _ in FIXED for _ in (1.0, -1.0) for tv in (0.0, 1.0)])
        x = np.concatenate([x, fx]).astype(np.float32)
        t = np.concatenate([t, ft]).astype(np.float32)
        if soft:
            t = np.where(t > 0.5, np.float32(0.95), np.float32(0.05)).astype(np.float32)
        terms64, gx64 = reference_terms(classes, x, t, wb, wf, wd, pw, alpha, gamma, torch.float64)
        terms32, gx32 = reference_terms(classes, x, t, wb, wf, wd, pw, alpha, gamma, torch.float32)
        assert np.isfinite(gx64).all() and np.isfinite(terms64).all(), name
        out[f"{name}/x"], out[f"{name}/t"] = x, t
        out[f"{name}/params"] = np.array([wb, wf, wd, pw, alpha, gamma, SMOOTH], dtype=np.float64)
        out[f"{name}/terms64"], out[f"{name}/gx64"] = terms64, gx64
        out[f"{name}/terms32"], out[f"{name}/gx32"] = terms32, gx32.astype(np.float32)
        e32 = np.abs(gx32 - gx64).max()
        print(f"{name}: terms64 {terms64}, max|gx64| {np.abs(gx64).max():.3e}, E32 {e32:.3e} "
              f"({e32 / np.abs(gx64).max():.2e} of it), fp32 finite: {bool(np.isfinite(gx32).all())}")
    np.savez_compressed(os.path.join(HERE, "focal.npz"), **out)


class _MaskDataset:
    """What the reference's LaneDataset serves without a transform (README.md:2011-2030): (image, mask) with
    mask = (png > 127) as float32."""

    def __init__(self, masks_u8):
        self.masks = masks_u8

    def __len__(self):
        return len(self.masks)

    def __getitem__(self, idx):
        return None, torch.from_numpy((self.masks[idx] > 127).astype(np.float32)).unsqueeze(0)


def make_focal2(ref_root):
    UNet = load_reference_unet(ref_root)
    _, _, FocalLoss = classes = load_reference_losses(ref_root)
    DiceLoss = classes[0]
    feats = [4, 8]
    sd = seeded_state_dict(feats, seed=1)
    rng = np.random.default_rng(17)          # the inputs of tiny_f4_8_adamw2.npz
    xb = rng.standard_normal((4, 3, 32, 32)).astype(np.float32)
    tb = (rng.random((4, 1, 32, 32)) < 0.085).astype(np.float32)
    out = {"input": xb, "target": tb}
    for tag, lr, wd in (("ref", 1e-4, 1e-4), ("amp", 1e-2, 1e-1)):
        m = UNet(3, 1, features=feats)
        m.load_state_dict(to_t(sd), strict=True)
        m.train()
        opt = torch.optim.AdamW(m.parameters(), lr=lr, weight_decay=wd)
        focal_fn, dice_fn = FocalLoss(alpha=0.25, gamma=2.0), DiceLoss(smooth=SMOOTH)
        bce_fn = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([3.0]))   # reported only (weight 0)
        for step in range(2):
            opt.zero_grad()
            logits, t = m(torch.from_numpy(xb)), torch.from_numpy(tb)
            focal, dice = focal_fn(logits, t), dice_fn(logits, t)
            total = 0.5 * focal + 0.5 * dice
            total.backward()
            opt.step()
            out[f"{tag}/loss{step}"] = np.array([total.item(), bce_fn(logits, t).item(), dice.item(), focal.item()],
                                                dtype=np.float64)
        out[f"{tag}/lr"], out[f"{tag}/wd"] = np.float64(lr), np.float64(wd)
        for k, v in m.state_dict().items():
            out[f"{tag}/post/{k}"] = v.detach().numpy().copy()
    # mask set: lane ratios from empty to full, grey levels on both sides of the 127 / 128 border
    rng = np.random.default_rng(23)
    ratios = (0.0, 0.01, 0.05, 0.085, 0.15, 0.3, 0.5, 0.9, 1.0, 0.085, 0.02, 0.6)
    masks = np.zeros((len(ratios), 24, 40), dtype=np.uint8)
    for i, r in enumerate(ratios):
        lane = rng.random((24, 40)) < r if 0.0 < r < 1.0 else np.full((24, 40), r == 1.0)
        masks[i] = np.where(lane, rng.choice(np.array([128, 200, 255], dtype=np.uint8), size=(24, 40)),
                            rng.choice(np.array([0, 60, 127], dtype=np.uint8), size=(24, 40)))
    weights = load_reference_sample_weights(ref_root)(_MaskDataset(masks))
    out["masks_u8"] = masks
    out["sample_weights"] = np.asarray(weights, dtype=np.float64)
    out["positive_counts"] = (masks > 127).reshape(len(ratios), -1).sum(1).astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "tiny_f4_8_focal2.npz"), **out)
    print("focal2 golden written:", {k: out[k] for k in out if "loss" in k}, out["sample_weights"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    make_focal(args.reference)
    make_focal2(args.reference)


if __name__ == "__main__":
    main()
