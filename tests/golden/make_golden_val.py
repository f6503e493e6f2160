#!/usr/bin/env python3
"""Generate tests/golden/tiny_f4_8_validate.npz from the REFERENCE's own validation function.

Runs only where the reference checkout is available.  Like make_golden.py it extracts code blocks of the reference's
README as text at run time - `UNet` (README.md:1418-1481), `BCEDiceLoss` (:1855-1893), `validate` and `compute_dice`
(:2087-2120) - executes them against torch-CPU and records numeric arrays only (allow_pickle=False).  No reference
source is written into this repository.

Fixture: tiny config features=[4, 8], 32 x 32, three batches of 2; weights = seeded_state_dict([4, 8], seed=1), the
weights of tiny_f4_8_eval.npz; criterion BCEDiceLoss(0.5, 0.5, pos_weight=3) as the training script builds it
(README.md:2169-2170).  Stored: the inputs, the uint8 0/255 masks, the logits, avg_loss / avg_dice as validate()
returns them and the per-batch values behind them.

The input seed is chosen so that NO pixel has |logit| < 1e-4: the thresholded prediction of every fp32 implementation
within 1e-4 of these logits is then the same, and the test that uses the fixture needs no tie allowance.

Usage:  python tests/golden/make_golden_val.py [--reference /root/reference]
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

README_VALIDATE_LINES = (2087, 2120)  # `def validate(model, dataloader, criterion, device, epoch):` .. compute_dice's return
TIE_BAND = 1e-4
FEATS, SIZE, BATCHES, BATCH = [4, 8], 32, 3, 2


def load_reference_validate(ref_root):
    with open(os.path.join(ref_root, "README.md"), encoding="utf-8") as f:
        lines = f.read().split("\n")
    lo, hi = README_VALIDATE_LINES
    # the loop wraps its loader in a progress bar: here the loader itself
    ns = {"torch": torch, "tqdm": lambda it, **kw: it}
    exec(compile("\n".join(lines[lo - 1:hi]), "reference:README.md", "exec"), ns)  # noqa: S102 - the reference oracle
    return ns["validate"], ns["compute_dice"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    torch.manual_seed(0)
    UNet = load_reference_unet(args.reference)
    BCEDiceLoss = load_reference_bcedice(args.reference)
    validate, compute_dice = load_reference_validate(args.reference)
    sd = seeded_state_dict(FEATS, seed=1)
    model = UNet(3, 1, features=FEATS)
    model.load_state_dict(to_t(sd), strict=True)
    crit = BCEDiceLoss(bce_weight=0.5, dice_weight=0.5, pos_weight=torch.tensor([3.0]))
    for seed in range(11, 11 + 64):
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((BATCHES * BATCH, 3, SIZE, SIZE)).astype(np.float32)
        mask = ((rng.random((BATCHES * BATCH, 1, SIZE, SIZE)) < 0.085) * 255).astype(np.uint8)
        model.eval()
        with torch.no_grad():
            logits = model(torch.from_numpy(x)).numpy()
        if np.abs(logits).min() >= TIE_BAND:
            break
        print(f"seed {seed}: a pixel with |logit| = {np.abs(logits).min():.2e} < {TIE_BAND:.0e}, next seed")
    else:
        raise SystemExit("no tie-free input among 64 seeds")
    assert np.abs(logits).min() >= TIE_BAND
    t = torch.from_numpy(mask.astype(np.float32) / 255.0)      # the dataset's mask / 255
    xs = torch.from_numpy(x)
    loader = [(xs[i:i + BATCH], t[i:i + BATCH]) for i in range(0, BATCHES * BATCH, BATCH)]
    avg_loss, avg_dice = validate(model, loader, crit, torch.device("cpu"), 1)
    per = []
    with torch.no_grad():
        for xb, tb in loader:
            out = model(xb)
            total, bce, dice = crit(out, tb)
            per.append((total.item(), bce.item(), dice.item(), compute_dice(torch.sigmoid(out) > 0.5, tb).item()))
    per = np.asarray(per, dtype=np.float64)
    assert abs(per[:, 0].mean() - avg_loss) < 1e-12 and abs(per[:, 3].mean() - avg_dice) < 1e-12
    np.savez_compressed(os.path.join(HERE, "tiny_f4_8_validate.npz"), input=x, mask_u8=mask, logits=logits,
                        avg_loss=np.float64(avg_loss), avg_dice=np.float64(avg_dice), batch_total=per[:, 0],
                        batch_bce=per[:, 1], batch_dice_loss=per[:, 2], batch_dice=per[:, 3],
                        input_seed=np.int64(seed), min_abs_logit=np.float64(np.abs(logits).min()))
    print(f"validate golden written: seed {seed}, min |logit| {np.abs(logits).min():.3e}, avg_loss {avg_loss:.6f}, "
          f"avg_dice {avg_dice:.6f}")


if __name__ == "__main__":
    main()
