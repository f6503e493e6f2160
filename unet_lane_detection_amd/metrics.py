"""Segmentation metrics of a validation pass (reference README.md:2087-2112 `validate`, :2115-2120 `compute_dice`,
:4177-4184 the published IoU / Dice / Precision / Recall / F1 / pixel accuracy).

`SegMetrics` is built from the 16 accumulators of `unet_seg_metrics_accumulate` (include/unet_hip.h) and is pure
Python / numpy: importable and usable without a GPU.  The loss terms and `dice` are means of per-batch values, as the
reference's loop averages them; IoU, precision, recall, F1 and pixel accuracy come from the confusion counts pooled over
the whole set.

Empty denominators: a ratio whose denominator is zero is 1.0 - nothing was there to find and nothing was claimed, the
value `compute_dice` tends to with its `smooth` term when prediction and truth are both empty.  (A zero denominator
implies a zero numerator for every ratio here, so there is no other case to decide.)  With no batch accumulated the
per-batch means are nan.
"""
from __future__ import annotations

import numpy as np

NUM_ACCUMULATORS = 16
TP, FP, FN, TN, LOSS, BCE, DICE_LOSS, DICE, BATCHES, PIXELS = range(10)
FOCAL = 10      # sum of the per-batch focal terms (unet_seg_metrics_accumulate_cfg, mode 2); 0 under the other modes


class LossSpec:
    """The general loss bce_weight * BCE(pos_weight) + focal_weight * Focal(alpha, gamma) + dice_weight * Dice(smooth)
    (mode 2 of include/unet_hip.h) as UNetTrainer.set_loss keeps it for the validation pass."""
    __slots__ = ("kind", "bce_weight", "focal_weight", "dice_weight", "pos_weight", "alpha", "gamma", "smooth")

    def __init__(self, kind, bce_weight, focal_weight, dice_weight, pos_weight, alpha, gamma, smooth):
        self.kind = kind
        self.bce_weight, self.focal_weight, self.dice_weight = float(bce_weight), float(focal_weight), float(dice_weight)
        self.pos_weight, self.alpha, self.gamma, self.smooth = float(pos_weight), float(alpha), float(gamma), float(smooth)

    def to_c(self):
        from . import _lib
        return _lib.LossConfig(2, self.bce_weight, self.focal_weight, self.dice_weight, self.pos_weight, self.alpha,
                               self.gamma, self.smooth)

    def __repr__(self):
        return "LossSpec(%s)" % ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__)


def _ratio(num, den):
    return 1.0 if den == 0 else float(num) / float(den)


class SegMetrics:
    def __init__(self, acc):
        a = np.asarray(acc, dtype=np.float64).reshape(-1)
        if a.size != NUM_ACCUMULATORS:
            raise ValueError(f"SegMetrics takes {NUM_ACCUMULATORS} accumulators, got {a.size}")
        self.acc = a.copy()
        self.tp, self.fp, self.fn, self.tn = (int(round(v)) for v in a[TP:TN + 1])
        self.batches = int(round(a[BATCHES]))
        self.pixels = int(round(a[PIXELS]))

    def _mean(self, i):
        return float(self.acc[i] / self.batches) if self.batches else float("nan")

    # ---- means of the per-batch values (reference README.md:2106-2110) ----
    @property
    def loss(self):
        return self._mean(LOSS)

    @property
    def bce(self):
        return self._mean(BCE)

    @property
    def dice_loss(self):
        return self._mean(DICE_LOSS)

    @property
    def focal(self):
        """Mean of the per-batch focal term (reference README.md:1914-1939); 0.0 for the losses that have none."""
        return self._mean(FOCAL)

    @property
    def dice(self):
        """Mean of the per-batch compute_dice: the reference's avg_dice."""
        return self._mean(DICE)

    # ---- from the pooled confusion counts ----
    @property
    def iou(self):
        return _ratio(self.tp, self.tp + self.fp + self.fn)

    @property
    def precision(self):
        return _ratio(self.tp, self.tp + self.fp)

    @property
    def recall(self):
        return _ratio(self.tp, self.tp + self.fn)

    @property
    def f1(self):
        return _ratio(2 * self.tp, 2 * self.tp + self.fp + self.fn)

    @property
    def pixel_accuracy(self):
        return _ratio(self.tp + self.tn, self.tp + self.fp + self.fn + self.tn)

    def as_dict(self):
        return {"loss": self.loss, "bce": self.bce, "dice_loss": self.dice_loss, "focal": self.focal, "dice": self.dice,
                "iou": self.iou,
                "precision": self.precision, "recall": self.recall, "f1": self.f1,
                "pixel_accuracy": self.pixel_accuracy, "tp": self.tp, "fp": self.fp, "fn": self.fn, "tn": self.tn,
                "batches": self.batches, "pixels": self.pixels}

    def __repr__(self):
        return ("SegMetrics(loss=%.6f, dice=%.6f, iou=%.6f, precision=%.6f, recall=%.6f, f1=%.6f, pixel_accuracy=%.6f, "
                "batches=%d, pixels=%d)" % (self.loss, self.dice, self.iou, self.precision, self.recall, self.f1,
                                            self.pixel_accuracy, self.batches, self.pixels))


def accumulate(lib, device_index, logits, targets, acc, stream, threshold=0.5, loss_cfg=None):
    """Add one batch to the device accumulators `acc` (16 float64 on the logits' device).  logits: float32 device
    tensor; targets: float (0/1) or uint8 (0 / non-zero) tensor of the same number of elements.  loss_cfg: what
    UNetTrainer.set_loss keeps - the 5-tuple of 'bce' / 'bce_dice' or the LossSpec of the general loss - or None for
    plain BCE-with-logits."""
    import ctypes as C

    import torch

    from . import _lib
    from .model import _logit
    if targets.dtype == torch.uint8:
        targets, u8 = targets.to(logits.device).contiguous(), 1
    else:
        targets, u8 = targets.to(logits.device, torch.float32).contiguous(), 0
    if logits.numel() != targets.numel():
        raise ValueError("logits and targets differ in size")
    if isinstance(loss_cfg, LossSpec):
        cfg = loss_cfg.to_c()
        rc = lib.unet_seg_metrics_accumulate_cfg(int(device_index), C.c_void_p(logits.data_ptr()),
                                                 C.c_void_p(targets.data_ptr()), u8, logits.numel(), _logit(threshold),
                                                 C.byref(cfg), C.c_void_p(acc.data_ptr()), stream)
        _lib.check(rc, "unet_seg_metrics_accumulate_cfg")
        return
    kind, bce_w, dice_w, pos_w, smooth = loss_cfg if loss_cfg else ("bce", 1.0, 0.0, 1.0, 1e-6)
    if kind == "bce":
        mode, bce_w, dice_w, pos_w = 0, 1.0, 0.0, 1.0
    else:
        mode = 1
    rc = lib.unet_seg_metrics_accumulate(int(device_index), C.c_void_p(logits.data_ptr()), C.c_void_p(targets.data_ptr()),
                                         u8, logits.numel(), _logit(threshold), mode, bce_w, dice_w, pos_w, smooth,
                                         C.c_void_p(acc.data_ptr()), stream)
    _lib.check(rc, "unet_seg_metrics_accumulate")


def evaluate_batches(lib, device, frames, targets, batch, threshold, stream_fn, forward_fn):
    """Shared body of UNetHIP.evaluate / UNetInt8.evaluate: forward_fn(frames on the device) -> device logits, reduced
    batch by batch into one accumulator; one host read at the end."""
    import torch
    frames, targets = torch.as_tensor(frames), torch.as_tensor(targets)
    n = int(frames.shape[0])
    if int(targets.shape[0]) != n:
        raise ValueError("frames and targets differ in their number of images")
    step = n if not batch else int(batch)
    acc = torch.zeros(NUM_ACCUMULATORS, dtype=torch.float64, device=device)
    for i in range(0, n, step):
        logits = forward_fn(frames[i:i + step].to(device).contiguous())
        accumulate(lib, device.index, logits, targets[i:i + step], acc, stream_fn(), threshold=threshold)
    return SegMetrics(acc.cpu().numpy())
