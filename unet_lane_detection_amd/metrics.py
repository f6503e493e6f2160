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


# ---- multi-class: confusion matrix (include/unet_hip.h, unet_confusion_accumulate) ---------------------------------
class ClassLossSpec:
    """ce_weight * CrossEntropy(class_weights, ignore_index) + dice_weight * softmax Dice(smooth): the loss of a K-class
    trainer (unet_class_loss_config of include/unet_hip.h) as UNetTrainer.set_loss keeps it for the validation pass."""
    __slots__ = ("kind", "ce_weight", "dice_weight", "smooth", "class_weights", "ignore_index")

    def __init__(self, kind="ce", ce_weight=1.0, dice_weight=0.0, smooth=1.0, class_weights=None, ignore_index=None):
        self.kind = kind
        self.ce_weight, self.dice_weight, self.smooth = float(ce_weight), float(dice_weight), float(smooth)
        self.class_weights = None if class_weights is None else tuple(float(v) for v in class_weights)
        self.ignore_index = -1 if ignore_index is None else int(ignore_index)

    def to_c(self, classes):
        from . import _lib
        cw = self.class_weights if self.class_weights is not None else (1.0,) * classes
        if len(cw) != classes:
            raise ValueError(f"class_weights has {len(cw)} entries for {classes} classes")
        cfg = _lib.ClassLossConfig()
        cfg.ce_weight, cfg.dice_weight, cfg.smooth, cfg.ignore_index = self.ce_weight, self.dice_weight, self.smooth, self.ignore_index
        for k in range(_lib.UNET_MAX_CLASSES):
            cfg.class_weight[k] = cw[k] if k < classes else 0.0
        return cfg

    def __repr__(self):
        return "ClassLossSpec(%s)" % ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__)


def _ratio_array(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.where(den == 0, 1.0, num / np.where(den == 0, 1.0, den))


class ClassMetrics:
    """Metrics of a K-class validation pass from the pooled confusion counts (counts[t, p]: pixels of true class t
    predicted as p; pure numpy).  An empty denominator gives 1.0, as in SegMetrics.  The loss terms are means of the
    per-batch values."""

    def __init__(self, counts, loss_sums=(0.0, 0.0, 0.0), batches=0, invalid=0):
        c = np.asarray(counts)
        k = int(round(np.sqrt(c.size)))
        if k * k != c.size:
            raise ValueError("ClassMetrics takes K * K counts")
        self.counts = np.rint(c.astype(np.float64)).astype(np.int64).reshape(k, k)
        self.classes = k
        self.batches = int(batches)
        self.invalid = int(invalid)
        self._loss = tuple(float(v) for v in loss_sums)

    def _mean(self, i):
        return self._loss[i] / self.batches if self.batches else float("nan")

    @property
    def loss(self):
        return self._mean(0)

    @property
    def ce(self):
        return self._mean(1)

    @property
    def dice_loss(self):
        return self._mean(2)

    @property
    def pixels(self):
        return int(self.counts.sum())

    @property
    def iou(self):
        """per class: TP / (TP + FP + FN)"""
        tp = np.diag(self.counts)
        return _ratio_array(tp, self.counts.sum(0) + self.counts.sum(1) - tp)

    @property
    def class_dice(self):
        """per class: 2 TP / (2 TP + FP + FN)"""
        tp = np.diag(self.counts)
        return _ratio_array(2 * tp, self.counts.sum(0) + self.counts.sum(1))

    @property
    def miou(self):
        return float(self.iou.mean())

    @property
    def dice(self):
        """mean per-class Dice from the counts: what loop.fit picks its best model by"""
        return float(self.class_dice.mean())

    @property
    def pixel_acc(self):
        return _ratio(int(np.trace(self.counts)), int(self.counts.sum()))

    pixel_accuracy = pixel_acc

    def as_dict(self):
        return {"loss": self.loss, "ce": self.ce, "dice_loss": self.dice_loss, "dice": self.dice, "miou": self.miou,
                "iou": self.iou.tolist(), "pixel_acc": self.pixel_acc, "batches": self.batches, "pixels": self.pixels,
                "invalid": self.invalid}

    def __repr__(self):
        return "ClassMetrics(loss=%.6f, dice=%.6f, miou=%.6f, pixel_acc=%.6f, batches=%d, pixels=%d)" % (
            self.loss, self.dice, self.miou, self.pixel_acc, self.batches, self.pixels)


class ConfusionMatrix:
    """K x K confusion counts kept on the device: accumulate(pred, truth) adds one batch of uint8 label planes
    (unet_confusion_accumulate: integers, no host synchronisation); counts() reads them."""

    def __init__(self, classes, device=0, ignore_index=None):
        import torch

        from . import _lib
        if not 1 <= int(classes) <= _lib.UNET_MAX_CLASSES:
            raise ValueError(f"classes must be 1..{_lib.UNET_MAX_CLASSES}")
        self.classes = int(classes)
        self.ignore_index = -1 if ignore_index is None else int(ignore_index)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._lib = _lib.load()
        self.acc = torch.zeros(self.classes * self.classes, dtype=torch.int64, device=self.device)
        self._work = torch.empty(int(self._lib.unet_confusion_work_bytes()) // 4, dtype=torch.int32, device=self.device)

    def reset(self):
        self.acc.zero_()

    def accumulate(self, pred, truth):
        import torch

        from . import _lib
        if pred.dtype != torch.uint8 or truth.dtype != torch.uint8:
            raise ValueError("pred and truth must be uint8 label planes")
        pred, truth = pred.to(self.device).contiguous(), truth.to(self.device).contiguous()
        if pred.numel() != truth.numel():
            raise ValueError("pred and truth differ in size")
        _lib.call("unet_confusion_accumulate", self.device, pred, truth, pred.numel(), self.classes, self.ignore_index,
                  self.acc, self._work)

    def counts(self):
        return self.acc.cpu().numpy().reshape(self.classes, self.classes)

    def metrics(self):
        return ClassMetrics(self.counts())

    def iou(self):
        return self.metrics().iou

    def miou(self):
        return self.metrics().miou

    def pixel_accuracy(self):
        return self.metrics().pixel_acc


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
        rc = lib.unet_seg_metrics_accumulate_cfg(int(device_index), _lib.ptr(logits), _lib.ptr(targets), u8, logits.numel(),
                                                 _logit(threshold), C.byref(cfg), _lib.ptr(acc), stream)
        _lib.check(rc, "unet_seg_metrics_accumulate_cfg")
        return
    kind, bce_w, dice_w, pos_w, smooth = loss_cfg if loss_cfg else ("bce", 1.0, 0.0, 1.0, 1e-6)
    if kind == "bce":
        mode, bce_w, dice_w, pos_w = 0, 1.0, 0.0, 1.0
    else:
        mode = 1
    rc = lib.unet_seg_metrics_accumulate(int(device_index), _lib.ptr(logits), _lib.ptr(targets), u8, logits.numel(),
                                         _logit(threshold), mode, bce_w, dice_w, pos_w, smooth, _lib.ptr(acc), stream)
    _lib.check(rc, "unet_seg_metrics_accumulate")


# ---- threshold sweeps (include/unet_hip.h, unet_score_sweep_accumulate) ------------------------------------------
# The operating point is the one knob the reference exposes at every layer (`predict(image, threshold=0.5)`
# src/unet.py:74, the ROS parameter ~threshold, README.md:4503-4524, and the int8 model whose probabilities shift,
# README.md:3437).  One pass over scores and targets counts every element into (class, bin); the confusion counts at
# every threshold are sums over those.

DEFAULT_THRESHOLDS = tuple(round(0.05 * i, 2) for i in range(1, 20))      # 0.05, 0.10, ..., 0.95
SWEEP_MAX = 64          # UNET_SWEEP_MAX
DOMAINS = ("probability", "logit")


def sweep_model(scores, targets, thresholds):
    """The counting rule of unet_score_sweep_accumulate in numpy: counts[cls, bin] with bin = #{j : score > t_j} (a
    score equal to t_j is not above it, a NaN is above nothing) and cls = target != 0.  scores: float32 values in any
    domain; thresholds: ascending float32.  Returns int64 (2, T + 1)."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    c = (np.asarray(targets).reshape(-1) != 0).astype(np.int64)
    t = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    if s.size != c.size:
        raise ValueError("scores and targets differ in size")
    bins = np.zeros(s.size, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for tj in t:
            bins += s > tj
    return np.bincount(c * (t.size + 1) + bins, minlength=2 * (t.size + 1)).reshape(2, t.size + 1).astype(np.int64)


def _ratios(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.where(den == 0, 1.0, num / np.where(den == 0, 1.0, den))      # _ratio, element by element


class ThresholdSweep:
    """Confusion counts and the metrics of SegMetrics at every threshold of a sweep, from counts[2, T + 1] as
    sweep_model / unet_score_sweep_accumulate give them.  `thresholds` are the values the scores were compared with,
    in `domain` ("probability" or "logit"); `probabilities` are the probabilities they stand for (default: the
    thresholds themselves, or their sigmoid).  Predicted positive at t_j means bin > j, so tp and fp are suffix sums
    of the two rows and fn and tn prefix sums.  tp, fp, fn, tn are int64 arrays of length T; iou, f1 (= dice),
    precision, recall and pixel_accuracy float64 arrays with the empty-denominator convention of SegMetrics."""

    def __init__(self, thresholds, counts, domain="probability", probabilities=None):
        if domain not in DOMAINS:
            raise ValueError(f"domain={domain!r}: one of {DOMAINS}")
        t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        c = np.asarray(counts).astype(np.int64).reshape(2, -1)
        if t.size < 1 or c.shape[1] != t.size + 1:
            raise ValueError(f"{t.size} thresholds need counts of shape (2, {t.size + 1})")
        with np.errstate(invalid="ignore"):
            ascending = bool((np.diff(t) > 0).all())          # written so that a NaN or inf - inf refuses
        if np.isnan(t).any() or not ascending:
            raise ValueError("thresholds must be strictly ascending")
        self.domain = domain
        self.thresholds = t
        if probabilities is None:
            with np.errstate(over="ignore"):
                probabilities = t if domain == "probability" else 1.0 / (1.0 + np.exp(-t))
        self.probabilities = np.asarray(probabilities, dtype=np.float64).reshape(-1)
        if self.probabilities.size != t.size:
            raise ValueError("one probability per threshold")
        self.counts = c
        above = np.cumsum(c[:, ::-1], axis=1)[:, ::-1]        # above[:, b] = sum of bins >= b
        below = np.cumsum(c, axis=1)                          # below[:, b] = sum of bins <= b
        self.tp, self.fp = above[1, 1:].copy(), above[0, 1:].copy()
        self.fn, self.tn = below[1, :-1].copy(), below[0, :-1].copy()
        self.pixels = int(c.sum())

    def __len__(self):
        return self.thresholds.size

    @property
    def iou(self):
        return _ratios(self.tp, self.tp + self.fp + self.fn)

    @property
    def precision(self):
        return _ratios(self.tp, self.tp + self.fp)

    @property
    def recall(self):
        return _ratios(self.tp, self.tp + self.fn)

    @property
    def f1(self):
        return _ratios(2 * self.tp, 2 * self.tp + self.fp + self.fn)

    dice = f1

    @property
    def pixel_accuracy(self):
        return _ratios(self.tp + self.tn, self.tp + self.fp + self.fn + self.tn)

    METRICS = ("iou", "f1", "dice", "precision", "recall", "pixel_accuracy")

    def best(self, metric="f1"):
        """(threshold as a probability, value, index) of the threshold at which `metric` is largest.  Ties go to the
        threshold nearest 0.5 in probability, then to the lower one."""
        if metric not in self.METRICS:
            raise ValueError(f"metric={metric!r}: one of {self.METRICS}")
        v = getattr(self, metric)
        tied = np.flatnonzero(v == v.max())
        j = int(min(tied, key=lambda i: (abs(self.probabilities[i] - 0.5), self.probabilities[i])))
        return float(self.probabilities[j]), float(v[j]), j

    def index(self, threshold):
        """Position of `threshold` in the list: a probability of `probabilities`, or a value of `thresholds`; equal
        when both round to the same fp32 value, which is what the scores were compared with."""
        for arr in (self.probabilities, self.thresholds):
            hit = np.flatnonzero(arr.astype(np.float32) == np.float32(threshold))
            if hit.size:
                return int(hit[0])
        raise KeyError(f"threshold {threshold!r} is not in the sweep")

    def at(self, threshold):
        """What SegMetrics.as_dict reports from the pooled counts, at one threshold of the list."""
        j = self.index(threshold)
        out = {"threshold": float(self.probabilities[j])}
        for k in ("iou", "precision", "recall", "f1", "pixel_accuracy"):
            out[k] = float(getattr(self, k)[j])
        for k in ("tp", "fp", "fn", "tn"):
            out[k] = int(getattr(self, k)[j])
        out["pixels"] = self.pixels
        return out

    def __repr__(self):
        p, v, _ = self.best("f1")
        return f"ThresholdSweep({len(self)} thresholds, {self.domain}, pixels={self.pixels}, best f1={v:.6f} at {p:.4f})"


def sweep_thresholds(thresholds, domain="probability"):
    """The float32 array unet_score_sweep_accumulate compares with: the thresholds themselves, or (domain "logit") the
    logit of each probability as model._logit forms it, rounded to fp32 - what the existing metrics pass compares a
    logit with."""
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= t.size <= SWEEP_MAX:
        raise ValueError(f"a sweep takes 1 .. {SWEEP_MAX} thresholds, got {t.size}")
    if domain == "logit":
        from .model import _logit
        t = np.array([_logit(p) for p in t], dtype=np.float64)
    elif domain != "probability":
        raise ValueError(f"domain={domain!r}: one of {DOMAINS}")
    return np.ascontiguousarray(t.astype(np.float32))


def sweep_accumulate(lib, device_index, scores, targets, thresholds, counts, stream):
    """Add one batch to the device counters `counts` (2 * (T + 1) int64 on the scores' device, zeroed by the caller).
    scores: float32 device tensor in any domain; targets: float (positive iff != 0) or uint8 (positive iff non-zero)
    tensor of the same number of elements; thresholds: T ascending float32 values in the scores' domain (numpy)."""
    import ctypes as C

    import torch

    from . import _lib
    if targets.dtype == torch.uint8:
        targets, u8 = targets.to(scores.device).contiguous(), 1
    else:
        targets, u8 = targets.to(scores.device, torch.float32).contiguous(), 0
    if scores.dtype != torch.float32 or not scores.is_contiguous():
        raise ValueError("scores must be a contiguous float32 tensor")
    if scores.numel() != targets.numel():
        raise ValueError("scores and targets differ in size")
    t = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
    if counts.dtype != torch.int64 or counts.numel() != 2 * (t.size + 1) or counts.device != scores.device:
        raise ValueError(f"counts must be {2 * (t.size + 1)} int64 on the scores' device")
    rc = lib.unet_score_sweep_accumulate(int(device_index), _lib.ptr(scores), _lib.ptr(targets), u8, scores.numel(),
                                         t.ctypes.data_as(C.POINTER(C.c_float)), int(t.size), _lib.ptr(counts), stream)
    _lib.check(rc, "unet_score_sweep_accumulate")


def sweep_batches(lib, device, frames, targets, batch, thresholds, domain, stream_fn, score_fn):
    """Shared body of UNetHIP.sweep / UNetInt8.sweep / Ensemble.evaluate: score_fn(frames on the device) -> device
    scores in `domain`, counted batch by batch into one set of counters; 2 * (T + 1) integers are read at the end."""
    import torch
    frames, targets = torch.as_tensor(frames), torch.as_tensor(targets)
    n = int(frames.shape[0])
    if int(targets.shape[0]) != n:
        raise ValueError("frames and targets differ in their number of images")
    probs = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    t = sweep_thresholds(probs, domain)
    step = n if not batch else int(batch)
    counts = torch.zeros(2 * (t.size + 1), dtype=torch.int64, device=device)
    for i in range(0, n, step):
        scores = score_fn(frames[i:i + step].to(device).contiguous())
        sweep_accumulate(lib, device.index, scores, targets[i:i + step], t, counts, stream_fn())
    return ThresholdSweep(t, counts.cpu().numpy(), domain, probabilities=probs)


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


def evaluate_class_batches(device, classes, frames, labels, batch, ignore_index, labels_fn):
    """Shared body of UNetHIP.evaluate_classes / UNetInt8.evaluate_classes: labels_fn(frames on the device) -> device
    (N,H,W) uint8 argmax labels, counted batch by batch into one ConfusionMatrix on the device; the K * K counts are read
    once, at the end.  Returns ClassMetrics (per-class IoU, miou, pixel_acc: what UNetTrainer.validate reports from its
    matrix; the loss terms stay NaN, no loss is formed here)."""
    import torch
    frames, labels = torch.as_tensor(frames), torch.as_tensor(labels)
    n = int(frames.shape[0])
    if labels.dtype != torch.uint8:
        raise ValueError("labels must be uint8 label planes (N,H,W)")
    if int(labels.shape[0]) != n or labels.numel() != n * int(frames.shape[1]) * int(frames.shape[2]):
        raise ValueError("labels must be (N,H,W), one byte per pixel of the frames")
    step = n if not batch else int(batch)
    cm = ConfusionMatrix(classes, device, ignore_index)
    for i in range(0, n, step):
        cm.accumulate(labels_fn(frames[i:i + step].to(device).contiguous()), labels[i:i + step])
    return cm.metrics()
