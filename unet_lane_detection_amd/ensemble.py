"""Checkpoint ensembles: the reference's `ensemble_predict` ("model ensembling", README.md:2623-2647) on the device.

The reference loads the checkpoints its training loop wrote (best_model.pth, epoch_80.pth, epoch_100.pth), runs each on
the frame and returns `torch.stack([sigmoid(m(x)) for m in models]).mean(0) > 0.5`.  Here every member runs its own
forward on torch's current stream and writes its probabilities from its head; one kernel (`unet_ensemble_combine`,
include/unet_hip.h) then forms the weighted mean and the mask.  Nothing touches the host.

  ens = Ensemble.from_checkpoints(["best_model.pth", "epoch_80.pth", "epoch_100.pth"])
  probs, mask = ens.run_u8(frames, return_mask=True)          # (N,1,H,W) float32, (N,H,W) uint8 0 / 255
  sweep = ens.evaluate(frames, targets)                       # metrics.ThresholdSweep over the mean probabilities
  video.FramePipeline(ens).process(frames_bgr)                # an ensemble stands where a model stands

The arithmetic of the mean is a contract that `combine_model` states in numpy float32, bit for bit:
    acc = w[0] * p0;   acc = acc + w[k] * pk   for k = 1 .. K-1, in that order,
every product and every sum rounded to fp32 on its own.  The inputs are probabilities and not logits on purpose: every
tier already writes them (the int8 tier's included), so the kernel repeats nobody's exponential and is exact against
this model.  Note that K equal inputs do not always average to themselves under this arithmetic.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .metrics import DEFAULT_THRESHOLDS

ENSEMBLE_MAX = 8        # UNET_ENSEMBLE_MAX


def normalise_weights(weights, k):
    """K fp32 weights that sum to 1 up to rounding: normalised in float64, then rounded to fp32.  None: equal weights,
    (float32)(1 / K) each - what the library uses for a NULL weight array."""
    if weights is None:
        return np.full(k, np.float32(1.0 / k), dtype=np.float32)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size != k:
        raise ValueError(f"{k} members need {k} weights, got {w.size}")
    if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError("weights must be finite, not negative and not all zero")
    return (w / w.sum()).astype(np.float32)


def combine_model(probs_list, weights=None, threshold=0.5):
    """The arithmetic of unet_ensemble_combine in numpy float32: (probs, mask).  weights: K fp32 values used as they
    are (None: (float32)(1 / K) each); mask = 255 where probs > threshold, else 0 (a NaN gives 0)."""
    ps = [np.asarray(p, dtype=np.float32) for p in probs_list]
    if not 1 <= len(ps) <= ENSEMBLE_MAX:
        raise ValueError(f"an ensemble has 1 .. {ENSEMBLE_MAX} members, got {len(ps)}")
    w = normalise_weights(None, len(ps)) if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
    if w.size != len(ps):
        raise ValueError(f"{len(ps)} members need {len(ps)} weights, got {w.size}")
    with np.errstate(invalid="ignore", under="ignore"):
        acc = (w[0] * ps[0]).astype(np.float32)
        for k in range(1, len(ps)):
            acc = (acc + (w[k] * ps[k]).astype(np.float32)).astype(np.float32)
        mask = np.where(acc > np.float32(threshold), 255, 0).astype(np.uint8)
    return acc, mask


def combine(probs_list, weights=None, threshold=0.5, return_probs=True, return_mask=False):
    """unet_ensemble_combine on K float32 device tensors of one shape, on torch's current stream: the weighted mean
    (shaped like the inputs) and / or the uint8 mask (0 / 255), as asked for.  weights: K fp32 values used as they are,
    or None for equal weights."""
    import torch

    from . import _lib
    ps = list(probs_list)
    k = len(ps)
    if not 1 <= k <= ENSEMBLE_MAX:
        raise ValueError(f"an ensemble has 1 .. {ENSEMBLE_MAX} members, got {k}")
    if not (return_probs or return_mask):
        raise ValueError("nothing asked for")
    dev, shape = ps[0].device, ps[0].shape
    for p in ps:
        if p.dtype != torch.float32 or p.device != dev or p.shape != shape or not p.is_contiguous():
            raise ValueError("the members' probabilities must be contiguous float32 tensors of one shape on one device")
    ptrs = (C.c_void_p * k)(*[p.data_ptr() for p in ps])
    w = None
    if weights is not None:
        wa = np.asarray(weights, dtype=np.float32).reshape(-1)
        if wa.size != k:
            raise ValueError(f"{k} members need {k} weights, got {wa.size}")
        w = (C.c_float * k)(*[float(v) for v in wa])
    out = torch.empty(shape, dtype=torch.float32, device=dev) if return_probs else None
    mask = torch.empty(shape, dtype=torch.uint8, device=dev) if return_mask else None
    _lib.call("unet_ensemble_combine", dev, ptrs, k, w, ps[0].numel(), float(threshold), out, mask)
    if return_probs and return_mask:
        return out, mask
    return out if return_probs else mask


class Ensemble:
    """Several models as one.  members: each a `UNetHIP` (run on the tier "f16x3"), a `(UNetHIP, precision)` pair or a
    `UNetInt8`, all on one device, 1 .. 8 of them.  weights: one per member, not negative; they are normalised on the
    host in float64 and rounded to fp32 (None: equal weights).

    `run_u8` has no `precision` argument, each member keeps its own tier: `video.FramePipeline(Ensemble(...))`
    therefore takes the path it has for a `UNetInt8`.  On that path the pipeline does not poll `device_error`; a
    caller with f16x3 members calls `Ensemble.device_error` per chunk and re-runs the chunk with those members on
    "fp32" after a range report."""

    def __init__(self, members, weights=None):
        from .int8 import UNetInt8
        from .model import UNetHIP
        parsed = []
        for m in members:
            if isinstance(m, UNetHIP):
                parsed.append((m, "f16x3"))
            elif isinstance(m, UNetInt8):
                parsed.append((m, None))
            elif isinstance(m, (tuple, list)) and len(m) == 2 and isinstance(m[0], UNetHIP):
                if m[1] not in UNetHIP.PRECISIONS:
                    raise ValueError(f"precision={m[1]!r}: one of {UNetHIP.PRECISIONS}")
                parsed.append((m[0], m[1]))
            else:
                raise TypeError("a member is a UNetHIP, a (UNetHIP, precision) pair or a UNetInt8")
        if not 1 <= len(parsed) <= ENSEMBLE_MAX:
            raise ValueError(f"an ensemble has 1 .. {ENSEMBLE_MAX} members, got {len(parsed)}")
        self.device = parsed[0][0].device
        if any(m.device != self.device for m, _ in parsed):
            raise ValueError("all members of an ensemble must be on one device")
        self.members = parsed
        self.multiple = max(m.multiple for m, _ in parsed)
        self.weights = normalise_weights(weights, len(parsed))
        self._equal = weights is None
        self._owned = []

    @classmethod
    def from_checkpoints(cls, paths, device=0, precision="f16x3", weights=None):
        """One `UNetHIP.from_checkpoint` per path (the files the reference's `ensemble_predict` names are what its
        training loop saves, README.md:2208-2213), each run on the tier `precision`.  The ensemble owns these models:
        `release` frees them."""
        from .model import UNetHIP
        models = []
        try:
            for p in paths:
                models.append(UNetHIP.from_checkpoint(p, device=device))
            ens = cls([(m, precision) for m in models], weights=weights)
        except Exception:
            for m in models:
                m.release()
            raise
        ens._owned = models
        return ens

    def __len__(self):
        return len(self.members)

    # ---- forward ---------------------------------------------------------------------------------------------------
    def _combine(self, probs, return_mask, threshold):
        out = combine(probs, None if self._equal else self.weights, threshold, True, return_mask)
        if not return_mask:
            return out
        return out[0], out[1].view(out[1].shape[0], out[1].shape[2], out[1].shape[3])

    def run_u8(self, frames, return_mask=False, threshold=0.5):
        """frames: (N,H,W,3) uint8 RGB -> the ensemble's probabilities (N,1,H,W) float32, or with return_mask
        (probabilities, mask (N,H,W) uint8 holding 0 / 255, mean > threshold).  Every member's forward and the
        combining kernel are enqueued on torch's current stream; nothing is read back."""
        import torch
        frames = torch.as_tensor(frames)
        if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise ValueError("frames must be (N,H,W,3) uint8")
        frames = frames.to(self.device).contiguous()
        probs = [m.run_u8(frames, return_probs=True)[1] if prec is None
                 else m.run_u8(frames, return_probs=True, precision=prec)[1] for m, prec in self.members]
        return self._combine(probs, return_mask, threshold)

    def forward(self, image, return_mask=False, threshold=0.5):
        """image: (N,3,H,W) float32, already normalised -> as run_u8.  `UNetHIP` members only, on "fp32" or "f16x3"."""
        from .model import UNetHIP
        if any(not isinstance(m, UNetHIP) for m, _ in self.members):
            raise TypeError("Ensemble.forward takes float input, which a UNetInt8 member has no entry for; use run_u8")
        probs = [m.forward(image, return_probs=True, precision=prec)[1] for m, prec in self.members]
        return self._combine(probs, return_mask, threshold)

    __call__ = forward

    # ---- metrics ---------------------------------------------------------------------------------------------------
    def evaluate(self, frames, targets, thresholds=DEFAULT_THRESHOLDS, batch=None):
        """Confusion counts and metrics of the ensemble at every threshold of `thresholds` (probabilities, ascending)
        over `frames` ((N,H,W,3) uint8, or (N,3,H,W) float32 for `UNetHIP` members) against `targets` ((N,1,H,W) or
        (N,H,W), float 0/1 or uint8 0 / non-zero), `batch` frames at a time.  The mean probabilities stay on the device
        and are counted there (unet_score_sweep_accumulate); 2 * (T + 1) integers are read at the end.  Returns
        metrics.ThresholdSweep in the probability domain."""
        import torch

        from . import _lib, metrics
        return metrics.sweep_batches(_lib.load(), self.device, frames, targets, batch, thresholds, "probability",
                                     lambda: _lib.stream(self.device),
                                     lambda f: self.run_u8(f) if f.dtype == torch.uint8 else self.forward(f))

    # ---- status and lifetime ---------------------------------------------------------------------------------------
    def device_error(self, current_stream_only=False):
        """The first non-zero `UNetHIP.device_error` of the members (every `UNetHIP` member is asked, so every
        member's record is cleared); 0 if none reports.  A `UNetInt8` member has no such record."""
        from .model import UNetHIP
        first = 0
        for m, _ in self.members:
            if isinstance(m, UNetHIP):
                rc = m.device_error(current_stream_only=current_stream_only)
                first = first or rc
        return first

    def release(self):
        """Release the members this ensemble created (from_checkpoints); members handed in stay the caller's."""
        for m in self._owned:
            m.release()
        self._owned = []
