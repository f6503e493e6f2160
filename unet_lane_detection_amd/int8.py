"""int8 tier of the deployed network ("model B": features [32, 64, 128], sigmoid head) on the HIP path
(SURVEY.md section 8 row f4).  Stands where the reference's quantised .rknn blob stands behind
`RKNN_model_container.run` (src/py_utils/rknn_executor.py:26-38): uint8 NHWC frames in, probabilities out.

  ranges = calibrate(float_model, frames)                  # device pass over calibration frames (README.md:3046-3078)
  ranges = calibrate(float_model, frames, algorithm="mmse")    # or "kl_divergence" (README.md:3407-3412): a second device
                                                           # pass takes histograms, the host chooses ranges from them
  qmodel = quant.quantize_model(state_dict, ranges)        # README.md:3106-3116 scheme, host arithmetic on weights
  net = UNetInt8(qmodel, device=0); net.run_u8(frames)
  compare_outputs(float_model, net, frames)                # float-vs-int8 MAE of probabilities (README.md:3512-3565)
  net.evaluate_classes(frames, labels)                     # K-class model: per-class IoU, mIoU, pixel accuracy of the tier
  units = choose_hybrid(float_model, state_dict, ranges, frames, k=3)      # not GOOD?  README.md:3466-3474, fourth remedy:
  qmodel = quant.quantize_model(state_dict, ranges, hybrid=units)          # those units in fp16 (hybrid quantisation)

A state dict whose output.weight has K = 2..8 rows gives a K-class quantised model (quantize_model emits the head's arrays
with K rows): every function here takes it, and UNetInt8.run_u8 then has UNetHIP.run_u8's K-class outputs.

All arithmetic on activations runs in libunet_hip.so (csrc/conv_i8.h, csrc/conv_h16.h, csrc/i8_classes_kernels.h); there is
no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, quant
from .metrics import DEFAULT_THRESHOLDS
from .model import _logit, _multi_class_only, _pack, _single_class_only


def calibrate(float_model, frames_u8, batch=8, algorithm="normal", bins=quant.HIST_BINS, return_histograms=False):
    """Per-tensor activation ranges of the float network over `frames_u8` ((N,H,W,3) uint8, host or device):
    {tensor name: (r_min, r_max)} for quant.quantize_model, by the reference's `quantized_algorithm`
    (README.md:3407-3412):

      "normal"          (min, max): the fp32 HIP tier with a min/max probe behind every layer
                        (unet_forward_u8_ranges; unet_forward_classes_u8_ranges for a K-class float model, whose
                        ranges are those of its body: the head's output carries none); frames are processed `batch`
                        at a time and the ranges merged;
      "mmse",           that pass first; its ranges, widened to contain 0, are the spans of a second pass over the same
      "kl_divergence"   frames with a histogram of `bins` bins behind every layer (unet_forward_u8_histograms).  The
                        histograms stay on the device across batches and are read once; quant.range_from_histogram
                        then chooses every tensor's range inside its (min, max).

    return_histograms: also return {tensor name: (uint64 histogram[bins + 1], lo, hi)} (quant.histogram_model's
    layout; None for "normal").  Raises ValueError when a tensor holds NaN."""
    if algorithm not in quant.ALGORITHMS:
        raise ValueError(f"algorithm={algorithm!r}: one of {quant.ALGORITHMS}")
    names = quant.tensor_names(len(float_model.features))
    frames = torch.as_tensor(frames_u8)
    normal = minmax_pass(float_model, frames, batch)
    if algorithm == "normal":
        return (normal, None) if return_histograms else normal
    for k in names:        # the order keys of the range pass put NaN beyond +-inf: it shows as a bound
        if not (np.isfinite(normal[k][0]) and np.isfinite(normal[k][1])):
            raise ValueError(f"calibrate: tensor {k!r} holds NaN or inf (range {normal[k]}); its range cannot be chosen")
    # a tensor that is 0 everywhere has no span to bin: it is counted over (0, 1) and keeps its (min, max)
    spans = np.array([(min(lo, 0.0), max(hi, 0.0)) for lo, hi in (normal[k] for k in names)], dtype=np.float32)
    dead = ~(spans[:, 1] > spans[:, 0])
    spans[dead] = (0.0, 1.0)
    hist_dev, elements = histogram_pass(float_model, frames, spans, bins, batch)
    hist = hist_dev.cpu().numpy().view(np.uint64)
    ranges, hists = {}, {}
    for i, name in enumerate(names):
        counted = int(hist[i].sum())
        if counted != int(elements[i]):
            raise ValueError(f"calibrate: tensor {name!r} holds {int(elements[i]) - counted} NaN of {int(elements[i])} "
                             "elements; its range cannot be chosen")
        lo, hi = float(spans[i, 0]), float(spans[i, 1])
        hists[name] = (hist[i].copy(), lo, hi)
        ranges[name] = normal[name] if dead[i] else quant.range_from_histogram(hist[i], lo, hi, algorithm)
    return (ranges, hists) if return_histograms else ranges


def _classes(model):
    return int(getattr(model, "out_channels", 1))


def minmax_pass(float_model, frames, batch=8):
    """{tensor name: (min, max)} over `frames`: the range pass of calibrate (one host read per batch)."""
    lib = _lib.load()
    h = float_model._h
    nt = int(lib.unet_num_range_tensors(h))
    names = quant.tensor_names(len(float_model.features))
    assert nt == len(names), (nt, names)
    lo = np.full(nt, np.inf)
    hi = np.full(nt, -np.inf)
    buf = (C.c_float * (2 * nt))()
    entry = "unet_forward_classes_u8_ranges" if _classes(float_model) > 1 else "unet_forward_u8_ranges"
    for i in range(0, frames.shape[0], batch):
        f = frames[i:i + batch].to(float_model.device).contiguous()
        n, hh, ww, _ = f.shape
        rc = getattr(lib, entry)(h, _lib.ptr(f), n, hh, ww, buf, _lib.stream(float_model.device))
        _lib.check(rc, entry, h)
        r = np.frombuffer(buf, dtype=np.float32).reshape(nt, 2)
        lo = np.minimum(lo, r[:, 0])
        hi = np.maximum(hi, r[:, 1])
    return {name: (float(lo[i]), float(hi[i])) for i, name in enumerate(names)}


def histogram_pass(float_model, frames, spans, bins=quant.HIST_BINS, batch=8):
    """The histogram pass of calibrate: every range tensor of the float network over `frames`, binned over its row of
    `spans` ((tensors, 2) float32: lo, hi).  Returns the (tensors, bins + 1) int64 device tensor of 64-bit counters,
    which stayed on the device across the batches and has not been waited for, and every tensor's element count."""
    lib = _lib.load()
    h = float_model._h
    nt = int(lib.unet_num_range_tensors(h))
    spans = np.ascontiguousarray(spans, dtype=np.float32)
    if spans.shape != (nt, 2):
        raise ValueError(f"spans must be ({nt}, 2)")
    hist_dev = torch.zeros((nt, bins + 1), dtype=torch.int64, device=float_model.device)
    elements = np.zeros(nt, dtype=np.int64)
    shapes = quant.tensor_shapes(float_model.features)
    entry = "unet_forward_classes_u8_histograms" if _classes(float_model) > 1 else "unet_forward_u8_histograms"
    for i in range(0, frames.shape[0], batch):
        f = frames[i:i + batch].to(float_model.device).contiguous()
        n, hh, ww, _ = f.shape
        rc = getattr(lib, entry)(h, _lib.ptr(f), n, hh, ww, spans.ctypes.data_as(C.c_void_p), int(bins),
                                 _lib.ptr(hist_dev), _lib.stream(float_model.device))
        _lib.check(rc, entry, h)
        elements += [n * (hh >> level) * (ww >> level) * c for c, level in shapes]
    return hist_dev, elements


class OutputComparison:
    """Per-frame mean absolute error between the probabilities of two tiers, with the reference's verdict on their mean
    (README.md:3553-3562): GOOD below 0.05, ACCEPTABLE below 0.10, POOR otherwise.  Pure numpy."""
    GOOD, ACCEPTABLE = 0.05, 0.10

    def __init__(self, per_frame):
        self.per_frame = np.asarray(per_frame, dtype=np.float64).reshape(-1).copy()
        if self.per_frame.size == 0:
            raise ValueError("OutputComparison needs at least one frame")
        self.mean = float(self.per_frame.mean())
        self.max = float(self.per_frame.max())

    @property
    def grade(self):
        return "GOOD" if self.mean < self.GOOD else "ACCEPTABLE" if self.mean < self.ACCEPTABLE else "POOR"

    def __repr__(self):
        return "OutputComparison(frames=%d, mean=%.6f, max=%.6f, grade=%s)" % (self.per_frame.size, self.mean, self.max,
                                                                             self.grade)


def prob_mae(probs_a, probs_b):
    """Per-frame sum of |a - b| over two (N, ...) float32 device tensors divided by the frame size, as a float64 device
    tensor (unet_prob_mae_accumulate: the sums are formed on the device)."""
    if probs_a.shape != probs_b.shape or probs_a.dtype != torch.float32 or probs_b.dtype != torch.float32:
        raise ValueError("prob_mae takes two float32 tensors of one shape")
    if probs_a.device != probs_b.device or probs_a.device.type != "cuda":
        raise ValueError("prob_mae takes two tensors on one HIP device")
    a, b = probs_a.contiguous(), probs_b.contiguous()
    n = int(a.shape[0])
    acc = torch.zeros(n, dtype=torch.float64, device=a.device)
    _lib.call("unet_prob_mae_accumulate", a.device, a, b, n, a.numel() // n, acc)
    return acc / (a.numel() // n)


def compare_outputs(float_model, int8_net, frames_u8, batch=8):
    """The reference's `compare_outputs` (README.md:3512-3565): per-frame MAE between the probabilities of the float
    tier (fp32) and of the int8 tier over `frames_u8` ((N,H,W,3) uint8).  The probabilities stay on the device, where
    each frame's |difference| is summed in float64; one number per frame is read.  Returns OutputComparison.  Two K-class
    models are compared on their softmax tensors: the mean runs over the K * H * W probabilities of a frame."""
    frames = torch.as_tensor(frames_u8)
    if float_model.device != int8_net.device:
        raise ValueError("compare_outputs needs both tiers on one device")
    if _classes(float_model) != _classes(int8_net):
        raise ValueError(f"compare_outputs: the float model has {_classes(float_model)} class(es), the int8 model "
                         f"{_classes(int8_net)}")
    out = []
    for i in range(0, frames.shape[0], batch):
        f = frames[i:i + batch].to(float_model.device).contiguous()
        pf = float_model.run_u8(f, return_probs=True)[1]
        pq = int8_net.run_u8(f, return_probs=True)[1]
        out.append(prob_mae(pf, pq))
    return OutputComparison(torch.cat(out).cpu().numpy())


def _mae_of(float_model, qmodel, frames_u8, batch):
    net = UNetInt8(qmodel, device=float_model.device.index)
    try:
        return compare_outputs(float_model, net, frames_u8, batch=batch).mean
    finally:
        net.release()


def sensitivity(float_model, state_dict, ranges, frames_u8, batch=8):
    """Which units are worth running in fp16 (hybrid quantisation, quant.py): the pure-int8 model and, per unit of
    quant.unit_names, the model with only that unit hybrid, each compared with the fp32 tier by compare_outputs over
    `frames_u8`.  Returns [(unit, mae_hybrid_this_unit, mae_int8)], the largest gain (mae_int8 - mae_hybrid) first.
    Everything runs on the device; one number per frame is read back."""
    frames = torch.as_tensor(frames_u8)
    base = _mae_of(float_model, quant.quantize_model(state_dict, ranges), frames, batch)
    rows = [(u, _mae_of(float_model, quant.quantize_model(state_dict, ranges, hybrid=(u,)), frames, batch), base)
            for u in quant.unit_names(float_model.features)]
    return sorted(rows, key=lambda r: r[1])          # stable: ties keep forward order


def choose_hybrid(float_model, state_dict, ranges, frames_u8, k, batch=8):
    """The `k` units to name in quantize_model(hybrid=...), chosen greedily: each pick is the unit that, added to the
    ones already picked, gives the smallest compare_outputs error; every candidate is re-measured after each pick (a
    tensor between two hybrid units becomes fp16, so gains do not add up)."""
    frames = torch.as_tensor(frames_u8)
    units = quant.unit_names(float_model.features)
    if not 0 <= k <= len(units):
        raise ValueError(f"k={k}: the model has {len(units)} units")
    chosen = []
    for _ in range(k):
        rest = [u for u in units if u not in chosen]
        maes = [_mae_of(float_model, quant.quantize_model(state_dict, ranges, hybrid=chosen + [u]), frames, batch)
                for u in rest]
        chosen.append(rest[int(np.argmin(maes))])
    return chosen


class UNetInt8:
    """Quantised U-Net forward on one MI355X (i8 MFMA; the units a model marks hybrid on f16 MFMA, csrc/conv_h16.h).
    hybrid=False runs a model with hybrid units as pure int8.  out_channels: 1, or the K classes of a model whose head
    arrays have K rows (csrc/i8_classes_kernels.h)."""

    def __init__(self, qmodel, device=0, hybrid=True):
        if not torch.cuda.is_available():
            raise RuntimeError("UNetInt8 needs a HIP device; there is no CPU fallback")
        self._lib = _lib.load()
        self.features = [int(f) for f in qmodel["features"]]
        self.device = torch.device("cuda", int(device))
        feats = (C.c_int * len(self.features))(*self.features)
        h = C.c_void_p()
        _lib.check(self._lib.unet_i8_create(len(self.features), feats, int(device), C.byref(h)), "unet_i8_create")
        self._h = h
        self.multiple = 1 << len(self.features)
        for k, v in qmodel.items():
            if k == "features":
                continue
            a = np.ascontiguousarray(np.asarray(v))
            if a.dtype == np.float64:
                a = a.astype(np.float32)
            if a.dtype == np.int64:
                a = a.astype(np.int32)
            self._check(self._lib.unet_i8_load(h, k.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes), f"unet_i8_load({k})")
        self._check(self._lib.unet_i8_set_hybrid(h, 1 if hybrid else 0), "unet_i8_set_hybrid")
        self._check(self._lib.unet_i8_finalize(h), "unet_i8_finalize")
        self.out_channels = int(self._lib.unet_i8_out_channels(h))

    @classmethod
    def from_file(cls, path, device=0, hybrid=True):
        return cls(quant.load_quantized(path), device=device, hybrid=hybrid)

    def tensor_dtype(self, name):
        """'int8' or 'fp16': how activation tensor `name` is stored (quant.tensor_dtypes states the rule)."""
        self._require_live()
        rc = int(self._lib.unet_i8_tensor_dtype(self._h, name.encode()))
        if rc not in (0, 1):
            raise KeyError(name)
        return "fp16" if rc else "int8"

    def _check(self, rc, where):
        if rc != 0:
            msg = self._lib.unet_i8_last_error(self._h)
            raise _lib.UnetError(rc, where, msg.decode() if msg else "")

    def _require_live(self):
        if self._h is None:
            raise RuntimeError("UNetInt8 has been released")

    def run_u8(self, frames, return_probs=False, return_mask=False, threshold=0.5, return_labels=False, mask_class=None):
        """frames: (N,H,W,3) uint8 RGB on this device -> logits (N,1,H,W) float32 [, probabilities, mask].
        A K-class model returns, as UNetHIP.run_u8 and in its order, logits (N,K,H,W) [, softmax (N,K,H,W)] [, labels
        (N,H,W) uint8 = argmax] [, the (N,H,W) uint8 plane that is 255 where the label is mask_class]; return_mask and
        threshold belong to the single-class head, return_labels and mask_class to a K-class model."""
        self._require_live()
        if self.out_channels > 1:
            _single_class_only(return_mask, "return_mask")
            _single_class_only(threshold != 0.5, "threshold")
            if mask_class is not None and not 0 <= int(mask_class) < self.out_channels:
                raise ValueError(f"mask_class={mask_class!r}: the model has classes 0..{self.out_channels - 1}")
        else:
            _multi_class_only(return_labels, mask_class)
        if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise ValueError("frames must be (N,H,W,3) uint8")
        frames = frames.to(self.device).contiguous()
        n, h, w, _ = frames.shape
        if self.out_channels > 1:
            return self._run_classes(frames, n, h, w, True, return_probs, return_labels, mask_class)
        logits = torch.empty((n, 1, h, w), dtype=torch.float32, device=self.device)
        probs = torch.empty_like(logits) if return_probs else None
        mask = torch.empty((n, h, w), dtype=torch.uint8, device=self.device) if return_mask else None
        p = _lib.ptr
        rc = self._lib.unet_i8_forward_u8(self._h, p(frames), n, h, w, p(logits), p(probs), p(mask), _logit(threshold),
                                          _lib.stream(self.device))
        self._check(rc, "unet_i8_forward_u8")
        return _pack(logits, probs, mask, return_probs, return_mask)

    def _run_classes(self, frames, n, h, w, want_logits, want_probs, want_labels, mask_class):
        """unet_i8_forward_classes_u8 with the outputs asked for: the tensors in the order logits, probs, labels, mask"""
        k = self.out_channels
        logits = torch.empty((n, k, h, w), dtype=torch.float32, device=self.device) if want_logits else None
        probs = torch.empty((n, k, h, w), dtype=torch.float32, device=self.device) if want_probs else None
        labels = torch.empty((n, h, w), dtype=torch.uint8, device=self.device) if want_labels else None
        mask = torch.empty((n, h, w), dtype=torch.uint8, device=self.device) if mask_class is not None else None
        p = _lib.ptr
        rc = self._lib.unet_i8_forward_classes_u8(self._h, p(frames), n, h, w, p(logits), p(probs), p(labels),
                                                  int(mask_class) if mask_class is not None else 0, p(mask),
                                                  _lib.stream(self.device))
        self._check(rc, "unet_i8_forward_classes_u8")
        out = [t for t in (logits, probs, labels, mask) if t is not None]
        return out[0] if len(out) == 1 else tuple(out)

    def predict_labels(self, frames):
        """frames: (N,H,W,3) uint8 RGB -> (N,H,W) uint8 labels of a K-class model and nothing else: the head writes one
        byte per pixel (the deployment form; run_u8 always returns the logits as well)."""
        self._require_live()
        if self.out_channels < 2:
            _multi_class_only(True, None)
        if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise ValueError("frames must be (N,H,W,3) uint8")
        frames = frames.to(self.device).contiguous()
        n, h, w, _ = frames.shape
        return self._run_classes(frames, n, h, w, False, False, True, None)

    def evaluate_classes(self, frames, labels_u8, batch=None, ignore_index=None):
        """Per-class IoU, miou and pixel_acc (metrics.ClassMetrics) of the K-class int8 tier over uint8 `frames` against
        `labels_u8` (N,H,W) uint8: as UNetHIP.evaluate_classes."""
        from . import metrics
        self._require_live()
        if self.out_channels < 2:
            _multi_class_only(True, None)
        return metrics.evaluate_class_batches(self.device, self.out_channels, frames, labels_u8, batch, ignore_index,
                                              self.predict_labels)

    def evaluate(self, frames, targets, threshold=0.5, batch=None):
        """Segmentation metrics of the int8 tier over uint8 `frames` against `targets`: as UNetHIP.evaluate."""
        from . import metrics
        self._require_live()
        return metrics.evaluate_batches(self._lib, self.device, frames, targets, batch, threshold,
                                        lambda: _lib.stream(self.device),
                                        self.run_u8)

    def sweep(self, frames, targets, thresholds=DEFAULT_THRESHOLDS, batch=None):
        """Confusion counts and metrics of the int8 tier at every threshold of `thresholds` in one forward of the set:
        as UNetHIP.sweep.  `.best()` is the operating point of this quantised model (its probabilities shift against
        the float model's, reference README.md:3437)."""
        from . import metrics
        self._require_live()
        return metrics.sweep_batches(self._lib, self.device, frames, targets, batch, thresholds, "logit",
                                     lambda: _lib.stream(self.device),
                                     self.run_u8)

    def read_tensor(self, name, n, h, w):
        """Activation tensor `name` of the last forward as an (N,C,h,w) numpy array (parity tests); h, w are that
        tensor's spatial size.  int8 for an int8 tensor, float32 (the stored fp16 values) for an fp16 tensor of a
        hybrid model."""
        self._require_live()
        if name != "im2col" and self.tensor_dtype(name) == "fp16":
            cap = n * h * w * 512 * 2
            buf = np.empty(cap // 2, dtype=np.float16)
            c = C.c_int()
            self._check(self._lib.unet_i8_read_tensor_f16(self._h, name.encode(), buf.ctypes.data_as(C.c_void_p), cap,
                                                          C.byref(c)), f"unet_i8_read_tensor_f16({name})")
            return buf[:n * h * w * c.value].reshape(n, h, w, c.value).transpose(0, 3, 1, 2).astype(np.float32)
        cap = n * h * w * 512
        buf = np.empty(cap, dtype=np.int8)
        c = C.c_int()
        self._check(self._lib.unet_i8_read_tensor(self._h, name.encode(), buf.ctypes.data_as(C.c_void_p), cap, C.byref(c)),
                    f"unet_i8_read_tensor({name})")
        return buf[:n * h * w * c.value].reshape(n, h, w, c.value).transpose(0, 3, 1, 2).copy()

    def release(self):
        if getattr(self, "_h", None) is not None:
            torch.cuda.synchronize(self.device)
            self._lib.unet_i8_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
