"""Training step on the HIP path: train-mode forward, BCE-with-logits, backward, Adam
(reference README.md:2060-2084, :1694-1709, :2173), with an optional data-parallel gradient
all-reduce between backward and the optimizer.  All arithmetic runs in libunet_hip.so; torch
provides the flat device buffers and torch.distributed (RCCL) the collective."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, checkpoint, dp, loop, metrics
from .model import infer_features, infer_out_channels
from .state import INPUT_MEAN, INPUT_STD


class UNetTrainer:
    STATUS_PAD = 4    # floats in front of the gradients in the all-reduce bucket (keeps them 16-byte aligned)

    def __init__(self, state_dict, device=0, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 decoupled=False, process_group=None, in_channels=3, overlap_allreduce=False,
                 check_device_status=True, accum_steps=1, max_grad_norm=None, skip_nonfinite=False):
        """accum_steps, max_grad_norm and skip_nonfinite (also plain attributes, changeable between updates): see
        step().  With the three defaults step, forward_backward and optimizer_step launch and allocate exactly what they
        did before these keywords existed."""
        if not torch.cuda.is_available():
            raise RuntimeError("UNetTrainer needs a HIP device; there is no CPU fallback")
        self._lib = _lib.load()
        self.features = infer_features(state_dict)
        self.out_channels = infer_out_channels(state_dict)   # 1: the lane head; K > 1: classes, labels, the class loss
        self.device = torch.device("cuda", int(device))
        cfg = _lib.UnetConfig()
        cfg.in_channels, cfg.out_channels, cfg.depth = in_channels, self.out_channels, len(self.features)
        for i, f in enumerate(self.features):
            cfg.features[i] = f
        cfg.device = int(device)
        for i in range(3):
            cfg.input_mean[i], cfg.input_std[i] = INPUT_MEAN[i], INPUT_STD[i]
        h = C.c_void_p()
        _lib.check(self._lib.unet_create(C.byref(cfg), C.byref(h)), "unet_create")
        self._h = h
        self.lr, self.betas, self.eps = lr, betas, eps
        self.weight_decay, self.decoupled = weight_decay, decoupled
        self.group = process_group
        self.step_count = 0
        self.overlap = bool(overlap_allreduce)
        self.check_device_status = bool(check_device_status)
        self._comm = None
        self._split = 0
        self._fb_rc = 0
        self._defer_fb_error = False
        # gradient accumulation, global-norm clipping, non-finite guard: nothing is allocated until one of them is used
        self.accum_steps = int(accum_steps)
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self.grad_norm = float("nan")     # scaled pre-clip norm of the last update (read only on the checked path)
        self.skipped_steps = 0
        self._pending = 0                 # micro-batches in the accumulation buffer
        self._latched_rc = 0              # several ranks: a micro-step's entry failure, held until the exchange
        self._acc = None
        self._grad_rec = None
        self._grad_work = None
        self._rec_host = None

        # flat buffers in unet_param_name order
        n = self._lib.unet_num_params(h)
        self.layout = []   # (name, is_buffer, offset, numel)
        for i in range(n):
            isb, off = C.c_int(), C.c_size_t()
            _lib.check(self._lib.unet_train_layout(h, i, C.byref(isb), C.byref(off)), "unet_train_layout", h)
            self.layout.append((self._lib.unet_param_name(h, i).decode(), bool(isb.value), int(off.value),
                                int(self._lib.unet_param_numel(h, i))))
        P = int(self._lib.unet_train_param_numel(h))
        B = int(self._lib.unet_train_buffer_numel(h))
        host_p = np.empty(P, dtype=np.float32)
        host_b = np.empty(B, dtype=np.float32)
        self._shapes = {}
        for name, isb, off, numel in self.layout:
            v = state_dict[name]
            v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            assert v.size == numel, (name, v.shape, numel)
            self._shapes[name] = tuple(v.shape)
            (host_b if isb else host_p)[off:off + numel] = v.astype(np.float32).reshape(-1)
        self.params = torch.from_numpy(host_p).to(self.device)
        self.bn = torch.from_numpy(host_b).to(self.device)
        # The all-reduce bucket: STATUS_PAD floats in front of the gradients, the first of them the step's status word
        # (0 = every launch of this rank's forward/backward was clean).  It is summed over the ranks by the same
        # all-reduce as the gradients, so all ranks agree on whether to apply the step (see step()).
        self._bucket = torch.zeros(self.STATUS_PAD + P, dtype=torch.float32, device=self.device)
        self.grads = self._bucket[self.STATUS_PAD:]
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.loss_terms = torch.zeros(4, dtype=torch.float32, device=self.device)   # total, bce, dice, focal
        self.loss = self.loss_terms[:1]
        # what the four slots hold: a K-class trainer reports (total, ce, dice, labels out of range)
        self.loss_term_names = ("total", "bce", "dice", "focal") if self.out_channels == 1 else ("total", "ce", "dice", "invalid")
        self.num_batches_tracked = 0
        self._loss_cfg = None if self.out_channels == 1 else metrics.ClassLossSpec()
        self._class_work = None
        self._metric = torch.zeros(4, dtype=torch.float32, device=self.device)
        rc = self._lib.unet_train_attach(h, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.exp_avg),
                                         _lib.ptr(self.exp_avg_sq), _lib.ptr(self.bn))
        _lib.check(rc, "unet_train_attach", h)
        if self.overlap and dp.world(self.group)[1] > 1:
            self._enable_overlap()

    def set_loss(self, kind="bce", bce_weight=0.5, dice_weight=0.5, pos_weight=3.0, smooth=1e-6, focal_weight=None,
                 alpha=0.25, gamma=2.0, ce_weight=None, class_weights=None, ignore_index=None):
        """The reference's `criterion = ...` line (INTEGRATION.md has the mapping).
        'bce': BCEWithLogitsLoss (reference README.md:1694-1709, BASELINE.json config);
        'bce_dice': the training script's BCEDiceLoss(0.5, 0.5, pos_weight=3) (README.md:1855-1893, :2169-2170);
        'focal': focal_weight (default 1) * FocalLoss(alpha, gamma) (README.md:1914-1939);
        'dice': dice_weight (as given; DiceLoss itself is dice_weight=1) * DiceLoss(smooth) (README.md:1781-1807);
        'focal_dice': focal_weight (default 0.5) * FocalLoss + dice_weight * DiceLoss - the table's choice for masks
        under 5 % lane (README.md:1949);
        'combo': bce_weight * BCE(pos_weight) + focal_weight * Focal + dice_weight * Dice, all three weights given.
        self.loss_terms then holds (total, bce, dice, focal); every term is reported whatever its weight.
        A K-class trainer takes 'ce': ce_weight (default 1) * F.cross_entropy(weight=class_weights,
        ignore_index=ignore_index), or 'ce_dice': ce_weight (default 0.5) * that + dice_weight * the softmax Dice loss
        over the classes with `smooth` (include/unet_hip.h has the formulas); self.loss_terms then holds (total, ce,
        dice, number of labels out of range)."""
        if kind in ("ce", "ce_dice") or self.out_channels > 1:
            if kind not in ("ce", "ce_dice"):
                raise ValueError(f"{kind!r}: a {self.out_channels}-class trainer takes 'ce' or 'ce_dice'")
            if self.out_channels == 1:
                raise ValueError(f"{kind!r} needs a K-class model (output.weight with K > 1 rows)")
            wc = (1.0 if kind == "ce" else 0.5) if ce_weight is None else ce_weight
            spec = metrics.ClassLossSpec(kind, wc, 0.0 if kind == "ce" else dice_weight, smooth, class_weights, ignore_index)
            cfg = spec.to_c(self.out_channels)
            _lib.check(self._lib.unet_train_set_class_loss(self._h, C.byref(cfg)), "unet_train_set_class_loss", self._h)
            self._loss_cfg = spec
            return
        if kind == "bce":
            rc = self._lib.unet_train_set_loss(self._h, 0, 1.0, 0.0, 1.0, smooth)
        elif kind == "bce_dice":
            rc = self._lib.unet_train_set_loss(self._h, 1, bce_weight, dice_weight, pos_weight, smooth)
        elif kind in ("focal", "dice", "focal_dice", "combo"):
            if kind == "combo":
                if focal_weight is None:
                    raise ValueError("'combo' takes bce_weight, focal_weight and dice_weight explicitly")
                wb, wf, wd = bce_weight, focal_weight, dice_weight
            elif kind == "focal":
                wb, wf, wd = 0.0, 1.0 if focal_weight is None else focal_weight, 0.0
            elif kind == "dice":
                wb, wf, wd = 0.0, 0.0, dice_weight
            else:
                wb, wf, wd = 0.0, 0.5 if focal_weight is None else focal_weight, dice_weight
            spec = metrics.LossSpec(kind, wb, wf, wd, pos_weight, alpha, gamma, smooth)
            cfg = spec.to_c()
            _lib.check(self._lib.unet_train_set_loss_cfg(self._h, C.byref(cfg)), "unet_train_set_loss_cfg", self._h)
            self._loss_cfg = spec
            return
        else:
            raise ValueError(kind)
        _lib.check(rc, "unet_train_set_loss", self._h)
        self.loss_terms[3:].zero_()     # these two losses have no focal term and never write the slot
        self._loss_cfg = (kind, bce_weight, dice_weight, pos_weight, smooth)

    def dice_metric(self, logits, targets, threshold=0.5, smooth=1e-6):
        """Dice score of the validation loop (reference README.md:2103-2104, :2115-2120):
        pred = sigmoid(logits) > threshold; returns a 1-element device tensor (no host sync)."""
        from .model import _logit
        logits = logits.to(self.device, torch.float32).contiguous()
        targets = targets.to(self.device, torch.float32).contiguous()
        if logits.numel() != targets.numel():
            raise ValueError("logits and targets differ in size")
        _lib.call("unet_dice_metric", self.device, logits, targets, logits.numel(), _logit(threshold), smooth, self._metric)
        return self._metric[:1].clone()

    # ---- one step, in the reference's order ------------------------------------------------------
    def forward_backward(self, images, targets, return_logits=False):
        """images: (N,H,W,3) uint8 frames or (N,3,H,W) float32 normalised; targets (N,1,H,W) float 0/1 - for a K-class
        trainer (N,H,W) uint8 class labels.  Fills self.grads (zero_grad + backward) and self.loss; returns the logits
        ((N,K,H,W) for K classes) if asked."""
        dp.broadcast_buffers(self.bn, self.group)
        multi = self.out_channels > 1
        if multi:
            if targets.dtype != torch.uint8:
                raise ValueError("a K-class trainer takes uint8 label planes (N,H,W)")
            targets = targets.to(self.device).contiguous()
        else:
            targets = targets.to(self.device, torch.float32).contiguous()
        images = images.to(self.device).contiguous()
        if images.dtype == torch.uint8:
            n, h, w, _ = images.shape
            fn = self._lib.unet_train_forward_backward_labels_u8 if multi else self._lib.unet_train_forward_backward_u8
        else:
            images = images.to(torch.float32)
            n, _, h, w = images.shape
            fn = self._lib.unet_train_forward_backward_labels_f32 if multi else self._lib.unet_train_forward_backward_f32
        if multi and targets.numel() != n * h * w:
            raise ValueError("labels must be (N,H,W), one byte per pixel of the images")
        logits = torch.empty((n, self.out_channels, h, w), dtype=torch.float32, device=self.device) if return_logits else None
        rc = fn(self._h, _lib.ptr(images), _lib.ptr(targets), n, h, w, _lib.ptr(self.loss_terms), _lib.ptr(logits),
                _lib.stream(self.device))
        self._fb_rc = int(rc)
        if rc != 0 and self._defer_fb_error:    # step() under data parallelism: the ranks have to fail together
            return logits
        _lib.check(rc, "unet_train_forward_backward", self._h)
        self.num_batches_tracked += 1
        return logits

    # overlap_allreduce (off by default): the exchange is 124 MB against a 49 ms step (1-2 % at xGMI rates), while the
    # persistent convolution kernels assume all 256 CUs - a collective kernel that holds some of them while the
    # encoder's backward runs makes every statically-strided kernel wait for its slowest CU.  Until an 8-GPU run has
    # measured both, the gradients are exchanged after the backward pass; the two-bucket overlap stays selectable.
    def _enable_overlap(self):
        """Two gradient buckets (reference: none; torch DDP's bucketing in miniature): the tail of the flat buffer -
        decoder, bottleneck, head: final two thirds into the backward pass - is all-reduced on a communication stream
        that the library releases at that point, under the encoder's backward; the encoder's bucket follows."""
        if self._comm is None:
            self._comm = torch.cuda.Stream(self.device)
            self._split = int(self._lib.unet_train_grad_split(self._h))
            _lib.check(self._lib.unet_train_set_comm_stream(self._h, C.c_void_p(self._comm.cuda_stream)),
                       "unet_train_set_comm_stream", self._h)

    def allreduce_grads(self):
        _, ws = dp.world(self.group)
        if ws == 1:
            return 1.0
        # the bucket (or its last part: the encoder's, exchanged after the backward pass has ended) starts with the
        # status word
        if not self.overlap:
            work, scale = dp.allreduce_flat_sum(self._bucket, self.group)
            return scale
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self._comm):     # already waiting for the mid-backward event
            dp.allreduce_flat_sum(self.grads[self._split:], self.group)
        dp.allreduce_flat_sum(self._bucket[:self.STATUS_PAD + self._split], self.group)
        main.wait_stream(self._comm)            # the optimizer step needs both buckets
        return 1.0 / ws

    def loss_dict(self):
        """The terms of the last step by name (one host read): total / bce / dice / focal, for a K-class trainer
        total / ce / dice / invalid."""
        return dict(zip(self.loss_term_names, (float(v) for v in self.loss_terms.cpu())))

    def optimizer_step(self, grad_scale=1.0):
        self.step_count += 1
        rc = self._lib.unet_train_adam_step(self._h, self.step_count, self.lr, self.betas[0], self.betas[1], self.eps,
                                            self.weight_decay, 1 if self.decoupled else 0, grad_scale,
                                            _lib.stream(self.device))
        _lib.check(rc, "unet_train_adam_step", self._h)

    def reset_optimizer(self):
        """A fresh Adam: zeroed moments and step count; parameters, BatchNorm buffers and the rate stay
        (loop.fit_progressive calls this at the start of every stage)."""
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.step_count = 0

    def device_error(self, current_stream_only=False):
        """Wait for the device (or, with current_stream_only, for torch's current stream of it: everything the trainer
        launches goes there) and return (and clear) the status of every launch on this handle since the last call: 0,
        UNET_ERR_HIP after a kernel-side failure, UNET_ERR_RANGE when an f16x3 activation left the fp16 range
        (include/unet_hip.h)."""
        if current_stream_only:
            return int(self._lib.unet_device_error_on(self._h, _lib.stream(self.device)))
        return int(self._lib.unet_device_error(self._h))

    def step(self, images, targets):
        """forward + backward, gradient exchange, optimizer step.  With check_device_status (default) the step refuses
        to update the parameters from gradients a failed launch produced - on EVERY rank: a failure is local to one rank
        (its kernels, its frames), but its gradients are summed into every rank's buffer, and a rank that raised alone
        would leave the others waiting in the next collective.  So each rank's status word (unet_device_status_to; or the
        status of a forward/backward call that failed at its entry) travels in front of the gradients through the same
        all-reduce; afterwards every rank reads the sum, and either all of them raise or all of them step.  One wait per
        step, for the trainer's stream only.

        accum_steps = k > 1: every call still returns its micro-batch's loss; calls 1 .. k-1 add the gradients to an
        accumulation buffer (the first is a copy), call k writes accumulated + own gradients into the bucket, and only
        then the exchange and ONE update with grad_scale = 1 / (k * world) follow.  max_grad_norm: the scaled gradient
        is clipped to that global norm (torch.nn.utils.clip_grad_norm_'s formula; the reference has no counterpart).
        skip_nonfinite: an update whose gradients hold an inf or a NaN is not applied.  With any of the three the
        update goes through unet_train_adam_step_rec and a 2-double record on the device (self.grad_record: sum of
        squares, number of non-finite gradients), taken from the bucket every rank holds after the exchange, so all
        ranks clip alike and skip together.  With check_device_status the record is read in the step's one wait:
        self.grad_norm is set, and a skipped update leaves step_count alone and counts in self.skipped_steps; without
        skip_nonfinite non-finite gradients reach the parameters as they always did.  With
        check_device_status=False nothing is read: the optimiser kernel's own guard leaves parameters and moments
        untouched when the record counts a non-finite gradient (whatever skip_nonfinite says), step_count advances
        all the same, and grad_norm and skipped_steps stay as they are.
        A failed micro-step on one rank raises as before and discards the pending accumulation; on several ranks it
        is latched and raised by all of them at the exchange, where none applies."""
        if self._extended():
            return self._step_extended(images, targets)
        _, ws = dp.world(self.group)
        if not self.check_device_status:
            self.forward_backward(images, targets)
            self.optimizer_step(self.allreduce_grads())
            return self.loss
        if ws == 1:
            self.forward_backward(images, targets)
            rc = self.device_error(current_stream_only=True)
            if rc != 0:
                raise _lib.UnetError(rc, "unet_device_error: the gradients of this step are invalid, no update was applied")
            self.optimizer_step(1.0)
            return self.loss
        self._defer_fb_error = True
        try:
            self.forward_backward(images, targets)
        finally:
            self._defer_fb_error = False
        if self._fb_rc != 0:     # failed at its entry: nothing (or not everything) was launched
            self._bucket[:1].fill_(1.0)
        else:
            _lib.check(self._lib.unet_device_status_to(self._h, _lib.ptr(self._bucket), _lib.stream(self.device)),
                       "unet_device_status_to", self._h)
        scale = self.allreduce_grads()
        failed = float(self._bucket[0].item())               # waits for the trainer's stream: backward + exchange
        local = self._fb_rc or self.device_error(current_stream_only=True)   # this rank's own record, cleared
        if failed != 0.0:
            who = "this rank" if local else "another rank"
            raise _lib.UnetError(local or _lib.UNET_ERR_HIP,
                                 f"data-parallel step: {int(round(failed))} of {ws} ranks reported a failed launch ({who}); "
                                 "the gradients of this step are invalid, no rank applied an update",
                                 self._lib.unet_last_error(self._h).decode() if local else "")
        self.optimizer_step(scale)
        return self.loss

    # ---- accumulation, clipping, non-finite guard (csrc/grad_kernels.h) -------------------
    def _extended(self):
        return (int(self.accum_steps) > 1 or self.max_grad_norm is not None or bool(self.skip_nonfinite)
                or self._pending > 0)

    @property
    def grad_record(self):
        """The 2-double device tensor the gradient pass writes: [sum of squares of the finite gradients of the last
        update's bucket, before grad_scale; number of non-finite ones].  Allocated on first need."""
        if self._grad_rec is None:
            self._grad_rec = torch.zeros(2, dtype=torch.float64, device=self.device)
            self._grad_work = torch.empty(int(self._lib.unet_grad_work_bytes()) // 8, dtype=torch.float64,
                                          device=self.device)
            self._rec_host = torch.zeros(2, dtype=torch.float64).pin_memory()
        return self._grad_rec

    def _grad_pass(self, dst, a, b=None, record=False):
        rec = self.grad_record if record else None
        _lib.call("unet_grad_accumulate_f32", self.device, dst, a, b, dst.numel(), rec, self._grad_work if record else None)

    def optimizer_step_rec(self, grad_scale=1.0):
        """optimizer_step with the multiplier formed on the device from self.grad_record (unet_train_adam_step_rec):
        clipping to max_grad_norm (None: none), and no update at all if the record counts a non-finite gradient."""
        self.step_count += 1
        max_norm = float("inf") if self.max_grad_norm is None else float(self.max_grad_norm)
        rc = self._lib.unet_train_adam_step_rec(self._h, self.step_count, self.lr, self.betas[0], self.betas[1],
                                                self.eps, self.weight_decay, 1 if self.decoupled else 0, grad_scale,
                                                max_norm, _lib.ptr(self.grad_record), _lib.stream(self.device))
        _lib.check(rc, "unet_train_adam_step_rec", self._h)

    def clip_coefficient(self, grad_scale, sumsq):
        """The multiplier unet_train_adam_step_rec forms from record[0] = sumsq, in the same double arithmetic."""
        max_norm = float("inf") if self.max_grad_norm is None else float(np.float32(self.max_grad_norm))
        gs = float(np.float32(grad_scale))
        return float(np.float32(gs * min(1.0, max_norm / (abs(gs) * float(np.sqrt(np.float64(sumsq))) + 1e-6))))

    def _step_extended(self, images, targets):
        _, ws = dp.world(self.group)
        checked = self.check_device_status
        together = checked and ws > 1          # the ranks fail together, at the exchange
        try:
            self._defer_fb_error = together
            try:
                self.forward_backward(images, targets)
            finally:
                self._defer_fb_error = False
            if together and self._fb_rc != 0:
                self._latched_rc = self._latched_rc or self._fb_rc
            self._pending += 1
            if self._pending < max(1, int(self.accum_steps)):
                if self._acc is None:
                    self._acc = torch.empty_like(self.params)
                # acc = grads (first micro-batch) or acc + grads; enqueued before the wait below
                self._grad_pass(self._acc, self.grads if self._pending == 1 else self._acc,
                                None if self._pending == 1 else self.grads)
                if checked and ws == 1:
                    rc = self.device_error(current_stream_only=True)
                    if rc != 0:
                        raise _lib.UnetError(rc, "unet_device_error: the gradients of this micro-step are invalid, the "
                                             "pending accumulation was discarded")
                return self.loss
            self._apply(in_bucket=True)
        except _lib.UnetError:
            self._pending, self._latched_rc = 0, 0
            raise
        return self.loss

    def apply_update(self):
        """The second half of step() for a caller that ran forward_backward itself: the bucket as it is counts as one
        more micro-batch, and what is pending with it is exchanged and applied as one update through the record entry
        (clipping and guard as configured), whatever accum_steps says."""
        self._pending += 1
        try:
            self._apply(in_bucket=True)
        except _lib.UnetError:
            self._pending, self._latched_rc = 0, 0
            raise

    def flush_accumulation(self):
        """Apply a partial accumulation (fewer than accum_steps micro-batches, e.g. at an epoch's end) as one update
        with grad_scale = 1 / (pending * world).  Nothing pending: nothing happens.  Under data parallelism every rank
        must call it at the same point (loop.fit does)."""
        if self._pending == 0:
            return False
        try:
            self._apply(in_bucket=False)
        except _lib.UnetError:
            self._pending, self._latched_rc = 0, 0
            raise
        return True

    def _apply(self, in_bucket):
        """The boundary of an accumulation: bucket, exchange, record, update.  in_bucket: the last of the pending
        micro-batches' gradients are still in the bucket (step), else all of them are in the accumulation buffer."""
        _, ws = dp.world(self.group)
        checked = self.check_device_status
        n = self._pending
        accumulated = n > 1 or not in_bucket
        one_rank_record = ws == 1
        if accumulated:      # grads = acc + grads, or the copy of acc; with one rank the record comes from this pass
            self._grad_pass(self.grads, self._acc, self.grads if in_bucket else None, record=one_rank_record)
        elif one_rank_record:
            self._grad_pass(self.grads, self.grads, None, record=True)
        scale = 1.0 / (n * ws)
        if ws > 1:
            if checked:
                if self._latched_rc != 0:
                    self._bucket[:1].fill_(1.0)
                else:
                    _lib.check(self._lib.unet_device_status_to(self._h, _lib.ptr(self._bucket), _lib.stream(self.device)),
                               "unet_device_status_to", self._h)
            if accumulated:  # the two-bucket overlap follows the backward pass, which this bucket no longer does
                dp.allreduce_flat_sum(self._bucket, self.group)
            else:
                self.allreduce_grads()
            self._grad_pass(self.grads, self.grads, None, record=True)    # from what every rank now holds
        self._pending = 0
        if not checked:
            self._latched_rc = 0
            self.optimizer_step_rec(scale)
            return
        self._rec_host.copy_(self.grad_record, non_blocking=True)         # read in the wait that follows
        if ws > 1:
            failed = float(self._bucket[0].item())
            latched, self._latched_rc = self._latched_rc, 0
            local = latched or self.device_error(current_stream_only=True)
            if failed != 0.0:
                who = "this rank" if local else "another rank"
                raise _lib.UnetError(local or _lib.UNET_ERR_HIP,
                                     f"data-parallel step: {int(round(failed))} of {ws} ranks reported a failed launch "
                                     f"({who}); the gradients of this update are invalid, no rank applied it",
                                     self._lib.unet_last_error(self._h).decode() if local else "")
        else:
            rc = self.device_error(current_stream_only=True)
            if rc != 0:
                raise _lib.UnetError(rc, "unet_device_error: the gradients of this step are invalid, no update was applied")
        sumsq, bad = float(self._rec_host[0]), float(self._rec_host[1])
        self.grad_norm = scale * float(np.sqrt(sumsq))
        if bad != 0.0:
            if self.skip_nonfinite:
                self.skipped_steps += 1
                return
            # not guarded: the non-finite gradients reach the parameters, as they do without these features
            self.optimizer_step(self.clip_coefficient(scale, sumsq))
            return
        self.optimizer_step_rec(scale)

    def snapshot_state(self):
        """Device clones of parameters, BatchNorm buffers and both moments, with step_count, num_batches_tracked, lr
        and the accumulation settings: what restore_state needs to put the trainer back (loop.find_lr).  A pending
        accumulation is not part of it."""
        return {"params": self.params.clone(), "bn": self.bn.clone(), "exp_avg": self.exp_avg.clone(),
                "exp_avg_sq": self.exp_avg_sq.clone(), "step_count": self.step_count,
                "num_batches_tracked": self.num_batches_tracked, "lr": self.lr, "accum_steps": self.accum_steps,
                "max_grad_norm": self.max_grad_norm, "skip_nonfinite": self.skip_nonfinite}

    def restore_state(self, s):
        """Back to a snapshot_state(); a pending accumulation is discarded; ends with unet_train_repack."""
        for name in ("params", "bn", "exp_avg", "exp_avg_sq"):
            getattr(self, name).copy_(s[name])
        for name in ("step_count", "num_batches_tracked", "lr", "accum_steps", "max_grad_norm", "skip_nonfinite"):
            setattr(self, name, s[name])
        self._pending, self._latched_rc = 0, 0
        _lib.check(self._lib.unet_train_repack(self._h, _lib.stream(self.device)), "unet_train_repack", self._h)

    # ---- validation (reference README.md:2087-2112) and the loop around both (README.md:2185-2231) ----------
    def eval_logits(self, images):
        """Eval-mode forward (running statistics, nothing of the training state written) on the parameters as they are
        on the device right now; images as forward_backward takes them -> logits (N,1,H,W) on the device, (N,K,H,W) for a
        K-class trainer."""
        images = images.to(self.device).contiguous()
        if images.dtype == torch.uint8:
            n, h, w, _ = images.shape
            fn = self._lib.unet_train_eval_u8
        else:
            images = images.to(torch.float32)
            n, _, h, w = images.shape
            fn = self._lib.unet_train_eval_f32
        logits = torch.empty((n, self.out_channels, h, w), dtype=torch.float32, device=self.device)
        _lib.check(fn(self._h, _lib.ptr(images), n, h, w, _lib.ptr(logits), _lib.stream(self.device)), "unet_train_eval",
                   self._h)
        return logits

    def validate(self, batches, threshold=0.5, return_logits=False):
        """The reference's validate(): eval-mode forward over `batches` (an iterable of (images, targets); images as
        forward_backward takes them, targets float 0/1 or uint8 0 / non-zero), the loss set by set_loss and the
        segmentation metrics reduced on the device, one host read at the end.  No state of the trainer moves:
        parameters, BatchNorm buffers, gradients, moments, step_count and num_batches_tracked stay as they are, and
        BatchNorm buffers are not broadcast.  Under a process group every rank validates its own batches and the
        accumulators are summed, so all ranks return the same SegMetrics.  Raises like step() when the device reports
        a failed launch or an activation beyond the fp16 range for the pass.  With return_logits: (SegMetrics, [logits
        per batch]).
        A K-class trainer takes (images, uint8 labels) batches and returns metrics.ClassMetrics: the labels are the
        argmax of the eval logits, the confusion matrix is filled on the device (unet_confusion_accumulate) and gives
        per-class IoU, miou, pixel_acc and dice (the mean per-class Dice, what loop.fit compares); the loss terms are
        those of set_loss.  With return_logits: (ClassMetrics, [logits per batch])."""
        if self.out_channels > 1:
            return self._validate_classes(batches, return_logits)
        acc = torch.zeros(metrics.NUM_ACCUMULATORS, dtype=torch.float64, device=self.device)
        kept = []
        for images, targets in batches:
            logits = self.eval_logits(images)
            metrics.accumulate(self._lib, self.device.index, logits, torch.as_tensor(targets), acc, _lib.stream(self.device),
                               threshold=threshold, loss_cfg=self._loss_cfg)
            if return_logits:
                kept.append(logits)
        rc = self.device_error(current_stream_only=True)
        _, ws = dp.world(self.group)
        if ws > 1:
            # the ranks fail together: this rank's status rides in a reserved accumulator
            acc[metrics.NUM_ACCUMULATORS - 1] = 1.0 if rc else 0.0
            dp.allreduce_accumulators(acc, self.group)
        host = acc.cpu().numpy()
        if rc != 0 or host[metrics.NUM_ACCUMULATORS - 1] != 0.0:
            raise _lib.UnetError(rc or _lib.UNET_ERR_HIP, "unet_device_error: the validation pass is invalid, no metrics "
                                 "are returned", self._lib.unet_last_error(self._h).decode() if rc else "")
        host[metrics.NUM_ACCUMULATORS - 1] = 0.0
        m = metrics.SegMetrics(host)
        return (m, kept) if return_logits else m

    def predict_labels(self, logits, mask_class=None):
        """(N,K,H,W) logits -> (N,H,W) uint8 argmax labels on the device (ties to the lowest class); with mask_class
        also the byte plane that is 255 where the label is that class."""
        n, k, h, w = logits.shape
        labels = torch.empty((n, h, w), dtype=torch.uint8, device=self.device)
        mask = torch.empty_like(labels) if mask_class is not None else None
        _lib.call("unet_class_labels_f32", self.device, logits, n, k, h * w, labels, int(mask_class or 0), mask)
        return labels if mask is None else (labels, mask)

    def _validate_classes(self, batches, return_logits):
        k = self.out_channels
        spec = self._loss_cfg
        cfg = spec.to_c(k)
        cm = metrics.ConfusionMatrix(k, self.device, None if spec.ignore_index < 0 else spec.ignore_index)
        if self._class_work is None:
            self._class_work = torch.empty(int(self._lib.unet_class_loss_work_bytes()) // 8, dtype=torch.float64,
                                           device=self.device)
        terms = torch.zeros(4, dtype=torch.float32, device=self.device)
        sums = torch.zeros(4, dtype=torch.float64, device=self.device)
        kept, nb = [], 0
        for images, labels in batches:
            labels = torch.as_tensor(labels)
            if labels.dtype != torch.uint8:
                raise ValueError("a K-class trainer validates against uint8 label planes (N,H,W)")
            labels = labels.to(self.device).contiguous()
            logits = self.eval_logits(images)
            n, _, h, w = logits.shape
            if labels.numel() != n * h * w:
                raise ValueError("labels must be (N,H,W), one byte per pixel of the images")
            _lib.call("unet_class_loss_grad", self.device, logits, labels, n, k, h * w, C.byref(cfg), terms, None,
                      self._class_work)
            sums += terms
            cm.accumulate(self.predict_labels(logits), labels)
            nb += 1
            if return_logits:
                kept.append(logits)
        rc = self.device_error(current_stream_only=True)
        # counts (exact below 2^53), the loss sums, the batches and this rank's status in one float64 vector
        acc = torch.cat([cm.acc.to(torch.float64), sums, torch.tensor([float(nb), 1.0 if rc else 0.0], dtype=torch.float64,
                                                                       device=self.device)])
        _, ws = dp.world(self.group)
        if ws > 1:
            dp.allreduce_accumulators(acc, self.group)
        host = acc.cpu().numpy()
        if rc != 0 or host[-1] != 0.0:
            raise _lib.UnetError(rc or _lib.UNET_ERR_HIP, "unet_device_error: the validation pass is invalid, no metrics "
                                 "are returned", self._lib.unet_last_error(self._h).decode() if rc else "")
        m = metrics.ClassMetrics(host[:k * k], host[k * k:k * k + 3], int(round(host[-2])), int(round(host[k * k + 3])))
        return (m, kept) if return_logits else m

    def sweep(self, batches, thresholds=metrics.DEFAULT_THRESHOLDS):
        """Confusion counts and metrics at every threshold of `thresholds` (probabilities, ascending) in one eval-mode
        forward over `batches` on the live parameters, as validate forwards them: each threshold is mapped to a logit as
        validate maps its one and compared with the logits on the device (unet_score_sweep_accumulate); 2 * (T + 1)
        integers are read at the end.  No state of the trainer moves.  Every rank sweeps its own batches (the counts
        are not summed over a process group).  Raises like validate when the device reports a failed launch or an
        activation beyond the fp16 range for the pass.  Returns metrics.ThresholdSweep."""
        probs = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        t = metrics.sweep_thresholds(probs, "logit")
        counts = torch.zeros(2 * (t.size + 1), dtype=torch.int64, device=self.device)
        for images, targets in batches:
            logits = self.eval_logits(images)
            metrics.sweep_accumulate(self._lib, self.device.index, logits, torch.as_tensor(targets), t, counts,
                                     _lib.stream(self.device))
        rc = self.device_error(current_stream_only=True)
        if rc != 0:
            raise _lib.UnetError(rc, "unet_device_error: the sweep is invalid, no metrics are returned",
                                 self._lib.unet_last_error(self._h).decode())
        return metrics.ThresholdSweep(t, counts.cpu().numpy(), "logit", probabilities=probs)

    def fit(self, train_batches, val_batches, epochs, scheduler=None, save_dir=None, patience=None, on_epoch=None):
        """The reference's train(config) loop: see loop.fit."""
        return loop.fit(self, train_batches, val_batches, epochs, scheduler=scheduler, save_dir=save_dir,
                        patience=patience, on_epoch=on_epoch)

    # ---- views in the reference's state_dict naming -----------------------------------------------
    def _view(self, flat_p, flat_b):
        out = {}
        for name, isb, off, numel in self.layout:
            out[name] = (flat_b if isb else flat_p)[off:off + numel].view(self._shapes[name])
        return out

    def state_dict(self):
        sd = {k: v.detach().cpu().clone() for k, v in self._view(self.params, self.bn).items()}
        for name in list(sd):
            if name.endswith("running_var"):
                sd[name.replace("running_var", "num_batches_tracked")] = torch.tensor(self.num_batches_tracked)
        return sd

    # ---- checkpoints in the reference's format (README.md:2208-2213) --------------------------------
    def _param_entries(self):
        return [(n, off, numel, self._shapes[n]) for (n, isb, off, numel) in self.layout if not isb]

    def save_checkpoint(self, path, epoch=0, best_dice=None, with_optimizer=True):
        """The reference's checkpoint.  A pending gradient accumulation (accum_steps > 1, between updates) is not
        stored: call flush_accumulation() first if it must not be lost."""
        osd = None
        if with_optimizer:
            osd = checkpoint.optimizer_state_dict(self._param_entries(), self.exp_avg, self.exp_avg_sq,
                                                  self.step_count, self.lr, self.betas, self.eps,
                                                  self.weight_decay, self.decoupled)
        checkpoint.save(path, self.state_dict(), epoch=epoch, optimizer_state=osd, best_dice=best_dice)

    def load_checkpoint(self, path):
        """Restore parameters, BatchNorm buffers and (if present) the Adam moments and step; returns the rest
        of the checkpoint (epoch, best_dice)."""
        msd, rest = checkpoint.load(path)
        for name, isb, off, numel in self.layout:
            (self.bn if isb else self.params)[off:off + numel].copy_(msd[name].reshape(-1).to(torch.float32))
        nbt = [v for k, v in msd.items() if k.endswith("num_batches_tracked")]
        if nbt:
            self.num_batches_tracked = int(nbt[0])
        if "optimizer_state_dict" in rest:
            step, group = checkpoint.load_optimizer_state(rest.pop("optimizer_state_dict"), self._param_entries(),
                                                          self.exp_avg, self.exp_avg_sq)
            self.step_count = step
            self.lr, self.betas, self.eps = group["lr"], tuple(group["betas"]), group["eps"]
            self.weight_decay = group["weight_decay"]
            # torch.optim.AdamW is Adam with decoupled_weight_decay=True (torch 2.10 writes that key for both classes);
            # older AdamW files lack the key, so a caller-selected AdamW is kept when the file does not say
            if "decoupled_weight_decay" in group:
                self.decoupled = bool(group["decoupled_weight_decay"])
        # packed MFMA operands follow the parameters; the TrainState (loss configuration, workspace) stays
        _lib.check(self._lib.unet_train_repack(self._h, _lib.stream(self.device)), "unet_train_repack", self._h)
        return rest

    def grad_dict(self):
        return {k: v for k, v in self._view(self.grads, self.bn).items() if "running_" not in k}

    def profile(self, on=True):
        _lib.check(self._lib.unet_profile_enable(self._h, 1 if on else 0), "unet_profile_enable", self._h)

    def profile_records(self):
        out = []
        name = C.create_string_buffer(64)
        ms, fl, by = C.c_double(), C.c_double(), C.c_double()
        for i in range(self._lib.unet_profile_count(self._h)):
            self._lib.unet_profile_get(self._h, i, name, 64, C.byref(ms), C.byref(fl), C.byref(by))
            out.append((name.value.decode(), ms.value, fl.value, by.value))
        return out

    def release(self):
        if getattr(self, "_h", None) is not None:
            torch.cuda.synchronize(self.device)
            self._lib.unet_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
