"""The reference's training loop (README.md:2185-2231) on a trainer object: train epoch -> validate ->
scheduler.step() -> best_model.pth when the validation Dice improves -> early stop -> checkpoint_epoch{N}.pth every 10th
epoch -> last_model.pth.  Pure host control flow: `fit` only calls `trainer.step`, `trainer.validate`,
`trainer.save_checkpoint` and sets `trainer.lr`, so it runs on any object with those (tests/test_validate_cpu.py).
`fit_progressive` runs `fit` once per stage of the reference's progressive training, on the data set at each size.
`find_lr` is the reference's learning-rate range test (tip 1, README.md:2364-2422) over `trainer.step`."""
from __future__ import annotations

import collections
import math
import os


def _epoch_iter(source):
    """A data set is a callable returning a fresh iterable per epoch, or a re-iterable sequence."""
    return source() if callable(source) else source


def fit(trainer, train_batches, val_batches, epochs, scheduler=None, save_dir=None, patience=None, on_epoch=None):
    """Returns the per-epoch history: a list of dicts {epoch, lr, train_loss, val_loss, val_dice, val (the SegMetrics),
    best_dice, improved, patience_counter}.  `lr` is the rate the epoch trained with.  scheduler: an object of
    schedules.py (step() returns the next rate); save_dir None writes no files; patience None never stops early;
    on_epoch(record) is called at the end of every epoch (there is no logging in here)."""
    best_dice = 0.0
    patience_counter = 0
    history = []
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    for epoch in range(1, int(epochs) + 1):
        lr = trainer.lr
        total, steps = 0.0, 0
        for images, targets in _epoch_iter(train_batches):
            total += float(trainer.step(images, targets))     # loss.item() per step (README.md:2077)
            steps += 1
        flush = getattr(trainer, "flush_accumulation", None)
        if flush is not None:
            flush()     # a partial gradient accumulation is applied here: an epoch never leaks gradients into the next
        train_loss = total / steps if steps else float("nan")
        val = trainer.validate(_epoch_iter(val_batches))
        if scheduler is not None:
            trainer.lr = scheduler.step()
        improved = val.dice > best_dice
        if improved:
            best_dice = val.dice
            patience_counter = 0
            if save_dir is not None:
                trainer.save_checkpoint(os.path.join(save_dir, "best_model.pth"), epoch=epoch, best_dice=best_dice)
        else:
            patience_counter += 1
        record = {"epoch": epoch, "lr": lr, "train_loss": train_loss, "val_loss": val.loss, "val_dice": val.dice,
                  "val": val, "best_dice": best_dice, "improved": improved, "patience_counter": patience_counter}
        for extra in ("grad_norm", "skipped_steps"):    # the epoch's last update's norm; skipped updates so far
            if hasattr(trainer, extra):
                record[extra] = getattr(trainer, extra)
        history.append(record)
        if on_epoch is not None:
            on_epoch(record)
        if patience is not None and patience_counter >= patience:
            break
        if epoch % 10 == 0 and save_dir is not None:
            trainer.save_checkpoint(os.path.join(save_dir, f"checkpoint_epoch{epoch}.pth"), epoch=epoch,
                                    with_optimizer=False)
    if save_dir is not None:
        trainer.save_checkpoint(os.path.join(save_dir, "last_model.pth"), epoch=None, with_optimizer=False)
    return history


LRSweep = collections.namedtuple("LRSweep", "lrs losses recommended stopped")


def find_lr(trainer, batches, init_lr=1e-8, final_lr=10, num_iter=100, restore=True, diverge=None):
    """The reference's learning-rate range test (tip 1, `find_lr`, README.md:2364-2422): the rate rises geometrically
    from init_lr to final_lr over num_iter updates - mult = (final_lr / init_lr) ** (1 / num_iter); set the rate, step,
    record (lr, loss), lr *= mult, by repeated multiplication as there - until num_iter updates are recorded or the
    batches run out.  Returns LRSweep(lrs, losses, recommended, stopped): recommended is the rate of the smallest
    finite loss divided by 10 (None without a finite loss); stopped is None (ran to the end), "exhausted" (the batches
    ran out), "diverged" or "range".  diverge None runs to the end as the reference does; a number stops the sweep once
    a loss exceeds diverge * the best loss before it or is not finite.  A UnetError with UNET_ERR_RANGE (the f16x3
    range watch) ends the sweep with "range" instead of propagating.  One iteration is one applied update: with
    trainer.accum_steps = k it takes k batches and records the mean of their losses.  The sweep runs into divergence
    on purpose, so trainer.skip_nonfinite (where the trainer has it) is on for its duration and put back afterwards.
    restore: trainer.snapshot_state() before and trainer.restore_state() after, so the trainer leaves as it came.  No
    plotting.  Pure host control flow, like `fit`: only trainer.step, .lr, .skip_nonfinite and the two state calls."""
    from ._lib import UNET_ERR_RANGE, UnetError
    snapshot = trainer.snapshot_state() if restore else None
    guard = getattr(trainer, "skip_nonfinite", None)
    if guard is not None:
        trainer.skip_nonfinite = True
    micro = max(1, int(getattr(trainer, "accum_steps", 1)))
    mult = (final_lr / init_lr) ** (1 / num_iter)
    lr, best = init_lr, math.inf
    lrs, losses, stopped = [], [], None
    it = iter(_epoch_iter(batches))
    try:
        while len(lrs) < int(num_iter):
            trainer.lr = lr
            total = 0.0
            try:
                for _ in range(micro):
                    images, targets = next(it)
                    total += float(trainer.step(images, targets))
            except StopIteration:
                stopped = "exhausted"
                break
            except UnetError as e:
                if e.code != UNET_ERR_RANGE:
                    raise
                stopped = "range"
                break
            loss = total / micro
            lrs.append(lr)
            losses.append(loss)
            if diverge is not None and not (math.isfinite(loss) and loss <= diverge * best):
                stopped = "diverged"
                break
            if math.isfinite(loss):
                best = min(best, loss)
            lr *= mult
    finally:
        if guard is not None:
            trainer.skip_nonfinite = guard
        if restore:
            trainer.restore_state(snapshot)
    finite = [i for i, v in enumerate(losses) if math.isfinite(v)]
    recommended = lrs[min(finite, key=lambda i: losses[i])] / 10 if finite else None
    return LRSweep(lrs, losses, recommended, stopped)


REFERENCE_STAGES =[(128, 30, 1e-3), (192, 30, 1e-4), (224, 20, 1e-5)]   # (image_size, epochs, learning_rate)


def fit_progressive(trainer, train_source, val_source, stages, batch_size, augmenter, save_dir=None, **fit_kwargs):
    """The reference's progressive training (tip 4, README.md:2562-2589): one `fit` per stage (size, epochs, lr), each
    on the data set at that stage's size and each starting from the previous stage's weights.  train_source and
    val_source give a data set per size through `.at(size)` (annotate.TrainingSource: frames resized, masks rasterised
    at that size); the batches are augment.AugmentedBatches and augment.val_batches.  Every stage starts with a fresh
    optimiser, as the reference's `'pretrained': 'stage1_best.pth'` into a new run does: `trainer.reset_optimizer()`
    zeroes the Adam moments and the step count.  The weights carried over are the last epoch's, not a reloaded best
    checkpoint.  save_dir: stage i (from 1) writes into save_dir/stage{i}.  The other keywords go to `fit`, which is
    unchanged.  Returns the per-stage histories.  Pure host control flow, like `fit`."""
    from .augment import AugmentedBatches, val_batches
    histories = []
    for i, (size, epochs, lr) in enumerate(stages, start=1):
        train = AugmentedBatches(train_source.at(size), batch_size, augmenter)
        val = val_batches(val_source.at(size), batch_size, mask_threshold=augmenter.mask_threshold)
        trainer.reset_optimizer()
        trainer.lr = lr
        stage_dir = os.path.join(save_dir, f"stage{i}") if save_dir is not None else None
        histories.append(fit(trainer, train, val, epochs, save_dir=stage_dir, **fit_kwargs))
    return histories
