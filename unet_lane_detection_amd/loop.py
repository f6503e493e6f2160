"""The reference's training loop (README.md:2185-2231) on a trainer object: train epoch -> validate ->
scheduler.step() -> best_model.pth when the validation Dice improves -> early stop -> checkpoint_epoch{N}.pth every 10th
epoch -> last_model.pth.  Pure host control flow: `fit` only calls `trainer.step`, `trainer.validate`,
`trainer.save_checkpoint` and sets `trainer.lr`, so it runs on any object with those (tests/test_validate_cpu.py).
`fit_progressive` runs `fit` once per stage of the reference's progressive training, on the data set at each size."""
from __future__ import annotations

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


REFERENCE_STAGES = [(128, 30, 1e-3), (192, 30, 1e-4), (224, 20, 1e-5)]   # (image_size, epochs, learning_rate)


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
