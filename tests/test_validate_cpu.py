"""Host side of the validation pass: SegMetrics formulas and conventions, the reference's loop order in loop.fit on a
fake trainer, the accumulator all-reduce over a 2-process gloo group, the exported symbols."""
import ctypes as C
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from unet_lane_detection_amd import dp, loop, metrics
from unet_lane_detection_amd.metrics import SegMetrics
from unet_lane_detection_amd.schedules import CosineAnnealingWarmRestarts


def _acc(tp=0, fp=0, fn=0, tn=0, loss=0.0, bce=0.0, dl=0.0, dice=0.0, batches=0, pixels=None):
    a = np.zeros(16)
    a[:10] = [tp, fp, fn, tn, loss, bce, dl, dice, batches, tp + fp + fn + tn if pixels is None else pixels]
    return a


def test_segmetrics_formulas_from_hand_made_counts():
    m = SegMetrics(_acc(tp=30, fp=10, fn=20, tn=940, loss=1.5, bce=0.9, dl=2.1, dice=1.2, batches=3))
    assert m.iou == 30 / 60
    assert m.precision == 30 / 40
    assert m.recall == 30 / 50
    assert m.f1 == 60 / 90
    assert abs(m.f1 - 2 * m.precision * m.recall / (m.precision + m.recall)) < 1e-15
    assert m.pixel_accuracy == 970 / 1000
    assert m.loss == 0.5 and m.bce == 0.3 and abs(m.dice_loss - 0.7) < 1e-15 and abs(m.dice - 0.4) < 1e-15
    assert (m.tp, m.fp, m.fn, m.tn, m.batches, m.pixels) == (30, 10, 20, 940, 3, 1000)
    d = m.as_dict()
    assert d["iou"] == m.iou and d["dice"] == m.dice and d["tp"] == 30 and d["pixels"] == 1000 and d["loss"] == 0.5
    assert set(d) >= {"loss", "bce", "dice_loss", "dice", "iou", "precision", "recall", "f1", "pixel_accuracy"}
    assert "iou=0.5" in repr(m)


def test_segmetrics_counts_beyond_float32_integers_stay_exact():
    big = (1 << 40) + 1
    m = SegMetrics(_acc(tp=big, fp=1, fn=2, tn=3, batches=1))
    assert m.tp == big and m.pixels == big + 6
    assert m.iou == big / (big + 3)


def test_segmetrics_empty_denominators():
    # nothing predicted, nothing there: every ratio is 1.0, as compute_dice tends to with its smooth term
    m = SegMetrics(_acc(tn=100, batches=1, dice=1.0))
    assert m.iou == 1.0 and m.precision == 1.0 and m.recall == 1.0 and m.f1 == 1.0 and m.pixel_accuracy == 1.0
    # lanes there, none predicted: precision has an empty denominator (nothing claimed), the others are 0
    m = SegMetrics(_acc(fn=7, tn=93, batches=1))
    assert m.precision == 1.0 and m.recall == 0.0 and m.iou == 0.0 and m.f1 == 0.0
    # lanes predicted, none there
    m = SegMetrics(_acc(fp=7, tn=93, batches=1))
    assert m.recall == 1.0 and m.precision == 0.0 and m.iou == 0.0 and m.f1 == 0.0
    # no pixel at all, no batch: ratios 1.0, per-batch means undefined
    m = SegMetrics(np.zeros(16))
    assert m.pixel_accuracy == 1.0 and math.isnan(m.loss) and math.isnan(m.dice)
    with pytest.raises(ValueError):
        SegMetrics(np.zeros(10))


class _Val:
    def __init__(self, dice, loss):
        self.dice, self.loss = dice, loss


class _FakeTrainer:
    def __init__(self, dices):
        self.lr = 1e-3
        self.calls = []
        self._dices = list(dices)
        self._epoch = 0

    def step(self, images, targets):
        self.calls.append(("step", images, self.lr))
        return torch.tensor([float(images)])

    def validate(self, batches):
        self.calls.append(("validate", list(batches)))
        d = self._dices[self._epoch]
        self._epoch += 1
        return _Val(d, 1.0 - d)

    def save_checkpoint(self, path, epoch=0, best_dice=None, with_optimizer=True):
        self.calls.append(("save", os.path.basename(path), epoch, best_dice, with_optimizer))


class _Sched:
    def __init__(self, trainer):
        self.t, self.n = trainer, 0

    def step(self):
        self.n += 1
        self.t.calls.append(("sched", self.n))
        return 1e-3 / (1 + self.n)


def test_fit_follows_the_reference_loop_order(tmp_path):
    dices = [0.2, 0.5, 0.4, 0.6]
    tr = _FakeTrainer(dices)
    fresh = []

    def train_set():            # a callable: a fresh iterable per epoch
        fresh.append(1)
        return iter([(1.0, None), (3.0, None)])

    val_set = [(10.0, None)]    # a re-iterable sequence
    seen = []
    hist = loop.fit(tr, train_set, val_set, epochs=4, scheduler=_Sched(tr), save_dir=str(tmp_path / "ck"),
                    on_epoch=seen.append)
    assert len(fresh) == 4 and os.path.isdir(tmp_path / "ck")
    kinds = [c[0] if c[0] != "save" else "save:" + c[1] for c in tr.calls]
    epoch = ["step", "step", "validate", "sched"]
    assert kinds == (epoch + ["save:best_model.pth"] + epoch + ["save:best_model.pth"] + epoch + epoch +
                     ["save:best_model.pth", "save:last_model.pth"])
    # checkpoints: the best one wrapped with epoch / best_dice / optimizer, the last one a bare state_dict
    saves = [c for c in tr.calls if c[0] == "save"]
    assert saves[0] == ("save", "best_model.pth", 1, 0.2, True)
    assert saves[1] == ("save", "best_model.pth", 2, 0.5, True)
    assert saves[2] == ("save", "best_model.pth", 4, 0.6, True)
    assert saves[3] == ("save", "last_model.pth", None, None, False)
    # the scheduler's rate applies from the next epoch on
    lrs = [c[2] for c in tr.calls if c[0] == "step"]
    assert lrs == [1e-3, 1e-3, 5e-4, 5e-4, 1e-3 / 3, 1e-3 / 3, 2.5e-4, 2.5e-4]
    assert [h["epoch"] for h in hist] == [1, 2, 3, 4] and seen == hist
    assert [h["train_loss"] for h in hist] == [2.0] * 4            # mean of the per-step losses
    assert [h["val_dice"] for h in hist] == dices
    assert [h["val_loss"] for h in hist] == [1.0 - d for d in dices]
    assert [h["best_dice"] for h in hist] == [0.2, 0.5, 0.5, 0.6]
    assert [h["improved"] for h in hist] == [True, True, False, True]
    assert [h["patience_counter"] for h in hist] == [0, 0, 1, 0]
    assert [h["lr"] for h in hist] == [1e-3, 5e-4, 1e-3 / 3, 2.5e-4]
    assert all(h["val"].dice == h["val_dice"] for h in hist)


def test_fit_early_stop_and_periodic_checkpoints(tmp_path):
    # early stop: two epochs without improvement, checked before the periodic checkpoint (reference order)
    tr = _FakeTrainer([0.5, 0.4, 0.3, 0.9])
    hist = loop.fit(tr, [(1.0, None)], [(1.0, None)], epochs=4, save_dir=str(tmp_path), patience=2)
    assert [h["epoch"] for h in hist] == [1, 2, 3] and hist[-1]["patience_counter"] == 2
    assert [c[1] for c in tr.calls if c[0] == "save"] == ["best_model.pth", "last_model.pth"]
    # every 10th epoch a model-only checkpoint; no improvement after the first epoch, no patience: runs to the end
    tr = _FakeTrainer([0.5] + [0.1] * 20)
    hist = loop.fit(tr, [(1.0, None)], [(1.0, None)], epochs=21, save_dir=str(tmp_path))
    assert len(hist) == 21
    saves = [c for c in tr.calls if c[0] == "save"]
    assert [s[1] for s in saves] == ["best_model.pth", "checkpoint_epoch10.pth", "checkpoint_epoch20.pth", "last_model.pth"]
    assert saves[1] == ("save", "checkpoint_epoch10.pth", 10, None, False)
    # without a save_dir nothing is written; a dice of 0 never counts as an improvement over the initial 0.0
    tr = _FakeTrainer([0.0, 0.0])
    hist = loop.fit(tr, [(1.0, None)], [(1.0, None)], epochs=2)
    assert not [c for c in tr.calls if c[0] == "save"] and [h["improved"] for h in hist] == [False, False]


def test_fit_with_the_project_scheduler():
    tr = _FakeTrainer([0.1, 0.2, 0.3])
    tr.lr = 1e-4
    sched = CosineAnnealingWarmRestarts(1e-4, T_0=10, T_mult=2)
    ref = CosineAnnealingWarmRestarts(1e-4, T_0=10, T_mult=2)
    hist = loop.fit(tr, [(1.0, None)], [(1.0, None)], epochs=3, scheduler=sched)
    want = [1e-4, ref.step(), ref.step()]
    assert [h["lr"] for h in hist] == want and tr.lr == ref.step()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    # rank 0: two batches, rank 1: one batch; counts beyond float32's exact integers
    own = _acc(tp=(1 << 25) + 1 + rank, fp=3 * rank, fn=5, tn=100 + rank, loss=0.5 + rank, bce=0.25, dl=0.125 * rank,
               dice=0.75 - 0.25 * rank, batches=2 - rank)
    acc = torch.from_numpy(own.copy())
    out = dp.allreduce_accumulators(acc)
    assert out is acc
    local = dp.allreduce_accumulators(torch.from_numpy(own.copy()), dp.LOCAL)     # a trainer that must not communicate
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), own=own, summed=acc.numpy(), local=local.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_accumulator_allreduce_two_ranks(tmp_path):
    world = 2
    mp.spawn(_rank_main, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [np.load(tmp_path / f"rank{i}.npz") for i in range(world)]
    want = r[0]["own"] + r[1]["own"]
    for i in range(world):
        assert np.array_equal(r[i]["summed"], want)
        assert np.array_equal(r[i]["local"], r[i]["own"])
    m0, m1 = SegMetrics(r[0]["summed"]), SegMetrics(r[1]["summed"])
    assert m0.as_dict() == m1.as_dict()
    assert m0.tp == 2 * (1 << 25) + 3 and m0.batches == 3
    assert m0.loss == (0.5 + 1.5) / 3 and m0.dice == (0.75 + 0.5) / 3


def test_accumulator_allreduce_without_a_group_is_the_identity():
    a = torch.arange(16, dtype=torch.float64)
    assert torch.equal(dp.allreduce_accumulators(a.clone()), a)


def test_new_symbols_exported_and_prototyped():
    from unet_lane_detection_amd import _lib
    lib = _lib.load()
    for name in ("unet_train_eval_u8", "unet_train_eval_f32", "unet_seg_metrics_accumulate"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.unet_seg_metrics_accumulate.argtypes) == 13
    assert len(lib.unet_train_eval_u8.argtypes) == 7
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unet_hip.h")) as f:
        header = f.read()
    for name in ("unet_train_eval_u8", "unet_train_eval_f32", "unet_seg_metrics_accumulate"):
        assert f"int {name}(" in header
    assert metrics.NUM_ACCUMULATORS == 16
