"""Gradient accumulation, global-norm clipping, the non-finite guard and the learning-rate range test on the device:
the gradient pass (csrc/grad_kernels.cpp) against its numpy model (tests/grad_model.py), unet_train_adam_step_rec
against unet_train_adam_step, and UNetTrainer / loop.find_lr on top of both."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_model as G
from oracle import unet_oracle as O
from unet_lane_detection_amd import _lib, loop, state as S

pytestmark = pytest.mark.gpu

PAD = 8             # floats around every view: a store outside the view would land in them
SENTINEL = -777.0


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=False)


def _grid(lib):
    return int(lib.unet_grad_work_bytes()) // 16         # one (sum, count) pair of doubles per block


def _host_inputs(numel):
    """a and b with +-inf, NaN, -0, fp32 subnormals and 1e30 among them (as many as numel has room for)"""
    if numel <= 5:
        a = np.array([1e30, np.inf, -0.0, np.nan, 1e-45], dtype=np.float32)[:numel]
        b = np.array([1e30, 1.0, 0.0, 2.0, 1e-45], dtype=np.float32)[:numel]
        return a, b
    rng = np.random.default_rng(numel)
    a = rng.standard_normal(numel).astype(np.float32)
    b = (rng.standard_normal(numel) * 3).astype(np.float32)
    where = np.linspace(0, numel - 1, 12).astype(np.int64)                     # first and last element included
    a[where] = [1e30, np.inf, -np.inf, np.nan, -0.0, 1e-45, -1e-40, 1e30, 3e38, np.inf, 5.0, -1e30]
    b[where] = [1e30, 1.0, 2.0, 3.0, 0.0, 1e-45, 1e-40, -1e30, 3e38, -np.inf, np.nan, 7.0]   # overflow, inf - inf
    return a, b


def _same_bits(got, want):
    """bit for bit; two NaNs count as equal (which NaN an addition returns is the hardware's choice: numpy's host
    gives inf - inf another sign bit than the device does)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | both_nan))


class _View:
    """numel floats on the device, `off` floats behind a 16-byte boundary, sentinels around them"""

    def __init__(self, host, off):
        self.n, self.off = host.size, off
        self.buf = torch.full((PAD + off + self.n + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[PAD + off:PAD + off + self.n]
        self.view.copy_(torch.from_numpy(host))
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * (PAD + off))    # also for numel 0, where the view is empty

    def host(self):
        return self.view.cpu().numpy()

    def intact(self):
        lo, hi = self.buf[:PAD + self.off].cpu().numpy(), self.buf[PAD + self.off + self.n:].cpu().numpy()
        return bool(np.all(lo == SENTINEL) and np.all(hi == SENTINEL))


FORMS = ("add_apart", "add_dst_is_a", "add_dst_is_b", "copy_apart", "reduce")


def _run_form(lib, form, a_h, b_h, offs):
    """one call (two, for the record's repeatability) -> (what dst holds, what a holds, record, views)"""
    oa, ob, od = offs
    a, b = _View(a_h, oa), _View(b_h, ob)
    dst = {"add_apart": None, "copy_apart": None, "add_dst_is_a": a, "add_dst_is_b": b, "reduce": a}[form]
    if dst is None:
        dst = _View(np.full(a_h.size, 123.0, np.float32), od)
    bb = b if form.startswith("add") else None
    work = torch.empty(int(lib.unet_grad_work_bytes()) // 8, dtype=torch.float64, device="cuda")
    recs = []
    for rep in range(2):
        if rep == 1:      # the same call on the same inputs: restore what an aliased first call overwrote
            a.view.copy_(torch.from_numpy(a_h))
            b.view.copy_(torch.from_numpy(b_h))
        rec = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
        rc = lib.unet_grad_accumulate_f32(0, dst.ptr, a.ptr, bb.ptr if bb else None, a_h.size, C.c_void_p(rec.data_ptr()),
                                          C.c_void_p(work.data_ptr()), None)
        assert rc == 0, (form, lib.unet_op_last_error())
        recs.append(rec.cpu().numpy())
    assert recs[0].tobytes() == recs[1].tobytes(), (form, offs, recs)          # bit-identical between two calls
    assert a.intact() and b.intact() and dst.intact(), (form, offs)
    return dst.host(), a.host(), b.host(), recs[0]


@pytest.mark.parametrize("numel", [0, 1, 3, 5, 255, 1025, "grid"])
def test_grad_pass_against_the_model(lib, numel):
    """every form (dst apart / a / b; b given or NULL), base pointers 0..3 floats behind a 16-byte boundary, and - the
    4-byte path - pointers at different distances from it.  dst bit-exact, the count exact, the sum within
    numel * 2^-53 of the exactly rounded one (derived in tests/grad_model.py), the record repeatable."""
    if numel == "grid":
        numel = 2 * _grid(lib) * 256 * 4 + 7          # the grid-stride loop runs more than twice
        assert _grid(lib) == 2048 and numel == 4194311
    a_h, b_h = _host_inputs(numel)
    want = {"add": G.accumulate(a_h, b_h), "copy": G.accumulate(a_h)}
    want_rec = {k: G.record(v) for k, v in want.items()}
    if numel >= 255:
        assert want_rec["add"][1] >= 4 and want_rec["copy"][1] == 4
    # (offset of a, of b, of a dst apart from both); the last two take the 4-byte path: a, b and dst all differ, and a
    # dst that differs from a and b alone.  Forms those two layouts would only repeat are left out.
    layouts = [((o, o, o), FORMS) for o in range(4)]
    layouts += [((0, 2, 1), ("add_apart", "add_dst_is_a", "add_dst_is_b", "copy_apart")),
                ((3, 3, 0), ("add_apart", "copy_apart"))]
    for offs, forms in layouts:
        for form in forms:
            kind = "add" if form.startswith("add") else "copy"
            dst, a_after, b_after, rec = _run_form(lib, form, a_h, b_h, offs)
            assert _same_bits(dst, want[kind]), (form, offs)
            if form in ("add_apart", "copy_apart", "reduce"):
                assert _same_bits(a_after, a_h), (form, offs)                  # a pure reduction stores nothing
            if form != "add_dst_is_b":
                assert _same_bits(b_after, b_h), (form, offs)
            assert rec[1] == want_rec[kind][1], (form, offs, rec)
            assert abs(rec[0] - want_rec[kind][0]) <= G.record_bound(numel) * want_rec[kind][0], (form, offs, rec)
    torch.cuda.synchronize()


def test_grad_pass_without_a_record_and_overwrites_the_record(lib):
    a_h, b_h = _host_inputs(1025)
    a, b, d = _View(a_h, 1), _View(b_h, 1), _View(np.zeros(1025, np.float32), 1)
    assert lib.unet_grad_accumulate_f32(0, d.ptr, a.ptr, b.ptr, 1025, None, None, None) == 0     # no record, no work
    assert _same_bits(d.host(), G.accumulate(a_h, b_h)) and d.intact()
    rec = torch.tensor([1e300, 55.0], dtype=torch.float64, device="cuda")                          # overwritten, not added to
    work = torch.empty(int(lib.unet_grad_work_bytes()) // 8, dtype=torch.float64, device="cuda")
    ones = _View(np.ones(7, np.float32), 0)
    assert lib.unet_grad_accumulate_f32(0, ones.ptr, ones.ptr, None, 7, C.c_void_p(rec.data_ptr()),
                                        C.c_void_p(work.data_ptr()), None) == 0
    assert rec.cpu().tolist() == [7.0, 0.0]


# ---- the trainer ---------------------------------------------------------------------------------------------------
def _tiny(seed=1, **kw):
    from unet_lane_detection_amd.trainer import UNetTrainer
    return UNetTrainer(S.seeded_state_dict([4, 8], seed=seed), device=0, **kw)


def _batch(seed, n=2, h=16, w=16):
    return torch.from_numpy(S.synthetic_frames(n, h, w, seed=seed)), torch.from_numpy(S.synthetic_targets(n, h, w, seed=seed))


def _state(tr):
    torch.cuda.synchronize()
    return [t.clone() for t in (tr.params, tr.exp_avg, tr.exp_avg_sq)]


def _equal(x, y):
    return all(torch.equal(p, q) for p, q in zip(x, y))


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_adam_step_rec_equals_adam_step_with_the_same_multiplier(decoupled):
    """the record path against the existing entry called with the Python-computed coefficient as grad_scale: parameters
    and both moments bit for bit, clipped (max_norm half the measured norm), not clipped, and with max_norm = inf.
    Both trainers first take two plain steps: from zero moments a fused and an unfused multiply-add give the same
    moments, so only an update from non-zero moments tells the two kernels' roundings apart.  Then two compared updates."""
    (x0, t0), (x, t) = _batch(4), _batch(3)
    kw = dict(lr=1e-2, weight_decay=0.01, decoupled=decoupled)

    def warmed(**extra):
        tr = _tiny(**kw, **extra)
        for _ in range(2):
            tr.step(x0, t0)
        assert tr.step_count == 2 and tr._grad_rec is None
        return tr
    probe = warmed()
    assert probe.params.numel() % 4 != 0                 # like the flagship model's: no whole number of 16-byte chunks
    probe.forward_backward(x, t)
    torch.cuda.synchronize()
    norm = float(np.sqrt(G.record(probe.grads.cpu().numpy())[0]))
    assert norm > 0
    probe.release()
    for max_norm, scale in ((norm / 2, 1.0), (norm * 2, 1.0), (None, 1.0), (norm / 8, 0.25)):
        a, b = warmed(), warmed()
        a.max_grad_norm = max_norm
        for update in (3, 4):
            if scale == 1.0 and max_norm is not None:
                a.step(x, t)                             # clipping alone: the pure reduction on the bucket, then the record entry
            else:
                if max_norm is None:
                    a.skip_nonfinite = True              # the guard alone also goes through the record entry
                a.forward_backward(x, t)
                a._grad_pass(a.grads, a.grads, None, record=True)
                a.optimizer_step_rec(scale)
            torch.cuda.synchronize()
            rec = a.grad_record.cpu().numpy()
            model_rec = G.record(a.grads.cpu().numpy())
            assert rec[1] == 0 and abs(rec[0] - model_rec[0]) <= G.record_bound(a.grads.numel()) * model_rec[0]
            coef, scaled_norm = G.coefficient(scale, max_norm, rec[0])
            if update == 3:                              # the norm measured for this very gradient
                assert (float(coef) < scale) == (max_norm is not None and max_norm < scale * norm)
            if max_norm is None:
                assert coef == np.float32(scale)
            if scale == 1.0 and max_norm is not None:
                assert a.grad_norm == scaled_norm and a.skipped_steps == 0
            assert a.step_count == update
            b.forward_backward(x, t)
            assert torch.equal(a.grads, b.grads)
            b.optimizer_step(float(coef))
            assert _equal(_state(a), _state(b)), (max_norm, scale, update)
        assert a.device_error() == 0 and b.device_error() == 0
        a.release()
        b.release()


@pytest.mark.parametrize("checked", [True, False], ids=["checked", "unchecked"])
def test_nonfinite_gradient_leaves_the_state_untouched(checked):
    x, t = _batch(3)
    tr = _tiny(lr=1e-2, skip_nonfinite=True, max_grad_norm=1.0, check_device_status=checked)
    tr.step(x, t)
    before, steps = _state(tr), tr.step_count
    assert steps == 1 and tr.skipped_steps == 0
    tr.forward_backward(x, t)
    tr.grads[5] = float("inf")                           # data, written into the buffer
    tr.apply_update()
    assert _equal(_state(tr), before)                    # parameters and both moments, bit for bit
    assert tr.grad_record.cpu().tolist()[1] == 1.0
    if checked:
        assert tr.skipped_steps == 1 and tr.step_count == steps
    else:                                                # nothing is read: the kernel's own guard did it
        assert tr.skipped_steps == 0 and tr.step_count == steps + 1
    tr.step(x, t)                                        # and the trainer goes on
    assert not _equal(_state(tr), before) and torch.isfinite(tr.params).all()
    assert tr.device_error() == 0
    tr.release()


def _tie_free_batches(sd_t, count, n, h, w):
    """`count` distinct synthetic batches whose train-mode forward keeps every BatchNorm output away from the ReLU kink
    (tests/test_train_gpu.py, _relu_margin: gradient parity is only defined away from those ties).  As _tie_free_frames
    there: the first seeds with a margin above 5e-6, else those with the largest margins among 64 seeds, which must still
    exceed 2e-6.  Finding too few is a hard failure."""
    from test_train_gpu import _relu_margin
    margins = []
    for seed in range(2, 66):
        margins.append((_relu_margin(sd_t, O.normalize_u8_nhwc(S.synthetic_frames(n, h, w, seed=seed))), seed))
        if sum(m > 5e-6 for m, _ in margins) == count:
            break
    best = sorted(margins, reverse=True)[:count]
    if best[-1][0] <= 2e-6:
        pytest.fail(f"fewer than {count} tie-free inputs among 64 seeds: largest margins {best}")
    print("tie-free inputs (margin, seed):", best)
    seeds = sorted(s for _, s in best)
    return [(S.synthetic_frames(n, h, w, seed=s), S.synthetic_targets(n, h, w, seed=s)) for s in seeds]


@pytest.mark.parametrize("feats,shape", [([4, 8], (2, 16, 16)), ([64, 128], (2, 32, 48))], ids=["tiny", "f16x3"])
def test_accumulation_of_three_micro_batches(feats, shape):
    from test_train_gpu import _rel
    from unet_lane_detection_amd.trainer import UNetTrainer
    sdn = S.seeded_state_dict(feats, seed=6)
    sd_t = O.to_torch_state(sdn)
    batches = [(torch.from_numpy(f), torch.from_numpy(t)) for f, t in _tie_free_batches(sd_t, 3, *shape)]
    a = UNetTrainer(sdn, device=0, lr=1e-3, accum_steps=3)
    b = UNetTrainer(sdn, device=0, lr=1e-3)
    for update in (1, 2):        # the second from non-zero moments: only there do the two optimiser kernels' roundings show
        start = _state(a)
        gs = []
        for i, (x, t) in enumerate(batches if update == 1 else batches[::-1]):
            loss = a.step(x, t)
            b.forward_backward(x, t)
            torch.cuda.synchronize()
            assert torch.equal(loss, b.loss)             # the micro-batch's own loss, every call
            gs.append(b.grads.clone())
            if i < 2:
                assert _equal(_state(a), start) and a.step_count == update - 1     # no update before the third call
        assert a.step_count == update and a._pending == 0
        bucket = (gs[0] + gs[1]) + gs[2]                 # fp32, in this order
        assert torch.equal(a.grads, bucket)
        want_norm = float(np.sqrt(G.record(bucket.cpu().numpy())[0])) / 3
        assert abs(a.grad_norm - want_norm) <= (G.record_bound(bucket.numel()) + 2.0 ** -50) * want_norm
        if update == 1:
            # ... whose third is the mean gradient of the three batches (the tolerance of test_mid_config_grads_vs_oracle)
            ref = None
            for x, t in batches:
                _, grads, _, _ = O.loss_and_grads(sd_t, O.normalize_u8_nhwc(x.numpy()), t)
                ref = {k: v.numpy() / 3 if ref is None else ref[k] + v.numpy() / 3 for k, v in grads.items()}
            got = {k: v.detach().cpu().numpy() / 3 for k, v in a.grad_dict().items()}
            worst = max((_rel(got[k], ref[k]), k) for k in ref)
            assert worst[0] < 1e-3, worst
        # the update: a plain unet_train_adam_step with grad_scale 1/3 on that bucket
        b.grads.copy_(bucket)
        b.optimizer_step(1.0 / 3)
        assert _equal(_state(a), _state(b)), update
    assert a.device_error() == 0 and b.device_error() == 0
    a.release()
    b.release()


def test_flush_applies_a_partial_accumulation():
    a, b = _tiny(lr=1e-3, accum_steps=4), _tiny(lr=1e-3)
    gs = []
    for seed in (3, 4):
        x, t = _batch(seed)
        a.step(x, t)
        b.forward_backward(x, t)
        gs.append(b.grads.clone())
    assert a.step_count == 0 and a.flush_accumulation() is True and a.step_count == 1
    assert a.flush_accumulation() is False and a.step_count == 1           # nothing pending: nothing happens
    b.grads.copy_(gs[0] + gs[1])
    b.optimizer_step(0.5)
    assert torch.equal(a.grads, b.grads) and _equal(_state(a), _state(b))
    a.release()
    b.release()


def test_defaults_launch_what_they_always_launched():
    from unet_lane_detection_amd.trainer import UNetTrainer
    x, t = _batch(3)
    names = []
    for kw in ({}, dict(accum_steps=1, max_grad_norm=None, skip_nonfinite=False), dict(max_grad_norm=1.0)):
        tr = UNetTrainer(S.seeded_state_dict([4, 8], seed=1), device=0, **kw)
        tr.profile(True)
        tr.step(x, t)
        torch.cuda.synchronize()
        names.append([r[0] for r in tr.profile_records()])
        tr.profile(False)
        if "max_grad_norm" not in kw or kw["max_grad_norm"] is None:
            assert tr._acc is None and tr._grad_rec is None and tr._grad_work is None      # nothing allocated
        tr.release()
    assert names[0] == names[1] and "adam" in names[0] and "adam_rec" not in names[0]
    assert "adam_rec" in names[2] and "adam" not in names[2]
    assert [n for n in names[2] if n != "adam_rec"] == [n for n in names[0] if n != "adam"]


def test_find_lr_on_the_tiny_configuration():
    tr = _tiny(lr=3e-4)
    x, t = _batch(3)
    tr.step(x, t)                                        # moments and a step count to restore
    before, bn, steps, nbt = _state(tr), tr.bn.clone(), tr.step_count, tr.num_batches_tracked
    batches = [_batch(s) for s in range(3, 15)]
    r = loop.find_lr(tr, batches, init_lr=1e-6, final_lr=1, num_iter=12)
    assert len(r.lrs) == 12 and len(r.losses) == 12 and r.stopped is None
    assert r.lrs[0] == 1e-6 and abs(r.lrs[-1] / 1e-6 ** (1 / 12) - 1) < 1e-9
    assert all(np.isfinite(v) for v in r.losses) or tr.skipped_steps > 0       # finite or skipped, never a ruined trainer
    assert r.recommended is not None and 1e-7 <= r.recommended <= 0.1
    assert _equal(_state(tr), before) and torch.equal(tr.bn, bn)
    assert tr.step_count == steps and tr.lr == 3e-4 and tr.num_batches_tracked == nbt and tr.skip_nonfinite is False
    tr.release()
    # without restore the sweep's updates stay
    tr = _tiny(lr=3e-4)
    r = loop.find_lr(tr, batches[:3], init_lr=1e-6, final_lr=1e-3, num_iter=3, restore=False)
    assert tr.step_count + tr.skipped_steps == 3 and tr.lr == r.lrs[-1]
    tr.release()


def test_snapshot_restore_round_trip():
    a, b = _tiny(lr=1e-2), _tiny(lr=1e-2)
    (x1, t1), (x2, t2), (x3, t3) = _batch(3), _batch(4), _batch(5)
    a.step(x1, t1)
    b.step(x1, t1)
    s = a.snapshot_state()
    a.lr, a.accum_steps = 0.5, 2
    a.step(x3, t3)                                       # pending accumulation ...
    a.accum_steps = 1
    a.step(x3, t3)                                       # ... applied, far away from the snapshot
    assert not torch.equal(a.params, b.params)
    a.restore_state(s)
    assert a.lr == 1e-2 and a.accum_steps == 1 and a.step_count == 1 and _equal(_state(a), _state(b))
    assert torch.equal(a.bn, b.bn)
    a.step(x2, t2)
    b.step(x2, t2)
    assert _equal(_state(a), _state(b)) and torch.equal(a.bn, b.bn) and torch.equal(a.loss, b.loss)
    assert a.num_batches_tracked == b.num_batches_tracked
    assert a.device_error() == 0
    a.release()
    b.release()
