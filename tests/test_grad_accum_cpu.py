"""Gradient accumulation, global-norm clipping and the learning-rate range test, host side: the numpy model
(tests/grad_model.py) discriminates and agrees with torch, the new entry points check their arguments before a device is
touched, and loop.find_lr / loop.fit drive a trainer as documented.  No kernels run here."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import grad_model as G
from unet_lane_detection_amd import _lib, loop


# ---- the model --------------------------------------------------------------------------------------------------
def test_record_model_discriminates():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(4097).astype(np.float32)
    x[1234] = 1e30
    want = G.record(x)
    assert want[1] == 0.0 and math.isfinite(want[0]) and want[0] > 1e59
    assert G.within_bound(want[0], x)
    assert not G.within_bound(G.record_fp32_sum(x), x)             # 1e60 is beyond fp32
    y = (rng.standard_normal(1 << 16) * 1e-3).astype(np.float32)
    y[0] = 64.0
    assert G.within_bound(G.record(y)[0], y)
    assert not G.within_bound(G.record_fp32_sum(y), y)             # fp32 drops the small squares behind 4096
    # a non-finite element is counted and excluded
    z = x.copy()
    z[[3, 77, 4000]] = [np.inf, -np.inf, np.nan]
    rz = G.record(z)
    keep = np.ones(z.size, bool)
    keep[[3, 77, 4000]] = False
    assert rz[1] == 3.0 and rz[0] == G.record(z[keep])[0] and math.isfinite(rz[0])
    assert np.array_equal(G.record(np.zeros(0, np.float32)), [0.0, 0.0])
    # -0 and subnormals are finite; a subnormal's square is a normal double
    s = np.array([-0.0, 1e-45, -1e-40], dtype=np.float32)
    assert G.record(s)[1] == 0.0 and G.record(s)[0] > 0.0


def test_accumulate_model_semantics():
    a = np.array([1.0, 1e30, -0.0, np.inf, 3e38], dtype=np.float32)
    b = np.array([2.0 ** -24, -1e30, 0.0, -np.inf, 3e38], dtype=np.float32)
    d = G.accumulate(a, b)
    assert d.dtype == np.float32 and d[0] == 1.0 and d[1] == 0.0 and np.isnan(d[3]) and np.isinf(d[4])
    c = G.accumulate(a)
    assert c is not a and np.array_equal(c.view(np.uint32), a.view(np.uint32))


@pytest.mark.parametrize("max_norm", [0.05, 1.0, 1e6])
def test_coefficient_is_torchs_clip_grad_norm(max_norm):
    """total norm and coefficient against torch.nn.utils.clip_grad_norm_ on random tensors.  torch forms its norm in
    fp32 with vectorised, pairwise partial sums - an error that grows with log2(n), n <= 2^15 here - so it agrees with
    the double norm within 64 * 2^-24, relative; the clipped gradients then agree within one more fp32 rounding."""
    g = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in ((33, 17), (4099,), (8, 8, 3, 3), (1,))]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g) * 0.01
    flat = torch.cat([p.grad.reshape(-1) for p in params]).numpy().copy()
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    coef, norm = G.coefficient(1.0, max_norm, G.record(flat)[0])
    tol = 64 * 2.0 ** -24
    assert abs(norm - total) <= tol * total
    want = min(1.0, max_norm / (total + 1e-6))
    assert abs(float(coef) - want) <= tol * want
    assert (float(coef) < 1.0) == (max_norm < total)
    clipped = torch.cat([p.grad.reshape(-1) for p in params]).numpy()
    assert np.abs(clipped - flat * coef).max() <= 2 * tol * np.abs(flat).max()


def test_coefficient_scale_and_infinity():
    s = G.record(np.full(100, 0.5, np.float32))[0]                  # norm 5
    for gs in (1.0, 1 / 3, 0.125, -0.25):
        assert G.coefficient(gs, None, s)[0] == np.float32(gs)      # no clipping: the scale itself, exactly
        assert G.coefficient(gs, math.inf, s)[0] == np.float32(gs)
        assert G.coefficient(gs, 1e9, s)[0] == np.float32(gs)
    coef, norm = G.coefficient(0.5, 1.0, s)                         # scaled norm 2.5 -> clipped to 1
    assert abs(norm - 2.5) < 1e-6 and abs(float(coef) - 0.5 / 2.5) < 1e-6
    assert float(G.coefficient(-0.5, 1.0, s)[0]) < 0


@pytest.mark.parametrize("decoupled", [False, True])
def test_clipped_adam_step_model_vs_torch(decoupled):
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(1001, generator=g)
    grad = torch.randn(1001, generator=g) * 0.1
    lr, wd, max_norm = 1e-2, 0.1, 1.0
    p = torch.nn.Parameter(p0.clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p], lr=lr, weight_decay=wd)
    mp, mm, mv = p0.numpy(), np.zeros(1001, np.float32), np.zeros(1001, np.float32)
    for step in (1, 2):
        p.grad = grad.clone() * step
        torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        coef, norm = G.coefficient(1.0, max_norm, G.record(grad.numpy() * step)[0])
        assert norm > max_norm
        mp, mm, mv = G.adam_step(mp, grad.numpy() * step, mm, mv, step, lr, 0.9, 0.999, 1e-8, wd, decoupled, coef)
        # every element moves by about lr; the two agree to a few fp32 roundings of the parameter
        assert np.abs(mp - p.detach().numpy()).max() < 4 * 2.0 ** -23 * max(1.0, float(np.abs(mp).max()))


# ---- the entry points' checks --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_grad_accumulate_checks_arguments_first(lib):
    buf = (C.c_double * 64)()
    base = C.addressof(buf)
    p = lambda off: C.c_void_p(base + off)

    def call(dst=p(0), a=p(0), b=None, numel=8, record=None, work=None, device=1 << 20):
        return lib.unet_grad_accumulate_f32(device, dst, a, b, numel, record, work, None)
    assert lib.unet_grad_work_bytes() >= 2 * 8 and lib.unet_grad_work_bytes() % 16 == 0
    for kwargs in (dict(dst=None), dict(a=None), dict(dst=p(2)), dict(a=p(1)), dict(b=p(130)),       # null, misaligned
                   dict(record=p(256)), dict(record=p(260), work=p(264)), dict(record=p(256), work=p(268)),
                   dict(dst=p(4), a=p(0)), dict(dst=p(32), a=p(64), b=p(40)),                       # partial overlap
                   dict(numel=(1 << 48) + 1)):
        assert call(**kwargs) == 1, kwargs
        assert lib.unet_op_last_error().startswith(b"invalid argument: unet_grad_accumulate_f32"), kwargs
    # what passes the checks reaches the device call, which this ordinal fails: nothing was touched before
    for kwargs in (dict(), dict(dst=p(4), a=p(4)), dict(dst=p(64), a=p(0)), dict(b=p(0)), dict(dst=p(100), a=p(100), b=p(32)),
                   dict(record=p(256), work=p(264)), dict(numel=0, record=p(256), work=p(264))):
        assert call(**kwargs) == 4, kwargs
        assert b"hipSetDevice" in lib.unet_op_last_error()


def test_adam_step_rec_checks_arguments_first(lib):
    cfg = _lib.UnetConfig()
    cfg.in_channels, cfg.out_channels, cfg.depth = 3, 1, 2
    cfg.features[0], cfg.features[1] = 4, 8
    h = C.c_void_p()
    assert lib.unet_create(C.byref(cfg), C.byref(h)) == 0
    rec = (C.c_double * 4)()
    r = C.c_void_p(C.addressof(rec))
    args = (1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0)
    assert lib.unet_train_adam_step_rec(None, *args, 1.0, r, None) == 1
    assert lib.unet_train_adam_step_rec(h, *args, 1.0, r, None) == 1            # no unet_train_attach
    assert lib.unet_train_adam_step_rec(h, *args, 1.0, None, None) == 1
    assert lib.unet_train_adam_step_rec(h, *args, 1.0, C.c_void_p(C.addressof(rec) + 4), None) == 1
    assert lib.unet_destroy(h) == 0


# ---- find_lr and fit on a fake trainer -----------------------------------------------------------------------------
class _Fake:
    def __init__(self, losses, accum_steps=1, raise_at=None):
        self.lr = 123.0
        self.skip_nonfinite = False
        self.accum_steps = accum_steps
        self.calls, self.guard_seen = [], []
        self._losses = list(losses)
        self._raise_at = raise_at

    def step(self, images, targets):
        i = len([c for c in self.calls if c[0] == "step"])
        self.calls.append(("step", images, self.lr))
        self.guard_seen.append(self.skip_nonfinite)
        if self._raise_at is not None and i == self._raise_at[0]:
            raise _lib.UnetError(self._raise_at[1], "fake")
        return torch.tensor([self._losses[i]], dtype=torch.float64)

    def snapshot_state(self):
        self.calls.append(("snapshot",))
        return {"lr": self.lr, "token": 42}

    def restore_state(self, s):
        self.calls.append(("restore", s["token"]))
        self.lr = s["lr"]


def _batches(n):
    return [(i, None) for i in range(n)]


def test_find_lr_rates_and_recommendation():
    losses = [1.0, 0.9, 0.5, float("nan"), 0.2, 0.7, 3.0, float("inf")]
    tr = _Fake(losses)
    r = loop.find_lr(tr, _batches(20), init_lr=1e-6, final_lr=1e-2, num_iter=8)
    mult = (1e-2 / 1e-6) ** (1 / 8)
    want, lr = [], 1e-6
    for _ in range(8):
        want.append(lr)
        lr *= mult                                    # repeated multiplication, as the reference does
    assert r.lrs == want and len(r.losses) == 8 and r.stopped is None
    assert [c[2] for c in tr.calls if c[0] == "step"] == want and [c[1] for c in tr.calls if c[0] == "step"] == list(range(8))
    assert r.recommended == want[4] / 10              # the smallest finite loss; the NaN is never chosen
    assert all(tr.guard_seen) and tr.skip_nonfinite is False      # on for the duration, put back
    assert tr.calls[0] == ("snapshot",) and tr.calls[-1] == ("restore", 42) and tr.lr == 123.0
    # the reference's defaults: 1e-8 -> 10 over 100 iterations
    tr = _Fake([1.0] * 100)
    r = loop.find_lr(tr, _batches(100), restore=False)
    assert len(r.lrs) == 100 and r.lrs[0] == 1e-8 and abs(r.lrs[-1] * (10 / 1e-8) ** 0.01 / 10 - 1) < 1e-9
    assert not any(c[0] in ("snapshot", "restore") for c in tr.calls)
    assert loop.find_lr(_Fake([float("nan")] * 3), _batches(3), num_iter=3).recommended is None


def test_find_lr_stops():
    tr = _Fake([1.0, 0.5, 0.6, 2.1, 0.1])
    r = loop.find_lr(tr, _batches(9), num_iter=5, diverge=4.0)
    assert r.stopped == "diverged" and r.losses == [1.0, 0.5, 0.6, 2.1] and r.recommended == r.lrs[1] / 10
    assert tr.calls[-1][0] == "restore"
    r = loop.find_lr(_Fake([1.0, float("nan"), 0.1]), _batches(9), num_iter=3, diverge=4.0)
    assert r.stopped == "diverged" and len(r.losses) == 2
    r = loop.find_lr(_Fake([1.0, float("nan"), 0.1]), _batches(9), num_iter=3)     # diverge None: to the end
    assert r.stopped is None and len(r.losses) == 3
    tr = _Fake([1.0, 0.5, 0.4], raise_at=(2, _lib.UNET_ERR_RANGE))
    r = loop.find_lr(tr, _batches(9), num_iter=5)
    assert r.stopped == "range" and r.losses == [1.0, 0.5] and tr.calls[-1][0] == "restore" and tr.skip_nonfinite is False
    tr = _Fake([1.0, 0.5, 0.4], raise_at=(1, _lib.UNET_ERR_HIP))
    with pytest.raises(_lib.UnetError):
        loop.find_lr(tr, _batches(9), num_iter=5)
    assert tr.calls[-1][0] == "restore" and tr.skip_nonfinite is False            # also on the way out of an error
    r = loop.find_lr(_Fake([1.0, 0.5, 0.4]), _batches(3), num_iter=5)
    assert r.stopped == "exhausted" and len(r.lrs) == 3


def test_find_lr_one_iteration_is_one_update_under_accumulation():
    tr = _Fake([1.0, 3.0, 0.5, 0.75, 9.0], accum_steps=2)
    r = loop.find_lr(tr, _batches(5), init_lr=1e-4, final_lr=1e-2, num_iter=4)
    assert r.losses == [2.0, 0.625] and r.stopped == "exhausted"                    # the fifth batch has no partner
    steps = [c for c in tr.calls if c[0] == "step"]
    assert [c[2] for c in steps[:4]] == [r.lrs[0], r.lrs[0], r.lrs[1], r.lrs[1]]


class _FitFake:
    def __init__(self, with_flush):
        self.lr = 1e-3
        self.calls = []
        if with_flush:
            self.flush_accumulation = lambda: self.calls.append("flush")
            self.grad_norm, self.skipped_steps = 0.25, 2

    def step(self, images, targets):
        self.calls.append("step")
        return torch.tensor([1.0])

    def validate(self, batches):
        self.calls.append("validate")
        return type("V", (), {"dice": 0.5, "loss": 0.5})()


def test_fit_flushes_the_accumulation_once_per_epoch():
    tr = _FitFake(True)
    hist = loop.fit(tr, _batches(3), _batches(1), epochs=2)
    assert tr.calls == ["step"] * 3 + ["flush", "validate"] + ["step"] * 3 + ["flush", "validate"]
    assert all(h["grad_norm"] == 0.25 and h["skipped_steps"] == 2 for h in hist)
    tr = _FitFake(False)
    hist = loop.fit(tr, _batches(3), _batches(1), epochs=1)
    assert tr.calls == ["step"] * 3 + ["validate"] and "grad_norm" not in hist[0] and "skipped_steps" not in hist[0]
