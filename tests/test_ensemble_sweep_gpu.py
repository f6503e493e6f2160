"""The ensemble combine and the threshold sweep on the GPU (csrc/ensemble_kernels.cpp through the C ABI,
unet_lane_detection_amd/ensemble.py, metrics.py) against their numpy models (ensemble.combine_model, metrics.sweep_model).
Every comparison is exact: the sweep is integer, the combine is held to stated fp32 arithmetic."""
import ctypes as C

import numpy as np
import pytest
import torch

import video_model as VM
from unet_lane_detection_amd import _lib, ensemble as E, metrics as M, state as S
from unet_lane_detection_amd import video as V

pytestmark = pytest.mark.gpu

# one element; less than a wave, odd, no multiple of 4; three blocks of four rounds each on the 16-byte path; the same
# with a tail element; 25 blocks with a partly filled last round
NUMELS = [1, 63, 7 * 9, 3 * 64 * 64, 3 * 64 * 64 + 1, 2 * 224 * 224]
GUARD = 16      # floats of canary on either side of every device buffer


@pytest.fixture(scope="module")
def lib():
    return _lib.load(build_if_missing=False)


class FBuf:
    """`n` elements of `dtype` at element `lead` of a larger canary-filled device buffer: lead = 16 floats (or 16 bytes)
    keeps the view 16-byte aligned, one more puts it one element off."""

    def __init__(self, n, dtype, lead=GUARD, data=None):
        self.canary = 0x5A if dtype == torch.uint8 else -777.0
        self.whole = torch.full((lead + n + GUARD,), self.canary, dtype=dtype, device="cuda")
        self.view = self.whole[lead:lead + n]
        self.lead, self.n = lead, n
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)))

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def numpy(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        w = self.whole.cpu().numpy()
        return bool((w[:self.lead] == self.canary).all() and (w[self.lead + self.n:] == self.canary).all())


# ---- combine: kernel against model -------------------------------------------------------------------------------

def member_planes(rng, k, numel, thr):
    """K planes of random fp32 in [0, 1] with exact 0 and 1, denormals and a NaN planted, and - where the plane is
    large enough - elements whose weighted mean is exactly the threshold"""
    ps = [rng.random(numel).astype(np.float32) for _ in range(k)]
    if numel >= 63:
        for j, p in enumerate(ps):
            p[1 + j] = 0.0
            p[11 + j] = 1.0
            p[21 + j] = np.float32(1e-45) * (j + 1)            # denormals
            p[31 + j] = np.float32(1e-39)
        ps[k - 1][41] = np.nan
        for i in (50, 51, 62):                                   # every member equal to thr ...
            for p in ps:
                p[i] = thr
        ps[0][51] = np.nextafter(np.float32(thr), np.float32(1))
    return ps


def run_combine(lib, ps, weights, thr, numel, want_probs=True, want_mask=True, lead=GUARD):
    k = len(ps)
    bufs = [FBuf(numel, torch.float32, lead, p) for p in ps]
    out = FBuf(numel, torch.float32, lead) if want_probs else None
    mask = FBuf(numel, torch.uint8, lead) if want_mask else None
    ptrs = (C.c_void_p * k)(*[b.view.data_ptr() for b in bufs])
    w = None if weights is None else (C.c_float * k)(*[float(v) for v in weights])
    rc = lib.unet_ensemble_combine(0, ptrs, k, w, numel, float(thr), out.ptr() if out else None,
                                   mask.ptr() if mask else None, None)
    assert rc == 0, lib.unet_op_last_error()
    for i in range(k):                                           # consumed before the call returned
        ptrs[i] = None
    torch.cuda.synchronize()
    for b, p in zip(bufs, ps):
        assert b.guards_intact() and np.array_equal(b.numpy().view(np.uint32), p.view(np.uint32))
    assert (out is None or out.guards_intact()) and (mask is None or mask.guards_intact())
    return (out.numpy() if out else None), (mask.numpy() if mask else None)


def same_bits(a, b):
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


@pytest.mark.parametrize("numel", NUMELS)
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_combine_against_model(lib, k, numel):
    rng = np.random.default_rng(1000 * k + numel)
    thr = np.float32(0.5)
    for weights in (None, E.normalise_weights(np.arange(1, k + 1) ** 1.5, k)):
        ps = member_planes(rng, k, numel, thr)
        want, want_mask = E.combine_model(ps, weights, thr)
        got, got_mask = run_combine(lib, ps, weights, thr, numel)
        assert same_bits(got, want), f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {numel} differ"
        assert np.array_equal(got_mask, want_mask) and set(np.unique(got_mask)) <= {0, 255}
        if numel >= 63:
            assert np.isnan(want[41]) and want_mask[41] == 0     # a NaN gives 0


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_combine_mean_equal_to_the_threshold_gives_zero(lib, k):
    """weights 1/k with k a power of two and members all equal to thr: acc == thr exactly, which is not above it"""
    thr, numel = np.float32(0.5), 200
    ps = [np.full(numel, thr, dtype=np.float32) for _ in range(k)]
    ps[0][100:] = np.nextafter(thr, np.float32(1))               # one ulp up in one member: above for k = 1 only ...
    ps[0][150:] = np.float32(0.75)                               # ... and clearly above
    want, want_mask = E.combine_model(ps, None, thr)
    assert (want[:100] == thr).all() and (want_mask[:100] == 0).all() and (want_mask[150:] == 255).all()
    got, got_mask = run_combine(lib, ps, None, thr, numel)
    assert same_bits(got, want) and np.array_equal(got_mask, want_mask)


@pytest.mark.parametrize("numel", [63, 3 * 64 * 64 + 1])
def test_combine_misaligned_views_and_single_outputs(lib, numel):
    rng = np.random.default_rng(numel)
    thr = np.float32(0.4)
    w = E.normalise_weights([3, 1, 2], 3)
    ps = member_planes(rng, 3, numel, thr)
    want, want_mask = E.combine_model(ps, w, thr)
    for lead in (GUARD, GUARD + 1):                              # one float (one mask byte) into the allocation
        got, got_mask = run_combine(lib, ps, w, thr, numel, lead=lead)
        assert same_bits(got, want) and np.array_equal(got_mask, want_mask)
        only, none = run_combine(lib, ps, w, thr, numel, want_mask=False, lead=lead)
        assert none is None and same_bits(only, want)
        none, only_mask = run_combine(lib, ps, w, thr, numel, want_probs=False, lead=lead)
        assert none is None and np.array_equal(only_mask, want_mask)


# ---- sweep: kernel against model ---------------------------------------------------------------------------------

def thresholds_of(t):
    if t == 1:
        return np.array([0.5], dtype=np.float32)
    if t == 2:
        return np.array([-np.inf, np.inf], dtype=np.float32)
    if t == 19:
        return np.array(M.DEFAULT_THRESHOLDS, dtype=np.float32)
    return np.linspace(0.0, 1.0, t).astype(np.float32)


def sweep_inputs(rng, numel, th, u8):
    s = rng.random(numel).astype(np.float32)
    plant = [v for v in th if np.isfinite(v)] + [np.nan, np.inf, -np.inf]
    if numel > 2 * len(plant):
        pos = rng.choice(numel, size=2 * len(plant), replace=False)
        s[pos] = np.array(plant + plant, dtype=np.float32)
    elif numel == 1:
        s[0] = th[0]
    truth = rng.random(numel) < 0.3
    if numel > 2 * len(plant):
        truth[pos[:len(plant)]], truth[pos[len(plant):]] = True, False   # every planted value in both classes
    if u8:
        t = np.where(truth, np.where(rng.random(numel) < 0.5, 255, 1), 0).astype(np.uint8)
    else:
        t = truth.astype(np.float32)
    return s, t


def run_sweep(lib, s, t, th, counts=None, lead=GUARD):
    u8 = t.dtype == np.uint8
    sb = FBuf(s.size, torch.float32, lead, s)
    tb = FBuf(t.size, torch.uint8 if u8 else torch.float32, lead, t)
    if counts is None:
        counts = torch.zeros(2 * (len(th) + 1) + 2 * GUARD, dtype=torch.int64, device="cuda")
    body = counts[GUARD:GUARD + 2 * (len(th) + 1)]
    host_t = np.ascontiguousarray(th, dtype=np.float32).copy()
    rc = lib.unet_score_sweep_accumulate(0, sb.ptr(), tb.ptr(), int(u8), s.size, host_t.ctypes.data_as(C.POINTER(C.c_float)),
                                         len(th), C.c_void_p(body.data_ptr()), None)
    host_t[:] = np.nan                                           # consumed before the call returned
    assert rc == 0, lib.unet_op_last_error()
    torch.cuda.synchronize()
    assert sb.guards_intact() and tb.guards_intact()
    c = counts.cpu().numpy()
    assert not c[:GUARD].any() and not c[GUARD + 2 * (len(th) + 1):].any()
    return counts, c[GUARD:GUARD + 2 * (len(th) + 1)].reshape(2, len(th) + 1)


@pytest.mark.parametrize("numel", NUMELS)
@pytest.mark.parametrize("t", [1, 2, 19, 64])
@pytest.mark.parametrize("u8", [False, True], ids=["float_targets", "byte_targets"])
def test_sweep_against_model(lib, t, numel, u8):
    rng = np.random.default_rng(100 * t + numel + int(u8))
    th = thresholds_of(t)
    s, tg = sweep_inputs(rng, numel, th, u8)
    want = M.sweep_model(s, tg, th)
    assert want.sum() == numel
    counts, got = run_sweep(lib, s, tg, th)
    assert np.array_equal(got, want), (got, want)
    # a second batch into the same counters adds
    s2, tg2 = sweep_inputs(rng, numel, th, u8)
    _, got2 = run_sweep(lib, s2, tg2, th, counts=counts)
    assert np.array_equal(got2, want + M.sweep_model(s2, tg2, th))


@pytest.mark.parametrize("combine", [1, 0], ids=["wave_combined", "per_lane"])
@pytest.mark.parametrize("u8", [False, True], ids=["float_targets", "byte_targets"])
def test_sweep_variants_contention_spread_and_misaligned(lib, combine, u8):
    prev = lib.unet_set_sweep_combine(combine)
    try:
        th = thresholds_of(19)
        rng = np.random.default_rng(7 + combine)
        for numel in (63, 3 * 64 * 64 + 1):
            # the contention case: every score below t_0, every target 0 - one counter takes everything
            s = (rng.random(numel) * 0.04).astype(np.float32)
            tg = np.zeros(numel, dtype=np.uint8 if u8 else np.float32)
            _, got = run_sweep(lib, s, tg, th)
            want = np.zeros((2, 20), dtype=np.int64)
            want[0, 0] = numel
            assert np.array_equal(got, want) and np.array_equal(M.sweep_model(s, tg, th), want)
            # the spread case: scores uniform over all bins, both classes
            s, tg = sweep_inputs(rng, numel, th, u8)
            want = M.sweep_model(s, tg, th)
            assert (want > 0).all() or numel < 100
            for lead in (GUARD, GUARD + 1):                      # and a view one element into its allocation
                _, got = run_sweep(lib, s, tg, th, lead=lead)
                assert np.array_equal(got, want)
    finally:
        lib.unet_set_sweep_combine(prev)


def test_sweep_accumulate_binding_and_lane_like_input(lib):
    """metrics.sweep_accumulate on torch tensors, on the input the kernel is built for: 8.5 % confident positives,
    the rest confident negatives"""
    n = 2 * 224 * 224
    tg = S.synthetic_targets(2, 224, 224, seed=3)
    rng = np.random.default_rng(4)
    s = np.where(tg.reshape(-1) > 0, 0.97, 0.01).astype(np.float32) + (rng.random(n).astype(np.float32) - 0.5) * 0.01
    th = M.sweep_thresholds(M.DEFAULT_THRESHOLDS)
    counts = torch.zeros(40, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for targets in (torch.from_numpy(tg), torch.from_numpy((tg * 255).astype(np.uint8))):
        M.sweep_accumulate(lib, 0, torch.from_numpy(s).cuda().view(2, 1, 224, 224), targets, th, counts, stream)
    want = M.sweep_model(s, tg, th)
    assert np.array_equal(counts.cpu().numpy().reshape(2, 20), 2 * want)
    sw = M.ThresholdSweep(th, want)
    assert sw.best()[1] == 1.0 and sw.at(0.5)["tp"] == int(tg.sum())
    with pytest.raises(ValueError):
        M.sweep_accumulate(lib, 0, torch.zeros(8, device="cuda"), torch.zeros(9), th, counts, stream)
    with pytest.raises(ValueError):
        M.sweep_accumulate(lib, 0, torch.zeros(8, device="cuda"), torch.zeros(8), th, counts[:10], stream)


# ---- sweep against the existing metrics pass -----------------------------------------------------------------------

def counts_of(sw, p):
    at = sw.at(p)
    return at["tp"], at["fp"], at["fn"], at["tn"]


def test_sweep_vs_evaluate_float_tier():
    from unet_lane_detection_amd.model import UNetHIP
    model = UNetHIP(S.seeded_state_dict([8, 16]), device=0)
    frames = torch.from_numpy(S.synthetic_frames(6, 64, 64))
    targets = torch.from_numpy(S.synthetic_targets(6, 64, 64))
    sw = model.sweep(frames, targets, precision="fp32", batch=4)           # two batches accumulate
    assert sw.domain == "logit" and len(sw) == 19 and sw.pixels == 6 * 64 * 64
    for p in (0.5, 0.3, 0.95):
        m = model.evaluate(frames, targets, precision="fp32", threshold=p)
        assert counts_of(sw, p) == (m.tp, m.fp, m.fn, m.tn), p
        assert sw.at(p)["iou"] == m.iou and sw.at(p)["f1"] == m.f1
    # byte targets, float input, another list of thresholds
    img = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 3, 32, 32)).astype(np.float32))
    tg = torch.from_numpy((S.synthetic_targets(2, 32, 32, seed=1) * 255).astype(np.uint8))
    sw = model.sweep(img, tg, thresholds=[0.2, 0.5])
    m = model.evaluate(img, tg, threshold=0.2)
    assert counts_of(sw, 0.2) == (m.tp, m.fp, m.fn, m.tn)
    assert model.device_error() == 0
    model.release()


@pytest.fixture(scope="module")
def int8_net():
    from unet_lane_detection_amd import quant
    from unet_lane_detection_amd.int8 import UNetInt8, calibrate
    from unet_lane_detection_amd.model import UNetHIP
    sdn = S.seeded_state_dict([32, 64, 128], seed=0)
    fm = UNetHIP(sdn, device=0)
    ranges = calibrate(fm, torch.from_numpy(S.synthetic_frames(6, 64, 64, seed=1)), batch=4)
    fm.release()
    net = UNetInt8(quant.quantize_model(sdn, ranges), device=0)
    yield net
    net.release()


def test_sweep_vs_evaluate_int8_tier(int8_net):
    frames = torch.from_numpy(S.synthetic_frames(6, 64, 64))
    targets = torch.from_numpy(S.synthetic_targets(6, 64, 64))
    sw = int8_net.sweep(frames, targets, batch=4)
    for p in (0.5, 0.4):
        m = int8_net.evaluate(frames, targets, threshold=p)
        assert counts_of(sw, p) == (m.tp, m.fp, m.fn, m.tn), p


def test_sweep_vs_validate_trainer():
    from unet_lane_detection_amd.trainer import UNetTrainer
    tr = UNetTrainer(S.seeded_state_dict([8, 16], seed=6), device=0, lr=1e-3)
    tr.step(torch.from_numpy(S.synthetic_frames(2, 32, 48, seed=20)), torch.from_numpy(S.synthetic_targets(2, 32, 48, seed=20)))
    batches = [(torch.from_numpy(S.synthetic_frames(2, 32, 48, seed=40 + i)),
                torch.from_numpy(S.synthetic_targets(2, 32, 48, seed=40 + i))) for i in range(2)]
    before = tr.params.clone()
    sw = tr.sweep(batches)
    assert torch.equal(tr.params, before)
    for p in (0.5, 0.65):
        m = tr.validate(batches, threshold=p)
        assert counts_of(sw, p) == (m.tp, m.fp, m.fn, m.tn), p
    assert sw.pixels == m.pixels
    tr.release()


# ---- the ensemble ------------------------------------------------------------------------------------------------

# seeds 3, 4, 6 of seeded_state_dict([8, 16]) on ENS_FRAMES: the float oracle's logits stay at least 3.7e-4 away from 0
# (checked on the CPU: min |logit| = 3.7e-4, 5.2e-4, 4.2e-4), three orders above the 2.4e-7 inside which sigmoid rounds
# to exactly 0.5 in fp32 - so no member probability is exactly 0.5 and a member's mask equals its ensemble-of-one's
ENS_SEEDS = (3, 4, 6)


def ens_frames():
    return torch.from_numpy(S.synthetic_frames(3, 48, 64, seed=7)).cuda()


@pytest.fixture(scope="module")
def three_models():
    from unet_lane_detection_amd.model import UNetHIP
    models = [UNetHIP(S.seeded_state_dict([8, 16], seed=s), device=0) for s in ENS_SEEDS]
    yield models
    for m in models:
        m.release()


@pytest.mark.parametrize("weights", [None, (0.5, 0.2, 0.3)], ids=["equal", "weighted"])
def test_ensemble_run_against_model(three_models, weights):
    frames = ens_frames()
    ens = E.Ensemble([(m, "fp32") for m in three_models], weights=weights)
    assert len(ens) == 3 and ens.weights.dtype == np.float32
    own = [m.run_u8(frames, return_probs=True, precision="fp32")[1].cpu().numpy() for m in three_models]
    want, want_mask = E.combine_model(own, None if weights is None else ens.weights, 0.45)
    probs, mask = ens.run_u8(frames, return_mask=True, threshold=0.45)
    assert probs.shape == (3, 1, 48, 64) and mask.shape == (3, 48, 64) and mask.dtype == torch.uint8 and probs.is_cuda
    assert np.array_equal(probs.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(mask.cpu().numpy(), want_mask[:, 0])
    assert torch.equal(ens.run_u8(frames), probs)                # without the mask: the probabilities alone
    assert ens.device_error() == 0
    # float input: the members' forward
    img = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 3, 32, 32)).astype(np.float32)).cuda()
    own = [m.forward(img, return_probs=True, precision="fp32")[1].cpu().numpy() for m in three_models]
    want, want_mask = E.combine_model(own, None if weights is None else ens.weights, 0.5)
    probs, mask = ens.forward(img, return_mask=True)
    assert np.array_equal(probs.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(mask.cpu().numpy(), want_mask[:, 0])
    ens.release()                                                # owns nothing: the members stay alive
    assert three_models[0].run_u8(frames).shape == (3, 1, 48, 64)


def test_ensemble_of_one_is_its_member(three_models):
    frames = ens_frames()
    for m in three_models:
        _, own, own_mask = m.run_u8(frames, return_probs=True, return_mask=True, precision="fp32")
        probs, mask = E.Ensemble([(m, "fp32")]).run_u8(frames, return_mask=True)
        assert np.array_equal(probs.cpu().numpy().view(np.uint32), own.cpu().numpy().view(np.uint32))
        assert int((own == 0.5).sum()) == 0                      # see ENS_SEEDS
        assert torch.equal(mask, own_mask)


def test_ensemble_from_checkpoints(tmp_path):
    from unet_lane_detection_amd.model import UNetHIP
    frames = ens_frames()
    paths = []
    for s in ENS_SEEDS[:2]:
        p = str(tmp_path / f"epoch_{s}.npz")
        np.savez(p, **S.seeded_state_dict([8, 16], seed=s))
        paths.append(p)
    first = UNetHIP.from_checkpoint(paths[0])
    _, own, own_mask = first.run_u8(frames, return_probs=True, return_mask=True, precision="fp32")
    one = E.Ensemble.from_checkpoints(paths[:1], precision="fp32")
    probs, mask = one.run_u8(frames, return_mask=True)
    assert torch.equal(probs, own) and torch.equal(mask, own_mask)
    two = E.Ensemble.from_checkpoints(paths, precision="fp32")
    second = UNetHIP.from_checkpoint(paths[1])
    want, _ = E.combine_model([own.cpu().numpy(), second.run_u8(frames, return_probs=True)[1].cpu().numpy()], None, 0.5)
    assert np.array_equal(two.run_u8(frames).cpu().numpy(), want)
    owned = list(two._owned)
    two.release()
    one.release()
    assert all(m._h is None for m in owned)
    with pytest.raises(RuntimeError):
        two.run_u8(frames)
    first.release()
    second.release()


def test_mixed_ensemble_f16x3_and_int8(int8_net):
    from unet_lane_detection_amd.int8 import UNetInt8
    from unet_lane_detection_amd.model import UNetHIP
    fm = UNetHIP(S.seeded_state_dict([64, 128], seed=2), device=0)
    frames = torch.from_numpy(S.synthetic_frames(2, 64, 64, seed=1)).cuda()
    ens = E.Ensemble([fm, int8_net], weights=[2, 1])             # a bare UNetHIP runs on f16x3
    assert ens.members[0][1] == "f16x3" and isinstance(ens.members[1][0], UNetInt8)
    own = [fm.run_u8(frames, return_probs=True, precision="f16x3")[1].cpu().numpy(),
           int8_net.run_u8(frames, return_probs=True)[1].cpu().numpy()]
    want, want_mask = E.combine_model(own, ens.weights, 0.5)
    probs, mask = ens.run_u8(frames, return_mask=True)
    assert np.array_equal(probs.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(mask.cpu().numpy(), want_mask[:, 0])
    assert ens.device_error(current_stream_only=True) == 0
    with pytest.raises(TypeError):
        ens.forward(torch.zeros(1, 3, 64, 64))
    with pytest.raises(TypeError):
        E.Ensemble([object()])
    with pytest.raises(ValueError):
        E.Ensemble([fm] * 9)
    fm.release()


def test_ensemble_evaluate_against_model(three_models):
    ens = E.Ensemble([(m, "fp32") for m in three_models], weights=[1, 1, 2])
    frames = torch.from_numpy(S.synthetic_frames(5, 48, 64, seed=9))
    targets = torch.from_numpy(S.synthetic_targets(5, 48, 64, seed=9, p=0.3))
    sw = ens.evaluate(frames, targets, batch=2)                  # 2 + 2 + 1 frames
    probs = np.concatenate([ens.run_u8(frames[i:i + 2].cuda()).cpu().numpy() for i in (0, 2, 4)])   # the same batches
    want = M.sweep_model(probs, targets.numpy(), np.array(M.DEFAULT_THRESHOLDS, dtype=np.float32))
    assert sw.domain == "probability" and np.array_equal(sw.counts, want) and sw.pixels == 5 * 48 * 64
    tp = int(((probs > np.float32(0.5)) & (targets.numpy() != 0)).sum())
    assert sw.at(0.5)["tp"] == tp
    p, v, j = sw.best("iou")
    assert v == sw.iou.max() and p == M.DEFAULT_THRESHOLDS[j]


def test_frame_pipeline_takes_an_ensemble(three_models):
    ens = E.Ensemble([(m, "fp32") for m in three_models])
    pipe = V.FramePipeline(ens, threshold=0.5, input_size=(32, 32))
    assert pipe.precision is None                                # the path a UNetInt8 takes
    frames = np.random.default_rng(14).integers(0, 256, (2, 48, 64, 3)).astype(np.uint8)
    overlay, mask = pipe.process(frames)
    small = VM.resize_batch(frames, 32, 32, swap_rb=True)
    own = ens.run_u8(torch.from_numpy(small).cuda(), return_mask=True)[-1].cpu().numpy()
    assert 0 < own.mean() < 255                                  # both classes are present
    ref, ref_m = VM.overlay_batch(frames, own, V.jet_table(), 0.7, 0.3, 0.0)
    assert np.array_equal(mask.cpu().numpy(), ref_m) and np.array_equal(overlay.cpu().numpy(), ref)
