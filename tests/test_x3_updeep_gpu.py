"""The f16x3 decoder's split step on the deep levels: kernel 1 (csrc/upconv_x3_win.h) forms P - the transposed
convolution folded into the up half of the 3x3 convolution, a 2 x 2-tap window convolution of the low-resolution x per
output parity, plus the border-class constant - into the up half of the concat buffer; kernel 2 (the addend epilogue of
csrc/conv_x3_t448.h) runs the 3x3 convolution over the skip half and adds P.

P is held to the float64 model and bound of tests/x3_model.py (every element: 2^-21 |r| + 2^-24 + 2^-15 |s| B), the pair
to the CPU oracle's upconv2x2 -> cat -> conv3x3 at the composed operator's bound (2e-5 of the output's range,
tests/test_x3_compose_gpu.py), the network to its two-kernel path (1e-4 on the logits).  Shapes: the smallest that reach
every branch - one 224-pixel item, a ragged last item, frame borders inside an item, the 28-wide instance, f = 512."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import x3_model as M
from oracle import unet_oracle as O
from unet_lane_detection_amd import state as S
from x3_gpu_helpers import SENTINEL, Planes, _h, _p, seed_of, to_dev

pytestmark = pytest.mark.gpu

# (n, h, w, f): h x w is the low-resolution map of x
CASES = [(1, 4, 14, 256), (1, 6, 14, 256), (3, 14, 14, 256), (2, 6, 28, 256), (1, 4, 14, 512)]


@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    return _lib.load(build_if_missing=False)


_cache = {}


def _case(lib, n, h, w, f):
    """parameters, planes and the float64 composition of one case, made once"""
    key = (n, h, w, f)
    if key in _cache:
        return _cache[key]
    g = torch.Generator().manual_seed(seed_of("updeep", *key))
    wt = (torch.randn(2 * f, f, 2, 2, generator=g) * (1.0 / (2 * f)) ** 0.5).float()
    bt = (torch.randn(f, generator=g) * 4.0).float()                  # non-zero: all nine border classes differ
    w3 = (torch.randn(f, 2 * f, 3, 3, generator=g) * (2.0 / (18 * f)) ** 0.5).float()
    scale = torch.rand(f, generator=g) + 0.5
    shift = torch.randn(f, generator=g) * 0.3
    x_act = torch.pow(2.0, torch.randint(-2, 3, (2 * f,), generator=g).float())
    s_act = torch.pow(2.0, torch.randint(-2, 3, (f,), generator=g).float())
    xh, xl = M.split_f16(torch.randn(n, h, w, 2 * f, generator=g) * x_act)
    sh, sl = M.split_f16(torch.randn(n, 2 * h, 2 * w, f, generator=g) * s_act)
    wp = np.zeros((4, f, 2 * f, 2, 2), dtype=np.float64)
    bias = np.zeros((9, f), dtype=np.float64)
    keep = [np.ascontiguousarray(a.numpy(), dtype=np.float32) for a in (wt, bt, w3)]
    assert lib.unet_host_compose_upcat(*[C.c_void_p(k.ctypes.data) for k in keep], f, C.c_void_p(wp.ctypes.data),
                                       C.c_void_p(bias.ctypes.data)) == 0
    _cache[key] = dict(wt=wt, bt=bt, w3=w3, scale=scale, shift=shift, x_act=x_act, s_act=s_act, xh=xh, xl=xl, sh=sh, sl=sl,
                       wp=torch.from_numpy(wp), bias=torch.from_numpy(bias))
    return _cache[key]


def _classes(h, w):
    rc = torch.ones(2 * h, dtype=torch.long)
    rc[0], rc[-1] = 0, 2
    cc = torch.ones(2 * w, dtype=torch.long)
    cc[0], cc[-1] = 0, 2
    return rc[:, None] * 3 + cc[None, :]


def _window(x, k4, h, w):
    """x (N,C,h,w) float64, k4 [4][co][ci][2][2] -> (N,co,2h,2w): per parity the 2 x 2 taps, zero outside the image"""
    out = torch.zeros(x.shape[0], k4.shape[1], 2 * h, 2 * w, dtype=torch.float64)
    xp = F.pad(x, (1, 1, 1, 1))
    for a in range(2):
        for b in range(2):
            out[:, :, a::2, b::2] = F.conv2d(xp, k4[a * 2 + b])[:, :, a:a + h, b:b + w]
    return out


def _model_P(c, n, h, w, f):
    """float64 model of kernel 1 with the host steps of pack_updeep_x3: w' = fp32(W') / act, pre per output channel over
    parities, channels and taps, w_hi / w_lo, three products, B; s = 1 / pre (no magnitude estimate: P's scale is 1),
    t = fp32(class constant) -> r, s, B as (N,2h,2w,f)"""
    wx = c["wp"].float() / c["x_act"][None, None, :, None, None]
    pre = M.prescale_pow2(wx.abs().amax(dim=(0, 2, 3, 4)))
    v = wx * pre[None, :, None, None, None]
    w_hi = v.half()
    w_lo = (v - w_hi.float()).half()
    w_hi, w_lo = w_hi.double(), w_lo.double()
    xh, xl = c["xh"].double().permute(0, 3, 1, 2), c["xl"].double().permute(0, 3, 1, 2)
    z = _window(xh, w_hi + w_lo, h, w) + _window(xl, w_hi, h, w)
    xt, wt_ = xh + xl, w_hi + w_lo
    B = _window(xt * xt, wt_ * wt_, h, w).sqrt()
    s = (1.0 / pre).double()
    t = c["bias"].float().double()[_classes(h, w)].permute(2, 0, 1)[None]
    r = (z * s[None, :, None, None] + t).clamp(-M.F16_MAX, M.F16_MAX)
    return r.permute(0, 2, 3, 1), s, B.permute(0, 2, 3, 1)


@pytest.mark.parametrize("n,h,w,f", CASES)
def test_window_kernel_against_the_float64_model(lib, n, h, w, f):
    c = _case(lib, n, h, w, f)
    xd, x_lo = to_dev(c["xh"], c["xl"])
    y = Planes(n, 2 * h, 2 * w, 2 * f)                                  # a concat buffer: P goes to channels [f, 2f)
    rng = (C.c_int * 1)(-1)
    rc = lib.unet_op_updeep_window_x3_planes(0, _p(xd), x_lo, n, h, w, f, _h(c["wt"]), _h(c["bt"]), _h(c["w3"]),
                                             _h(c["x_act"]), y.ptr, y.lo_off, 2 * f, f, rng, None)
    assert rc == 0
    assert rng[0] == 0
    y.assert_written_only(f, 2 * f, f"window {n}x{h}x{w} f{f}")         # guards and the skip half untouched
    r, s, B = _model_P(c, n, h, w, f)
    hi, lo = y.halves(f, 2 * f)
    M.check(hi, lo, r, s, B, f"upconv2x2_win n{n} {h}x{w} f{f}")


@pytest.mark.parametrize("n,h,w,f", CASES)
def test_pair_against_the_oracle(lib, n, h, w, f):
    c = _case(lib, n, h, w, f)
    xd, x_lo = to_dev(c["xh"], c["xl"])
    x = ((c["xh"].double() + c["xl"].double()) / c["x_act"].double()).float().permute(0, 3, 1, 2)
    skip = ((c["sh"].double() + c["sl"].double()) / c["s_act"].double()).float().permute(0, 3, 1, 2)
    up = O.upconv2x2(x, c["wt"], c["bt"])
    pre = O.conv3x3(torch.cat([skip, up], 1), c["w3"]) * c["scale"][None, :, None, None] + c["shift"][None, :, None, None]
    for relu in (1, 0):
        ref = (torch.relu(pre) if relu else pre).permute(0, 2, 3, 1)
        cat = Planes(n, 2 * h, 2 * w, 2 * f)
        ch, cl = cat.bits(0, f)
        ch.copy_(c["sh"].view(torch.int16).cuda())
        cl.copy_(c["sl"].view(torch.int16).cuda())
        before = cat.buf.clone()
        out = Planes(n, 2 * h, 2 * w, f)
        rng = (C.c_int * 1)(-1)
        rc = lib.unet_op_updeep_conv3x3_x3_planes(0, _p(xd), x_lo, n, h, w, f, _h(c["wt"]), _h(c["bt"]), _h(c["w3"]),
                                                  _h(c["scale"]), _h(c["shift"]), relu, _h(c["x_act"]), _h(c["s_act"]),
                                                  cat.ptr, cat.lo_off, out.ptr, out.lo_off, rng, None)
        assert rc == 0
        assert rng[0] == 0
        label = f"pair n{n} {h}x{w} f{f} relu{relu}"
        out.assert_written_only(0, f, label)
        # the concat buffer: the skip half and every guard bit for bit as before, the up half written
        ph, pl = cat.bits(f, 2 * f)
        assert not (ph == SENTINEL).any() and not (pl == SENTINEL).any(), f"{label}: P not written"
        after = cat.buf.clone()
        for k in (0, 1):
            o = cat.guard + k * cat.lo_off
            after[o:o + cat.elems].view(cat.shape)[..., f:] = before[o:o + cat.elems].view(cat.shape)[..., f:]
        assert torch.equal(after, before), f"{label}: the skip half or a guard of the concat buffer changed"
        hi, lo = out.halves()
        got = M.merged(hi, lo).float()
        rge = ref.abs().max().item()
        err = (got - ref).abs().max().item()
        print(f"{label}: max err {err:.3e} = {err / (2e-5 * rge):.4f} of the bound (range {rge:.3f})")
        assert err <= 2e-5 * rge, (label, err, rge)
        lo_form = (lo.double().abs() / M.ulp_f16(hi)).max().item()
        assert lo_form <= 0.5, (label, lo_form)


def test_shapes_neither_kernel_takes_are_refused(lib):
    f = 256
    c = _case(lib, 1, 4, 14, f)
    x = torch.zeros(2, 1 * 4 * 40 * 2 * f, dtype=torch.float16, device="cuda")
    y = torch.zeros(2, 1 * 8 * 80 * 2 * f, dtype=torch.float16, device="cuda")
    args = (_h(c["wt"]), _h(c["bt"]), _h(c["w3"]), None)
    # a 40-wide map does not fit the staging
    assert lib.unet_op_updeep_window_x3_planes(0, _p(x), x[0].numel(), 1, 4, 40, f, *args, _p(y), y[0].numel(), 2 * f, f,
                                               None, None) != 0
    # cin = 2 f = 192: not a multiple of 128
    assert lib.unet_op_updeep_window_x3_planes(0, _p(x), x[0].numel(), 1, 4, 14, 96, *args, _p(y), y[0].numel(), 192, 96,
                                               None, None) != 0
    # the pair needs the 256-channel form
    assert lib.unet_op_updeep_conv3x3_x3_planes(0, _p(x), x[0].numel(), 1, 4, 14, 128, _h(c["wt"]), _h(c["bt"]), _h(c["w3"]),
                                                _h(c["scale"]), _h(c["shift"]), 1, None, None, _p(y), y[0].numel(), _p(y),
                                                y[0].numel(), None, None) != 0


@pytest.fixture(scope="module")
def modelA():
    from unet_lane_detection_amd.model import UNetHIP
    m = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    yield m
    m.release()


def _labels(m, frames):
    m.profile(True)
    out = m.run_u8(frames, precision="f16x3").clone()
    recs = m.profile_records()
    m.profile(False)
    return [r[0] for r in recs], out


def test_network_batch256_takes_the_split_step_once_per_deep_level(lib, modelA):
    frames = torch.from_numpy(S.synthetic_frames(2, seed=0)).cuda().repeat(128, 1, 1, 1).contiguous()
    prev_c, prev_d = lib.unet_set_x3_compose(-1), lib.unet_set_x3_compose_deep(1)
    try:
        names, on = _labels(modelA, frames)
        assert modelA.device_error() == 0
        lib.unet_set_x3_compose_deep(0)
        names_off, off = _labels(modelA, frames)
        assert modelA.device_error() == 0
    finally:
        lib.unet_set_x3_compose(prev_c)
        lib.unet_set_x3_compose_deep(prev_d)
    assert names.count("upconv2x2_win_f16x3") == 2, names
    assert names.count("conv3x3_t448add_f16x3_t28_c4") == 1 and names.count("conv3x3_t448add_f16x3_t28_c4_flat") == 1, names
    assert not any(n.startswith(("upconv2x2_win", "conv3x3_t448add")) for n in names_off), names_off
    assert sum(n.startswith("upconv2x2") for n in names_off) == 2, names_off
    d = (on - off).abs().max().item()
    print(f"batch 256: max |logit(split step) - logit(two-kernel path)| = {d:.3e}")
    assert d < 1e-4


def test_network_small_batch_keeps_the_two_kernel_path(lib, modelA):
    frames = torch.from_numpy(S.synthetic_frames(2, seed=0)).cuda().contiguous()
    prev_c, prev_d = lib.unet_set_x3_compose(-1), lib.unet_set_x3_compose_deep(1)
    try:
        names, auto = _labels(modelA, frames)
        lib.unet_set_x3_compose(1)                                       # mode 1 lifts the work-item rule
        names_forced, forced = _labels(modelA, frames)
        assert modelA.device_error() == 0
    finally:
        lib.unet_set_x3_compose(prev_c)
        lib.unet_set_x3_compose_deep(prev_d)
    assert not any(n.startswith(("upconv2x2_win", "conv3x3_t448add")) for n in names), names
    assert names_forced.count("upconv2x2_win_f16x3") == 2, names_forced
    assert (auto - forced).abs().max().item() < 1e-4
