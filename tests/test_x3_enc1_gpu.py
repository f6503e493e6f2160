"""The f16x3 tier's fused first encoder block (csrc/conv_x3_enc1.h) on the GPU.

The kernel stands for two launches - conv_first_x3.h, then the 64-channel form of conv_x3_t448.h with the pooled
epilogue - and promises THEIR bits: same packed weights, same operators, same order of operations.  So the operator test
is torch.equal on whole allocations (both planes of y and of the pooled tensor, sentinels around and between them
included) against unet_op_conv_first_x3_planes followed by unet_op_conv3x3_x3_planes on the same seeded inputs, and the
network test is torch.equal on the logits with the switch on and off.  Nothing is masked or skipped.

Shapes: (1, 16, 28) one tile holding all four borders; (2, 48, 84) 3 x 3 tiles, all nine border classes, two images;
(3, 40, 56) a ragged bottom tile (8 of 16 rows); (3, 224, 224) 336 items on a grid of 256, more than one item per block."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from unet_lane_detection_amd import state as S
from x3_gpu_helpers import T448, Planes, _h, _p

pytestmark = pytest.mark.gpu

MEAN = torch.tensor(O.INPUT_MEAN, dtype=torch.float32).contiguous()
STD = torch.tensor(O.INPUT_STD, dtype=torch.float32).contiguous()
SHAPES = [(1, 16, 28), (2, 48, 84), (3, 40, 56), (3, 224, 224)]
FORCED = 628            # the third structure, whatever the number of work items
LDO = 128


@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    lib = _lib.load(build_if_missing=False)
    prev_q8 = lib.unet_set_x3_cross_fp8(0)
    yield lib
    lib.unet_set_x3_cross_fp8(prev_q8)


def pow2(c, gen, lo=-6, hi=7):
    return torch.ldexp(torch.ones(c), torch.randint(lo, hi, (c,), generator=gen).to(torch.int32)).contiguous()


@functools.lru_cache(maxsize=None)
def case(n, h, w):
    """seeded frames (the last image all 0 in its top half and all 255 in its bottom half) and both layers' parameters;
    act1 / act2: non-trivial per-channel powers of two, the planes hold O(1) values"""
    gen = torch.Generator().manual_seed(1000 * n + 10 * h + w)
    frames = torch.randint(0, 256, (n, h, w, 3), generator=gen, dtype=torch.uint8)
    frames[-1, : h // 2, : w // 2] = 0
    frames[-1, h // 2:, w // 2:] = 255
    w1 = (torch.randn(64, 3, 3, 3, generator=gen) * (2.0 / 27) ** 0.5).float().contiguous()
    w2 = (torch.randn(64, 64, 3, 3, generator=gen) * (2.0 / 576) ** 0.5).float().contiguous()
    p = {}
    for k in (1, 2):
        sign = torch.where(torch.rand(64, generator=gen) < 0.25, -1.0, 1.0)
        p[f"s{k}"] = ((torch.rand(64, generator=gen) + 0.5) * sign).float().contiguous()
        p[f"b{k}"] = (torch.randn(64, generator=gen) * 0.3).float().contiguous()
        p[f"a{k}"] = pow2(64, gen)
    return dict(frames=frames.contiguous(), w1=w1, w2=w2, **p)


def run_fused(lib, c, n, h, w, *, scale1=None, scale2=None, expect_rc=0):
    y, yp = Planes(n, h, w, LDO), Planes(n, h // 2, w // 2, 64)
    path = (C.c_int * 8)()
    rng = C.c_int(-1)
    fr = c["frames"].cuda()
    s1 = c["s1"] if scale1 is None else scale1
    s2 = c["s2"] if scale2 is None else scale2
    rc = lib.unet_op_enc1_x3_planes(0, _p(fr), n, h, w, _h(c["w1"]), _h(s1), _h(c["b1"]), 1, _h(MEAN), _h(STD), _h(c["a1"]),
                                    _h(c["w2"]), _h(s2), _h(c["b2"]), 1, _h(c["a2"]), FORCED, y.ptr, y.lo_off, LDO, 0,
                                    yp.ptr, yp.lo_off, path, C.byref(rng), None)
    assert rc == expect_rc, rc
    torch.cuda.synchronize()
    return y, yp, tuple(path), rng.value


def run_two_launches(lib, c, n, h, w):
    t = Planes(n, h, w, 64)
    r1, r2 = C.c_int(-1), C.c_int(-1)
    fr = c["frames"].cuda()
    rc = lib.unet_op_conv_first_x3_planes(0, _p(fr), 1, n, h, w, _h(c["w1"]), _h(c["s1"]), _h(c["b1"]), 64, 1, _h(MEAN), _h(STD),
                                          _h(c["a1"]), t.ptr, t.lo_off, 0, C.byref(r1), None)
    assert rc == 0, rc
    y, yp = Planes(n, h, w, LDO), Planes(n, h // 2, w // 2, 64)
    path = (C.c_int * 8)()
    rc = lib.unet_op_conv3x3_x3_planes(0, t.ptr, t.lo_off, n, h, w, 64, _h(c["w2"]), _h(c["s2"]), _h(c["b2"]), 64, 1, FORCED,
                                       _h(c["a1"]), _h(c["a2"]), 0, y.ptr, y.lo_off, LDO, 0, yp.ptr, yp.lo_off, None, 0.0, 0.0,
                                       None, None, None, path, C.byref(r2), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert tuple(path)[:7] == (T448, 28, 1, 0, 1, 1, 0), tuple(path)     # the form the fused kernel stands for
    assert r1.value == 0 and r2.value == 0
    return y, yp


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_fused_block_is_the_two_launches_bit_for_bit(lib, shape):
    n, h, w = shape
    c = case(n, h, w)
    y, yp, path, rng = run_fused(lib, c, n, h, w)
    assert path == (T448, 28, 1, 0, 1, 1, 0, 1) and rng == 0, (path, rng)
    y.assert_written_only(0, 64, f"enc1 {shape}")
    yp.assert_written_only(0, 64, f"enc1 {shape} pool")
    ry, ryp = run_two_launches(lib, c, n, h, w)
    for name, got, want in (("y", y, ry), ("pool", yp, ryp)):
        for plane, (g, r) in zip(("hi", "lo"), zip(got.bits(0, 64), want.bits(0, 64))):
            diff = (g != r)
            assert torch.equal(g, r), f"{shape} {name} {plane}: {int(diff.sum())} halfs differ, first at {diff.nonzero()[:4].tolist()}"
        assert torch.equal(got.buf, want.buf), f"{shape} {name}: the allocations differ outside the planes"
    assert float(y.halves(0, 64)[0].float().abs().max()) > 0.1      # not a comparison of zeros


def test_fused_block_against_the_oracle(lib):
    """oracle.conv3x3 twice, in real units: the tier's single-layer bound, 2e-5 of the output's range"""
    n, h, w = 2, 48, 84
    c = case(n, h, w)
    y, yp, _, rng = run_fused(lib, c, n, h, w)
    assert rng == 0
    x = O.normalize_u8_nhwc(c["frames"].numpy())

    def bc(v):
        return v[None, :, None, None]
    t = torch.relu(O.conv3x3(x, c["w1"]) * bc(c["s1"]) + bc(c["b1"]))
    want = torch.relu(O.conv3x3(t, c["w2"]) * bc(c["s2"]) + bc(c["b2"]))
    hi, lo = y.halves(0, 64)
    got = ((hi.double() + lo.double()) / c["a2"].double()).permute(0, 3, 1, 2)
    err = float((got - want.double()).abs().max())
    bound = 2e-5 * float(want.abs().max())
    print(f"enc1 fused vs oracle: max |dy| {err:.3e}, bound {bound:.3e}")
    assert err < bound
    ph, pl = yp.halves(0, 64)
    gotp = ((ph.double() + pl.double()) / c["a2"].double()).permute(0, 3, 1, 2)
    # the pooled planes are the max of positive multiples of the activation: pooling commutes with the scale only for
    # act2 > 0, which powers of two are
    assert float((gotp - O.maxpool2x2(want).double()).abs().max()) < bound


def test_first_layer_leaving_the_range_is_reported(lib):
    """a scale that drives enc1.conv1's output past 65504: the fused kernel's own range watch (phase A) reports it"""
    n, h, w = 1, 16, 28
    c = case(n, h, w)
    _, _, _, rng = run_fused(lib, c, n, h, w)
    assert rng == 0
    big = (c["s1"] / c["a1"] * 1e7).contiguous()        # |planes| ~ 1e7 whatever the channel's activation scale
    tiny = (c["s2"] * 1e-9).contiguous()                # ... while the second layer's own output stays far inside it
    _, _, path, rng = run_fused(lib, c, n, h, w, scale2=tiny)
    assert rng == 0
    _, _, path, rng = run_fused(lib, c, n, h, w, scale1=big, scale2=tiny)
    assert path[7] == 1 and rng == 1


def test_entry_point_refuses_what_the_plan_declines(lib):
    c = case(1, 16, 28)
    y, yp = Planes(1, 16, 30, LDO), Planes(1, 8, 15, 64)
    fr = torch.zeros(1, 16, 30, 3, dtype=torch.uint8, device="cuda")
    rc = lib.unet_op_enc1_x3_planes(0, _p(fr), 1, 16, 30, _h(c["w1"]), _h(c["s1"]), _h(c["b1"]), 1, _h(MEAN), _h(STD), None,
                                    _h(c["w2"]), _h(c["s2"]), _h(c["b2"]), 1, None, FORCED, y.ptr, y.lo_off, LDO, 0, yp.ptr,
                                    yp.lo_off, None, None, None)
    assert rc == 1                                      # UNET_ERR_INVALID_ARG: no whole 28-wide tiles


# ---- the network ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def modelA():
    from unet_lane_detection_amd.model import UNetHIP
    m = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    yield m
    m.release()


def enc1_takes(lib, n, h, w, on):
    q = (C.c_int * 13)(1, n, h, w, 64, 0, 0, 1 if on else 0, 1, 1, 1, 1, 0)
    plan = (C.c_int * 8)()
    assert lib.unet_host_plan_enc1_x3(q, 13, plan, 8) == 0
    return plan[0] == 1


@pytest.mark.parametrize("batch", [2, 1], ids=["batch2-taken", "batch1-declined"])
def test_network_logits_do_not_depend_on_the_switch(lib, modelA, batch):
    frames = torch.from_numpy(S.synthetic_frames(batch, seed=7)).cuda().contiguous()
    out, names = {}, {}
    prev = lib.unet_set_x3_fuse_first(1)
    try:
        for on in (1, 0):
            lib.unet_set_x3_fuse_first(on)
            modelA.profile(True)
            out[on] = modelA.run_u8(frames, precision="f16x3").clone()
            assert modelA.device_error() == 0
            names[on] = [r[0] for r in modelA.profile_records()]
            modelA.profile(False)
    finally:
        lib.unet_set_x3_fuse_first(prev)
    assert torch.equal(out[1], out[0])
    assert bool(np.isfinite(out[1].cpu().numpy()).all())
    for on in (1, 0):
        taken = enc1_takes(lib, batch, 224, 224, on)
        assert taken == (on == 1 and batch == 2)
        assert names[on][0] == ("conv3x3_enc1_f16x3" if taken else "conv3x3_first_f16x3"), names[on][:3]
        assert ("conv3x3_enc1_f16x3" in names[on]) == taken
    # one launch fewer where the block is fused
    assert len(names[0]) - len(names[1]) == (1 if batch == 2 else 0)
