"""CPU-side checks of the C ABI: the library loads, exports every symbol the header declares,
and its host logic (spec enumeration, shape checks) behaves.  No kernels run here."""
import ctypes as C
import os
import re

import pytest

from unet_lane_detection_amd import _lib, state as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_symbols_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/unet_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)


def test_version_string(lib):
    assert b"gfx950" in lib.unet_version()


def test_invalid_create_arguments(lib):
    h = C.c_void_p()
    assert lib.unet_create(None, C.byref(h)) == 1
    cfg = _lib.UnetConfig()
    cfg.in_channels, cfg.out_channels, cfg.depth = 3, 1, 0
    assert lib.unet_create(C.byref(cfg), C.byref(h)) == 1
    cfg.depth = 2
    cfg.features[0], cfg.features[1] = 6, 8          # channels must be multiples of 4
    assert lib.unet_create(C.byref(cfg), C.byref(h)) == 1


def test_param_spec_matches_reference_state_dict(lib):
    """The library expects exactly the reference module's float state_dict keys and sizes."""
    import numpy as np
    cfg = _lib.UnetConfig()
    cfg.in_channels, cfg.out_channels, cfg.depth = 3, 1, 4
    for i, f in enumerate(S.DEFAULT_FEATURES):
        cfg.features[i] = f
    h = C.c_void_p()
    assert lib.unet_create(C.byref(cfg), C.byref(h)) == 0
    n = lib.unet_num_params(h)
    got = {lib.unet_param_name(h, i).decode(): lib.unet_param_numel(h, i) for i in range(n)}
    want = {k: int(np.prod(shape)) if shape else 1 for k, shape, kind in S.state_dict_spec() if kind != "bn_count"}
    assert got == want
    assert sum(v for k, v in got.items() if "running_" not in k) == 31_037_633   # reference README.md:2288
    # wrong size and unknown name are rejected with the documented codes
    buf = (C.c_float * 4)()
    assert lib.unet_load_param(h, b"output.bias", buf, 4) == 2
    assert lib.unet_load_param(h, b"nope.weight", buf, 4) == 6
    assert lib.unet_finalize(h) == 3                   # parameters missing
    assert lib.unet_workspace_bytes(h, 1, 225, 224) == 0   # 225 is not a multiple of 16
    assert lib.unet_workspace_bytes(h, 256, 224, 224) > 10 * 2**30
    assert lib.unet_destroy(h) == 0


def test_act_scale_of_nearly_dead_bn_channel(lib):
    """f16x3 tier, host logic (csrc/unet_x3.inc, act_from_bn): the per-channel power-of-two activation scale puts
    4 |gamma| + |beta| into [512, 1024) - and must stay finite for a channel that is almost, but not exactly, dead
    (the unclamped 2^(10 - e) was +inf below 2^-118: inf / NaN scale and shift, a range report on every frame)."""
    import math
    for gamma, beta in ((1.0, 0.0), (0.02, -0.3), (3e-5, 0.0), (250.0, 10.0)):
        s = lib.unet_debug_act_scale(gamma, beta)
        m = (4 * abs(gamma) + abs(beta)) * s
        assert 512.0 <= m < 1024.0 and math.log2(s) == int(math.log2(s)), (gamma, beta, s)
    assert lib.unet_debug_act_scale(0.0, 0.0) == 1.0                    # a dead channel is stored as it is
    for gamma, beta in ((1e-38, 0.0), (0.0, 1e-40), (3e-36, 1e-37)):    # nearly dead: finite, no scaling
        s = lib.unet_debug_act_scale(gamma, beta)
        assert math.isfinite(s) and s == 1.0, (gamma, beta, s)
    s = lib.unet_debug_act_scale(1e-20, 0.0)                            # tiny but alive: clamped to 2^40
    assert s == 2.0 ** 40
    assert lib.unet_debug_act_scale(1e30, 0.0) == 2.0 ** -40


def test_x3_plane_entry_points_check_arguments_first(lib):
    """the plane-level f16x3 entry points (tests/test_x3_ops_gpu.py) reject what they cannot run before touching a device"""
    buf = (C.c_uint16 * 64)()
    f = (C.c_float * 64)()
    p, q = C.cast(buf, C.c_void_p), C.cast(f, C.c_void_p)

    def conv(cin=64, cout=64, tw=0, ldo=0, co_off=0, x_lo=64, pool=None, head=None, y=p, h=8, w=8):
        return lib.unet_op_conv3x3_x3_planes(0, p, x_lo, 1, h, w, cin, q, q, q, cout, 1, tw, None, None, 0, y, 64, ldo, co_off,
                                             pool, 0, head, 0.0, 0.0, q if head else None, None, None, None, None, None)
    assert conv(cin=32) == 1 and conv(cout=96) == 1 and conv(cout=2048) == 1
    assert conv(tw=428) == 1 and conv(tw=414) == 1 and conv(tw=24) == 1          # the f16q8 widths are not this entry's
    assert conv(ldo=64, co_off=64) == 1 and conv(ldo=96) == 1 and conv(ldo=128, co_off=32) == 1
    assert conv(x_lo=63) == 1 and conv(y=None) == 1
    assert conv(pool=p, h=7) == 1 and conv(pool=p, head=q) == 1 and conv(cout=128, head=q, y=None) == 1
    assert lib.unet_op_upconv2x2_x3_planes(0, p, 64, 1, 4, 4, 64, q, q, 64, None, p, 64, 128, 128, None, None, None) == 1
    assert lib.unet_op_conv_first_x3_planes(0, p, 1, 1, 8, 8, q, q, q, 64, 1, None, None, None, p, 64, 0, None, None) == 1
    assert lib.unet_op_maxpool2x2_x3_planes(0, p, 64, 1, 3, 4, 8, 0, p, 64, None) == 1
    assert lib.unet_op_head1x1_x3_planes(0, p, 64, 1, 2, 2, 8, q, 0.0, 0.0, None, None, None, None) == 1
    assert lib.unet_op_split_planes_x3(0, q, 3, p, 64, None, None) == 1


def test_train_x3_entry_points_check_arguments_first(lib):
    """the training step's operator entry points (tests/test_train_x3_ops_gpu.py) reject what they cannot run before
    touching a device"""
    buf = (C.c_uint16 * 64)()
    f = (C.c_float * 64)()
    p, q = C.cast(buf, C.c_void_p), C.cast(f, C.c_void_p)

    def conv(planes=p, x32=None, scaled=0, cin=64, cout=64, mode=0, packer=0, tw=0, ldo=0, off=0, y=q, stat=None, cap=0,
             rows=None, w=q):
        return lib.unet_op_train_conv3x3_x3(0, planes, x32, scaled, 1, 8, 8, cin, cout, w, mode, packer, tw, y, ldo, off, stat,
                                            cap, rows, None, None, None, None)
    assert conv(cin=32) == 1 and conv(cout=96) == 1 and conv(cout=2048) == 1 and conv(cin=2048) == 1
    assert conv(planes=None) == 1 and conv(x32=q) == 1 and conv(scaled=1) == 1          # exactly one input; scaled needs fp32
    assert conv(mode=2) == 1 and conv(packer=2) == 1 and conv(w=None) == 1 and conv(y=None) == 1
    assert conv(packer=1, w=C.c_void_p(C.addressof(f) + 4)) == 1                        # the LDS packer's float4 loads
    assert conv(tw=428) == 1 and conv(tw=414) == 1 and conv(tw=24) == 1
    assert conv(ldo=64, off=64) == 1 and conv(ldo=96) == 1 and conv(ldo=128, off=32) == 1
    assert conv(stat=q) == 1 and conv(stat=q, cap=4) == 1                               # rows requested without a count word

    def bwd(f_=64, ldd=128, offd=64, dy=q, planes=p):
        return lib.unet_op_upconv_bwd_x3(0, dy, ldd, offd, planes, q, 1, 4, 4, f_, q, q, q, None, None, None)
    assert bwd(f_=32) == 1 and bwd(f_=96) == 1 and bwd(f_=1024) == 1      # 4 f and 2 f must be multiples of 128
    assert bwd(ldd=64) == 1 and bwd(offd=2) == 1 and bwd(ldd=130) == 1 and bwd(dy=None) == 1 and bwd(planes=None) == 1
    assert lib.unet_op_upconv_fwd_train_x3(0, p, 64, 1, 4, 4, 64, q, q, 64, p, 64, 128, 128, None, None, None) == 1
    assert lib.unet_op_upconv_fwd_train_x3(0, p, 64, 1, 4, 4, 96, q, q, 64, p, 64, 0, 0, None, None, None) == 1
    assert lib.unet_op_upconv_fwd_train_x3(0, p, 64, 1, 4, 4, 64, q, None, 64, p, 64, 0, 0, None, None, None) == 1
    # the 3x3 weight gradient: channel counts multiples of 64, even heights
    assert lib.unet_op_wgrad3x3_x3(0, q, q, 1, 7, 8, 64, 64, q, 0, None) == 1
    assert lib.unet_op_wgrad3x3_x3(0, q, q, 1, 8, 8, 96, 64, q, 0, None) == 1


def test_f32_entry_points_check_arguments_first(lib):
    """the fp32 tier's entry points (tests/test_f32_ops_gpu.py) reject what they cannot run before touching a device, and
    then fail at the device selection (an ordinal the runtime refuses: no device is touched)"""
    f = (C.c_float * 64)()
    q = C.cast(f, C.c_void_p)
    bad = 1 << 20

    def conv(dev=0, x=q, cin=16, cout=8, h=4, w=4, algo=0, ldo=0, off=0, y=q, pool=None, n=1):
        return lib.unet_op_conv3x3_f32(dev, x, n, h, w, cin, q, q, q, cout, 1, algo, ldo, off, y, pool, None, None)
    assert conv(x=None) == 1 and conv(y=None) == 1 and conv(cin=6) == 1 and conv(cout=6) == 1 and conv(n=0) == 1
    assert conv(algo=3) == 1 and conv(algo=-1) == 1
    assert conv(algo=2, cin=4) == 1 and conv(algo=2, h=3) == 1 and conv(algo=2, w=5) == 1     # Winograd cannot take these
    assert conv(ldo=8, off=4) == 1 and conv(ldo=18, off=0) == 1 and conv(ldo=16, off=2) == 1 and conv(off=8) == 1
    assert conv(ldo=16, off=-4) == 1 and conv(pool=q, h=3) == 1 and conv(pool=q, w=5) == 1
    assert lib.unet_op_last_error().startswith(b"invalid argument")
    assert conv(dev=bad) == 4 and conv(dev=bad, algo=2, ldo=16, off=8, pool=q) == 4 and conv(dev=bad, algo=1, cin=4) == 4
    assert b"hipSetDevice" in lib.unet_op_last_error()

    def up(dev=0, x=q, cin=16, cout=8, ldo=0, off=0, y=q):
        return lib.unet_op_upconv2x2_f32(dev, x, 1, 4, 4, cin, q, q, cout, ldo, off, y, None, None)
    assert up(x=None) == 1 and up(y=None) == 1 and up(cin=2) == 1 and up(cout=10) == 1
    assert up(ldo=8, off=4) == 1 and up(ldo=12, off=2) == 1 and up(off=4) == 1
    assert up(dev=bad) == 4 and up(dev=bad, ldo=16, off=8) == 4

    def c1(dev=0, x=q, cin=16, cout=8, ldo=0, off=0, y=q):
        return lib.unet_op_conv1x1_f32(dev, x, 1, 4, 4, cin, q, cout, ldo, off, y, None, None)
    assert c1(x=None) == 1 and c1(y=None) == 1 and c1(cin=2) == 1 and c1(cout=10) == 1 and c1(ldo=8, off=4) == 1
    assert c1(dev=bad) == 4

    def pool(dev=0, x=q, h=4, w=4, c=8, ldi=0, y=q):
        return lib.unet_op_maxpool2x2_f32(dev, x, 1, h, w, c, ldi, y, None)
    assert pool(x=None) == 1 and pool(y=None) == 1 and pool(h=3) == 1 and pool(w=5) == 1 and pool(c=6) == 1
    assert pool(ldi=4) == 1 and pool(ldi=10) == 1
    assert pool(dev=bad) == 4 and pool(dev=bad, ldi=16) == 4

    def head(dev=0, x=q, c=8, w=q, logits=q, probs=None, mask=None):
        return lib.unet_op_head1x1_f32(dev, x, 1, 2, 2, c, w, 0.0, 0.0, logits, probs, mask, None)
    assert head(x=None) == 1 and head(w=None) == 1 and head(c=6) == 1 and head(logits=None) == 1     # no output at all
    assert head(dev=bad) == 4 and head(dev=bad, logits=None, mask=q) == 4

    def pack(dev=0, src=q, is_u8=1, mean=q, std=q, y=q, h=2):
        return lib.unet_op_pack_input_f32(dev, src, is_u8, 1, h, 2, mean, std, y, None)
    assert pack(src=None) == 1 and pack(y=None) == 1 and pack(mean=None) == 1 and pack(std=None) == 1 and pack(h=0) == 1
    assert pack(dev=bad) == 4 and pack(dev=bad, is_u8=0, mean=None, std=None) == 4


def test_op_last_error_names_the_failing_call(lib):
    """a handle-less entry point that fails leaves its text for unet_op_last_error, per thread: a device ordinal the
    runtime refuses (no device is touched, with or without GPUs) in one entry point of each of three files"""
    import threading
    buf = (C.c_uint16 * 64)()
    f = (C.c_float * 64)()
    p, q = C.cast(buf, C.c_void_p), C.cast(f, C.c_void_p)
    seen = {}

    def other():   # a thread that has made no failing call
        seen["other"] = lib.unet_op_last_error()
    t = threading.Thread(target=other)
    bad = 1 << 20
    calls = {
        "unet_op_maxpool2x2": lambda: lib.unet_op_maxpool2x2(bad, q, 1, 2, 2, 4, q, None),
        "unet_op_maxpool2x2_bf16": lambda: lib.unet_op_maxpool2x2_bf16(bad, p, 1, 2, 2, 8, 0, p, None),
        "unet_op_split_planes_x3": lambda: lib.unet_op_split_planes_x3(bad, q, 4, p, 4, None, None),
    }
    for name, call in calls.items():
        assert call() == 4, name                       # UNET_ERR_HIP
        msg = lib.unet_op_last_error()
        assert msg and b"hipSetDevice" in msg, (name, msg)
    assert lib.unet_op_maxpool2x2(0, q, 1, 3, 2, 4, q, None) == 1      # a refusal by the argument checks replaces the text
    assert lib.unet_op_last_error().startswith(b"invalid argument")
    t.start()
    t.join()
    assert seen["other"] == b""
    with pytest.raises(_lib.UnetError, match="hipSetDevice"):   # _lib.check appends the text when there is no handle
        _lib.check(calls["unet_op_maxpool2x2"](), "unet_op_maxpool2x2")


# ---- the frame of the handle-less entry points that live in translation units of their own (csrc/op_entry.h) ---------
FRAMED_ENTRY_POINTS = {
    "unet_fill_polygons_u8_batch", "unet_augment_u8", "unet_correct_u8_batch", "unet_frame_stats_u8_batch",
    "unet_prob_stats_f32_batch", "unet_ensemble_combine", "unet_score_sweep_accumulate", "unet_hsv_lanes_u8_batch",
    "unet_lane_center_u8_batch", "unet_grad_accumulate_f32", "unet_label_u8_batch", "unet_keep_components_u8_batch",
    "unet_lane_fit_u8_batch", "unet_lane_view_u8_batch", "unet_resize_u8_batch", "unet_overlay_u8_batch"}


def _framed_calls(lib):
    """name -> the arguments between `device` and `stream` of a call that passes every argument check: 8 x 8 images in
    host memory, every buffer a 4 KB slot of its own on a 64-byte boundary (the checks look at addresses only)"""
    work = max(int(lib.unet_correct_work_bytes(1, 1, 1)), int(lib.unet_label_work_bytes(1, 8, 8)), 4096)
    arena = (C.c_uint8 * (8 * 4096 + work + 64))()
    base = (C.addressof(arena) + 63) & ~63
    a, b, c, d, e, f, g, big = (C.c_void_p(base + 4096 * i) for i in range(8))
    cfg = _lib.CorrectConfigStruct()
    cfg.max_gain, cfg.grid_x, cfg.grid_y, cfg.clip_q8, cfg.bright_limit = 1, 1, 1, 256, 255
    members = (C.c_void_p * 1)(a.value)
    thresholds = (C.c_float * 2)(0.25, 0.75)
    rows = (C.c_int * 1)(5)
    m = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    calls = {
        "unet_fill_polygons_u8_batch": (a, b, c, d, 1, 8, 8, 8, 8, e),
        "unet_augment_u8": (a, None, 1, 8, 8, b, 1, 127, c, None),
        "unet_correct_u8_batch": (a, 1, 8, 8, 0, 0, C.byref(cfg), b, 0, big, work),
        "unet_frame_stats_u8_batch": (a, 1, 8, 8, 0, 0, b),
        "unet_prob_stats_f32_batch": (a, 1, 64, 0.5, b),
        "unet_ensemble_combine": (members, 1, None, 64, 0.5, b, None),
        "unet_score_sweep_accumulate": (a, b, 0, 64, thresholds, 2, c),
        "unet_hsv_lanes_u8_batch": (a, 1, 8, 8, 1, b, c, 5, 5, d),
        "unet_lane_center_u8_batch": (a, 1, 8, 8, rows, 1, 127, b),
        "unet_grad_accumulate_f32": (a, b, None, 64, None, None),
        "unet_label_u8_batch": (a, 1, 8, 8, 127, 8, b, 4, c, d, big, work),
        "unet_keep_components_u8_batch": (a, 1, 8, 8, b, c, 4, 0, 0, 0, 0, d, e),
        "unet_lane_fit_u8_batch": (a, 1, 8, 8, 127, 4, 2, 1, None, b),
        "unet_lane_view_u8_batch": (a, 1, 8, 8, 24, m, 8, 8, b, 127, None, 0, None, c, None),
        "unet_resize_u8_batch": (a, 1, 8, 8, 3, 0, 4, 4, b),
        "unet_overlay_u8_batch": (a, 1, 8, 8, b, 8, 8, c, 0.5, 0.5, 0.0, d, None),
    }
    return calls, (arena, cfg, members, thresholds, rows, m)


def test_framed_entry_points_refuse_and_fail_alike(lib):
    """every entry point built on csrc/op_entry.h, from one table: a null first pointer is refused as an invalid
    argument with the entry point's name in the text, and a call that passes every check fails at the device
    selection with the HIP error in the text (an ordinal the runtime refuses: no device is touched)"""
    calls, keep = _framed_calls(lib)
    assert set(calls) == FRAMED_ENTRY_POINTS and len(calls) == 16
    for name, args in calls.items():
        assert name in _lib.SIGNATURES, name
        argtypes = _lib.SIGNATURES[name][1]
        assert len(argtypes) == len(args) + 2 and argtypes[0] is C.c_int and argtypes[-1] is C.c_void_p, name
        assert argtypes[1] is C.c_void_p or issubclass(argtypes[1], C._Pointer), name   # args[0]: the first pointer
        fn = getattr(lib, name)
        assert fn(0, None, *args[1:], None) == 1, name                       # UNET_ERR_INVALID_ARG
        msg = lib.unet_op_last_error()
        assert msg.startswith(b"invalid argument: ") and name.encode() in msg, (name, msg)
        assert fn(1 << 20, *args, None) == _lib.UNET_ERR_HIP, (name, lib.unet_op_last_error())
        msg = lib.unet_op_last_error()
        assert b"hipSetDevice" in msg, (name, msg)
    del keep
