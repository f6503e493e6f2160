"""The host side of the f16x3 decoder's split step on the deep levels (csrc/unet_x3.inc, pack_updeep_x3 / x3_plan_updeep):
the window weights as kernel 1 (csrc/upconv_x3_win.h) is handed them - read back out of the pack's own layout - and the
nine border-class constants, held in float64 to torch's conv_transpose2d -> cat -> conv2d; the fp16 planes of the pack
against the split of those weights; and the plan's answers for the network's shapes.  No kernels run here."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from unet_lane_detection_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _pack(lib, wt, bt, w3, f, x_act=None):
    n = (f // 64) * (2 * f // 32) * 4 * 2 * 4 * 4 * 64 * 8
    ordered = np.zeros(n, dtype=np.float64)
    packed = np.zeros(n, dtype=np.uint16)
    pre = np.zeros(f, dtype=np.float32)
    cls = np.zeros((9, f), dtype=np.float64)
    keep = [np.ascontiguousarray(a.numpy(), dtype=np.float32) for a in (wt, bt, w3)]
    act = None if x_act is None else np.ascontiguousarray(x_act.numpy(), dtype=np.float32)
    rc = lib.unet_host_pack_updeep_x3(*[C.c_void_p(k.ctypes.data) for k in keep], f,
                                      C.c_void_p(act.ctypes.data) if act is not None else None,
                                      C.c_void_p(ordered.ctypes.data), C.c_void_p(packed.ctypes.data),
                                      C.c_void_p(pre.ctypes.data), C.c_void_p(cls.ctypes.data))
    assert rc == 0
    return ordered, packed, torch.from_numpy(pre), torch.from_numpy(cls)


def _unpack(flat, f):
    """[f/64][2f/32][tap][plane][ab][cs][lane][8] -> (hi-plane positions, lo-plane positions) as [ab][co][ci][tap]:
    row j = lane & 15 of subtile cs is channel 64 ct + 16 (j >> 2) + 4 cs + (j & 3); ci = 32 kc + 8 (lane >> 4) + e"""
    t = torch.from_numpy(flat.astype(np.float64) if flat.dtype != np.float64 else flat)
    t = t.view(f // 64, 2 * f // 32, 4, 2, 4, 4, 4, 16, 8)              # ct kc tap plane ab cs lq j e
    t = t.view(f // 64, 2 * f // 32, 4, 2, 4, 4, 4, 4, 4, 8)            # ... j -> (j >> 2, j & 3)
    # co = 64 ct + 16 jh + 4 cs + jl ; ci = 32 kc + 8 lq + e
    t = t.permute(3, 4, 0, 7, 5, 8, 1, 6, 9, 2)                         # plane ab ct jh cs jl kc lq e tap
    t = t.reshape(2, 4, f, 2 * f, 4)
    return t[0], t[1]


def _params(f, seed):
    g = torch.Generator().manual_seed(seed)
    wt = (torch.randn(2 * f, f, 2, 2, generator=g) * (1.0 / (2 * f)) ** 0.5).float()
    bt = torch.randn(f, generator=g).float()                            # non-zero: all nine border classes differ
    w3 = (torch.randn(f, 2 * f, 3, 3, generator=g) * (2.0 / (18 * f)) ** 0.5).float()
    return g, wt, bt, w3


@pytest.mark.parametrize("f", [128, 256])
def test_window_weights_and_class_constants_match_torch_float64(lib, f):
    g, wt, bt, w3 = _params(f, seed=f + 1)
    ordered, packed, pre, cls = _pack(lib, wt, bt, w3, f)
    wp, lo_positions = _unpack(ordered, f)
    assert lo_positions.abs().max().item() == 0.0
    h, w = 6, 5
    x = torch.randn(2, 2 * f, h, w, generator=g, dtype=torch.float64)
    skip = torch.randn(2, f, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    up = F.conv_transpose2d(x, wt.double(), bt.double(), stride=2)
    ref = F.conv2d(torch.cat([skip, up], 1), w3.double(), padding=1)
    # P as kernel 1 forms it: per output parity (a, b) the taps (di, dj) over x rows i + a - 1 + di, columns j + b - 1 + dj
    P = torch.zeros(2, f, 2 * h, 2 * w, dtype=torch.float64)
    xp = F.pad(x, (1, 1, 1, 1))
    for a in range(2):
        for b in range(2):
            k = wp[a * 2 + b].reshape(f, 2 * f, 2, 2)
            y = F.conv2d(xp, k)                                          # (2, f, h + 1, w + 1)
            P[:, :, a::2, b::2] = y[:, :, a:a + h, b:b + w]
    rc = torch.ones(2 * h, dtype=torch.long)
    rc[0], rc[-1] = 0, 2
    cc = torch.ones(2 * w, dtype=torch.long)
    cc[0], cc[-1] = 0, 2
    klass = rc[:, None] * 3 + cc[None, :]
    out = F.conv2d(skip, w3[:, :f].double(), padding=1) + P
    out = out + cls[klass].permute(2, 0, 1)[None]
    scale = max(ref.abs().max().item(), 1.0)
    assert (out - ref).abs().max().item() <= 1e-12 * scale
    assert (cls - cls[4:5]).abs().max().item() > 1e-3                   # the classes are distinct constants


@pytest.mark.parametrize("with_act", [False, True])
def test_packed_planes_are_the_split_of_the_scaled_weights(lib, with_act):
    f = 128
    g, wt, bt, w3 = _params(f, seed=9)
    act = torch.pow(2.0, torch.randint(-3, 4, (2 * f,), generator=g).float()) if with_act else None
    ordered, packed, pre, _ = _pack(lib, wt, bt, w3, f, act)
    wp, _ = _unpack(ordered, f)
    ph, pl = _unpack(packed.view(np.float16).astype(np.float64), f)
    wx = wp.float()
    if act is not None:
        wx = wx / act[None, None, :, None]
    mx = wx.abs().amax(dim=(0, 2, 3))
    _, e = torch.frexp(mx)
    assert torch.equal(pre, torch.ldexp(torch.ones_like(mx), 10 - e))    # max |w'| into [512, 1024) per output channel
    v = wx * pre[None, :, None, None]
    hi = v.half()
    lo = (v - hi.float()).half()
    assert torch.equal(ph, hi.double()) and torch.equal(pl, lo.double())


def _plan(lib, n, h, w, f, compose=-1, deep=1, q8=0):
    q = (C.c_int * 7)(n, h, w, f, compose, deep, q8)
    out = (C.c_int * 8)()
    assert lib.unet_host_plan_updeep_x3(q, 7, out, 8) == 0
    return list(out)


def test_plan_takes_the_deep_levels_at_batch_256_and_only_them(lib):
    # model A at batch 256, 224 x 224: the 28 x 28 level (x is 14 x 14, f = 512) and the 56 x 56 level (28 x 28, f = 256)
    p28 = _plan(lib, 256, 14, 14, 512)
    p56 = _plan(lib, 256, 28, 28, 256)
    assert p28[:5] == [1, 14, 224, 8, 256] and p28[6] == 1              # 8-row tiles do not divide 28 rows: flat
    assert p56[:5] == [1, 28, 896, 4, 256] and p56[6] == 0
    assert _plan(lib, 256, 56, 56, 128) == [0] * 8                      # f % 256: the composed kernel's level
    # switches: composed paths off, the deep switch off, the f16q8 tier on
    assert _plan(lib, 256, 14, 14, 512, compose=0) == [0] * 8
    assert _plan(lib, 256, 14, 14, 512, deep=0) == [0] * 8
    assert _plan(lib, 256, 14, 14, 512, q8=1) == [0] * 8
    # the 640 x 640 configuration's deep levels are 40 and 80 wide: they keep the transposed convolution
    assert _plan(lib, 64, 40, 40, 512, compose=1) == [0] * 8
    assert _plan(lib, 64, 80, 80, 256, compose=1) == [0] * 8


def test_plan_work_item_rule(lib):
    # a small batch has no work item for half of the CUs: back to the two-kernel path, unless mode 1 lifts the rule
    assert _plan(lib, 2, 14, 14, 512) == [0] * 8
    assert _plan(lib, 2, 28, 28, 256) == [0] * 8
    assert _plan(lib, 2, 14, 14, 512, compose=1)[0] == 1
    assert _plan(lib, 1, 28, 28, 256, compose=1)[0] == 1
