"""The f16x3 tier's weight packs on the CPU (csrc/unet_x3.inc: pack_conv_x3, pack_upconv_x3, pack_first_x3, pack_upcat_x3,
all written through x3_put_frag) through the host hook unet_host_pack_x3: every layout is read back with a view and a
permute and must hold exactly half(w * pre) and half(w * pre - hi).  No kernels run here.

In every layout lane = 16 lq + j, row j = 4 jh + jl of subtile cs of tile ct is channel 64 ct + 16 jh + 4 cs + jl, and the
lane's eight halfs e are k = 32 chunk + 8 lq + e."""
import ctypes as C

import numpy as np
import pytest
import torch

from unet_lane_detection_amd import _lib

CONV, UPCONV, FIRST, COMPOSED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _pack(lib, kind, w, wx, cout, cin, pre, n_packed):
    packed = np.zeros(n_packed, dtype=np.uint16)
    keep = [None if a is None else np.ascontiguousarray(a.numpy(), dtype=np.float32) for a in (w, wx, pre)]
    ptr = [None if k is None else C.c_void_p(k.ctypes.data) for k in keep]
    rc = lib.unet_host_pack_x3(kind, ptr[0], ptr[1], cout, cin, ptr[2], C.c_void_p(packed.ctypes.data), n_packed)
    assert rc == 0
    assert lib.unet_host_pack_x3(kind, ptr[0], ptr[1], cout, cin, ptr[2], C.c_void_p(packed.ctypes.data), n_packed + 8) == 1
    return torch.from_numpy(packed.view(np.float16).astype(np.float32))


def _weights(shape, cout, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(*shape, generator=g) * 0.05).float()
    pre = torch.pow(2.0, torch.randint(6, 11, (cout,), generator=g).float())
    return w, pre


def _split(v):
    hi = v.half()
    return hi.float(), (v - hi.float()).half().float()


@pytest.mark.parametrize("f", [64, 128])
def test_conv3x3_pack(lib, f):
    cout, cin = f, f // 2
    w, pre = _weights((cout, cin, 3, 3), cout, seed=f)
    t = _pack(lib, CONV, w, None, cout, cin, pre, (cout // 64) * (cin // 32) * 3 * 2 * 3 * 4 * 64 * 8)
    t = t.view(cout // 64, cin // 32, 3, 2, 3, 4, 4, 4, 4, 8)           # ct kc r plane kx cs lq jh jl e
    t = t.permute(3, 0, 7, 5, 8, 1, 6, 9, 2, 4).reshape(2, cout, cin, 3, 3)
    hi, lo = _split(w * pre[:, None, None, None])
    assert torch.equal(t[0], hi) and torch.equal(t[1], lo)
    assert lo.abs().max().item() > 0


@pytest.mark.parametrize("f", [64, 128])
def test_upconv2x2_pack(lib, f):
    cout, cin = f, f // 2
    w, pre = _weights((cin, cout, 2, 2), cout, seed=f + 1)
    t = _pack(lib, UPCONV, w, None, cout, cin, pre, (cout // 64) * (cin // 32) * 2 * 16 * 64 * 8)
    t = t.view(cout // 64, cin // 32, 2, 4, 4, 4, 4, 4, 8)              # ct kc plane ab cs lq jh jl e
    t = t.permute(2, 1, 5, 8, 0, 6, 4, 7, 3).reshape(2, cin, cout, 2, 2)
    hi, lo = _split(w * pre[None, :, None, None])
    assert torch.equal(t[0], hi) and torch.equal(t[1], lo)


@pytest.mark.parametrize("f", [64, 128])
def test_first_conv_pack(lib, f):
    w, pre = _weights((f, 3, 3, 3), f, seed=f + 2)
    t = _pack(lib, FIRST, w, None, f, 3, pre, (f // 64) * 4 * 2 * 64 * 8)
    t = t.view(f // 64, 4, 2, 4, 4, 4, 8)                               # ct cs plane lq jh jl e
    t = t.permute(2, 0, 4, 1, 5, 3, 6).reshape(2, f, 32)                # k = tap * 3 + ci
    hi, lo = _split((w * pre[:, None, None, None]).reshape(f, 3, 9).permute(0, 2, 1).reshape(f, 27))
    assert torch.equal(t[0, :, :27], hi) and torch.equal(t[1, :, :27], lo)
    assert t[:, :, 27:].abs().max().item() == 0.0


@pytest.mark.parametrize("f", [64, 128])
def test_composed_pack(lib, f):
    ws, pre = _weights((f, f, 3, 3), f, seed=f + 3)
    wx, _ = _weights((4, f, 2 * f, 4), f, seed=f + 4)
    n_ct, n_s, n_x, tap = f // 64, f // 32, 2 * f // 32, 2 * 4 * 64 * 8
    t = _pack(lib, COMPOSED, ws, wx, f, 2 * f, pre, n_ct * (n_s * 9 + n_x * 16) * tap).view(n_ct, -1)
    s = t[:, :n_s * 9 * tap].reshape(n_ct, n_s, 9, 2, 4, 4, 4, 4, 8)     # ct kc tap plane cs lq jh jl e
    s = s.permute(3, 0, 6, 4, 7, 1, 5, 8, 2).reshape(2, f, f, 3, 3)
    hi, lo = _split(ws * pre[:, None, None, None])
    assert torch.equal(s[0], hi) and torch.equal(s[1], lo)
    x = t[:, n_s * 9 * tap:].reshape(n_ct, n_x, 4, 4, 2, 4, 4, 4, 4, 8)  # ct kc parity tap plane cs lq jh jl e
    x = x.permute(4, 2, 0, 7, 5, 8, 1, 6, 9, 3).reshape(2, 4, f, 2 * f, 4)
    hi, lo = _split(wx * pre[None, :, None, None])
    assert torch.equal(x[0], hi) and torch.equal(x[1], lo)
