"""The host composition behind the f16x3 tier's composed decoder step (csrc/unet_x3.inc, compose_upcat): the transposed
convolution folded into the up half of the 3x3 convolution behind it, checked in float64 against torch's own
ConvTranspose2d -> Conv3x3 at all four decoder level widths.  No kernels run here."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from unet_lane_detection_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _compose(lib, wt, bt, w3, f):
    wp = np.zeros((4, f, 2 * f, 2, 2), dtype=np.float64)
    bias = np.zeros((9, f), dtype=np.float64)
    wt32, bt32, w332 = (np.ascontiguousarray(a.numpy(), dtype=np.float32) for a in (wt, bt, w3))
    rc = lib.unet_host_compose_upcat(C.c_void_p(wt32.ctypes.data), C.c_void_p(bt32.ctypes.data),
                                     C.c_void_p(w332.ctypes.data), f, C.c_void_p(wp.ctypes.data),
                                     C.c_void_p(bias.ctypes.data))
    assert rc == 0
    return torch.from_numpy(wp), torch.from_numpy(bias)


@pytest.mark.parametrize("f", [64, 128, 256, 512])
def test_composition_matches_torch_float64(lib, f):
    g = torch.Generator().manual_seed(f)
    wt = (torch.randn(2 * f, f, 2, 2, generator=g) * (1.0 / (2 * f)) ** 0.5).float()
    bt = torch.randn(f, generator=g).float()                         # large enough that every border class differs
    w3 = (torch.randn(f, 2 * f, 3, 3, generator=g) * (2.0 / (18 * f)) ** 0.5).float()
    wp, bias = _compose(lib, wt, bt, w3, f)
    # the float32 parameters as float64: the composition itself is what is checked
    wt64, bt64, w3up = wt.double(), bt.double(), w3[:, f:].double()
    h, w = 3, 4                                                      # low resolution: all nine border classes occur
    x = torch.randn(2, 2 * f, h, w, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.conv_transpose2d(x, wt64, bt64, stride=2), w3up, padding=1)
    out = torch.zeros_like(ref)
    xp = F.pad(x, (1, 1, 1, 1))
    for a in range(2):
        for b in range(2):
            y = F.conv2d(xp, wp[a * 2 + b])                          # (2, f, h + 1, w + 1)
            out[:, :, a::2, b::2] = y[:, :, a:a + h, b:b + w]
    rc = torch.ones(2 * h, dtype=torch.long)
    rc[0], rc[-1] = 0, 2
    cc = torch.ones(2 * w, dtype=torch.long)
    cc[0], cc[-1] = 0, 2
    cls = rc[:, None] * 3 + cc[None, :]                              # (2h, 2w)
    out += bias[cls].permute(2, 0, 1)[None]
    scale = ref.abs().max().item()
    assert (out - ref).abs().max().item() <= 1e-12 * max(scale, 1.0)
    # the nine classes are distinct constants: the bias is not simply the interior one everywhere
    assert (bias - bias[4:5]).abs().max().item() > 1e-3
