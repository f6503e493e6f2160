"""The handle-less test entry points own their device scratch per call (csrc/unet_hip.cpp, OpScratch / OpGuard): whatever
a call allocates is back when it returns, on the success path and on a refusal after the allocations.

One entry point per tier at the smallest shape of its test table: 3 warm-up calls, torch.cuda.mem_get_info(), 20 more calls,
mem_get_info() again - free device memory must not have dropped.  Measured drop over the 20 calls on an MI355X, bytes, the
library before the shared scratch owner / with it: fp32 0 / 0, bf16 0 / 0, f16x3 0 / 0, training 0 / 0, bf16 refusal 0 / 0
(the runtime hands a freed block straight back to the device, so there is no allowance to make)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG = 1


@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    return _lib.load(build_if_missing=False)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _h(t):
    return C.c_void_p(t.numpy().ctypes.data)


def fp32_conv(lib):
    x, y = torch.zeros(1, 8, 8, 4, device="cuda"), torch.zeros(1, 8, 8, 4, device="cuda")
    w, sc, sh = torch.zeros(4, 4, 3, 3), torch.ones(4), torch.zeros(4)
    return lambda: lib.unet_op_conv3x3(0, _p(x), 1, 8, 8, 4, _h(w), _h(sc), _h(sh), 4, 1, _p(y), None), 0


def bf16_conv(lib, width=32, kernel=0, want=0):
    x = torch.zeros(1, 16, width, 32, dtype=torch.int16, device="cuda")
    y = torch.zeros(1, 16, width, 64, dtype=torch.int16, device="cuda")
    w, sc, sh = torch.zeros(64, 32, 3, 3), torch.ones(64), torch.zeros(64)
    return lambda: lib.unet_op_conv3x3_bf16(0, _p(x), 1, 16, width, 32, _h(w), _h(sc), _h(sh), 64, 1, kernel, 0, 0, _p(y), None,
                                            None, None), want


def bf16_refusal(lib):   # the one-wave-per-SIMD kernel forced on a width it does not take: refused after the allocations
    return bf16_conv(lib, width=8, kernel=3, want=ERR_INVALID_ARG)


def x3_conv(lib):
    x, y = torch.zeros(1, 16, 32, 64, device="cuda"), torch.zeros(1, 16, 32, 64, device="cuda")
    w, sc, sh = torch.zeros(64, 64, 3, 3), torch.ones(64), torch.zeros(64)
    return lambda: lib.unet_op_conv3x3_x3(0, _p(x), 1, 16, 32, 64, _h(w), _h(sc), _h(sh), 64, 1, 0, _p(y), None, None), 0


def train_upconv(lib):
    n, h, w, cin, cout = 1, 4, 4, 128, 64
    ex, ey = n * h * w * cin, n * 2 * h * 2 * w * cout
    x = torch.zeros(2 * ex, dtype=torch.int16, device="cuda")      # [hi | lo]
    y = torch.zeros(2 * ey, dtype=torch.int16, device="cuda")
    wt, b = torch.zeros(cin, cout, 2, 2, device="cuda"), torch.zeros(cout, device="cuda")
    return lambda: lib.unet_op_upconv_fwd_train_x3(0, _p(x), ex, n, h, w, cin, _p(wt), _p(b), cout, _p(y), ey, 0, 0, None, None,
                                                   None), 0


@pytest.mark.parametrize("case", [fp32_conv, bf16_conv, x3_conv, train_upconv, bf16_refusal], ids=lambda f: f.__name__)
def test_entry_point_returns_its_scratch(lib, case):
    call, want = case(lib)
    for _ in range(3):
        assert call() == want
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        assert call() == want
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    print(f"{case.__name__}: free memory dropped by {before - after} bytes over 20 calls")
    assert after >= before, (case.__name__, before - after)
