"""fp32 tier, per kernel, on the paths the network runs: csrc/igemm_f32.h (3x3, transposed 2x2 and plain 1x1 convolution,
every template instance the host code can select), csrc/wino_f32.h (with its fused pool) and the kernels of
csrc/elementwise.h, through the unet_op_*_f32 entry points, against the float64 model of tests/f32_model.py.

Per output element, with r the float64 result of the fp32 inputs held exactly:

    |got - r| <= C_ULP * ulp32(|r|) + C_ACC * 2^-24 * sqrt(K) * |scale| * B,     C_ACC = 10.5, C_ULP = 7.5

B = sqrt(conv(x^2, w^2)), K the number of terms.  The constants are 4 x what two fp32 emulations of the kernels' own
summation order reach on the CPU over this file's case table (tests/test_f32_model_cpu.py): accumulators within 2.57
(direct order) and 1.64 (Winograd order) of 2^-24 sqrt(K) B, results within 1.81 ulp32 where the ulp term is the larger
one.  The same CPU test shows that a dropped term, two swapped taps, 10-bit operands, exchanged scale / shift and unmasked
border taps all leave the bound on every case.  Worst error / bound measured on an MI355X per family: direct 3x3 0.36,
Winograd 0.15, transposed 0.23, plain 1x1 0.19, head 0.13.

Every case fills y over its whole pixel stride, and y_pool, with a NaN of a fixed bit pattern first; afterwards every
element the kernel owns is inside the bound, every other element still holds the pattern, and path_out names the instance
the case was written for (printed with the worst error / bound).  Tolerance-free on top: a strided or offset output, an
image run alone and a second launch give the very same bits as the dense batched run, and y_pool is the maximum over the
kernel's own y.

Not reached from here: wino_fits' fallback to the direct kernel past 2^34 input elements (host logic; no device buffer
of this suite is that large), and the bf16 store of the direct kernel (tests/test_bf16_ops_gpu.py, kernel 2 of
unet_op_conv_first_bf16)."""
import ctypes as C

import numpy as np
import pytest
import torch

import f32_model as M

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF      # a quiet NaN no kernel produces


@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load(build_if_missing=False)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _hp(t):
    return C.c_void_p(t.data_ptr())       # a contiguous CPU tensor


def sentinel(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda:0").view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def untouched(t):
    return bool((bits(t) == SENTINEL).all())


def run(lib, c, xd, w, scale, shift, ldo=0, co_off=0, pool=False, n=None, algo=None):
    """-> y over the whole stride (N,Ho,Wo,ldo or cout) on the device, y_pool or None, path_out"""
    n = c.n if n is None else n
    ho, wo = (2 * c.h, 2 * c.w) if c.kind == "up" else (c.h, c.w)
    y = sentinel((n, ho, wo, ldo or c.cout))
    yp = sentinel((n, c.h // 2, c.w // 2, c.cout)) if pool else None
    path = (C.c_int * 8)(*([-1] * 8))
    if c.kind == "conv":
        rc = lib.unet_op_conv3x3_f32(0, _p(xd), n, c.h, c.w, c.cin, _hp(w), _hp(scale), _hp(shift), c.cout, c.relu,
                                     c.algo if algo is None else algo, ldo, co_off, _p(y), _p(yp), path, None)
    elif c.kind == "up":
        rc = lib.unet_op_upconv2x2_f32(0, _p(xd), n, c.h, c.w, c.cin, _hp(w), _hp(shift), c.cout, ldo, co_off, _p(y), path, None)
    else:
        rc = lib.unet_op_conv1x1_f32(0, _p(xd), n, c.h, c.w, c.cin, _hp(w), c.cout, ldo, co_off, _p(y), path, None)
    assert rc == 0, (c.name, rc, lib.unet_op_last_error())      # also: no bounded wait of the Winograd kernel gave up
    return y, yp, list(path)


def host_plan(lib, c, n=None):
    q = M.plan_query(c)
    if n is not None:
        q[1] = n
    out = (C.c_int * 8)()
    assert lib.unet_host_plan_conv_f32((C.c_int * 7)(*q), 7, out, 8) == 0
    return list(out)


def owned(y, c, co_off):
    """the slice a call owns, and whether everything else still holds the sentinel"""
    mine = y[..., co_off:co_off + c.cout]
    rest = torch.cat([y[..., :co_off], y[..., co_off + c.cout:]], dim=-1)
    return mine, untouched(rest)


def check_bound(got, c, label):
    r, bound = M.reference(c.name)[:2]
    g = got.cpu().double().numpy()
    assert not np.isnan(g).any(), f"{label}: elements not written"
    ratio = np.abs(g - r) / bound
    worst = float(ratio.max())
    print(f"{label}: worst |got - r| / bound = {worst:.3f}")
    if worst > 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{label}: {int((ratio > 1).sum())} elements outside the bound; worst at {i}: got {g[i]!r} "
                             f"want {r[i]!r} (bound {bound[i]:.3e})")
    return worst


@pytest.mark.parametrize("c", M.CASES, ids=lambda c: c.name)
def test_gemm_kernels(lib, c):
    x, w, scale, shift = M.make_inputs(c.name)
    xd = x.cuda()
    plan = host_plan(lib, c)
    instance = M.check_plan(c, plan)
    fused = 1 if (c.algo == 2 and c.pool) else 0
    y, yp, path = run(lib, c, xd, w, scale, shift, pool=c.pool)
    assert path == plan[:7] + [fused], (path, plan)
    check_bound(y, c, f"{c.name} [{instance}]")
    if c.pool:       # the fused pool of the Winograd kernel, the pooling kernel behind the direct one: max over the kernel's y
        assert np.array_equal(yp.cpu().numpy().view(np.int32), M.pool_max(y.cpu().numpy()).view(np.int32)), "y_pool"
    if c.algo == 2:  # the wave-progress counters order the staging only: a second launch gives the same bits
        y2, yp2, _ = run(lib, c, xd, w, scale, shift, pool=c.pool)
        assert torch.equal(bits(y2), bits(y)) and torch.equal(bits(yp2), bits(yp)), "second launch differs"
    for ldo, co_off in c.slices:
        ys, yps, paths = run(lib, c, xd, w, scale, shift, ldo=ldo, co_off=co_off, pool=c.pool)
        mine, clean = owned(ys, c, co_off)
        assert paths == path
        assert clean, f"{c.name}: ldo {ldo} co_off {co_off}: wrote outside its channels"
        # a lane's accumulation order does not depend on where its result is stored
        assert torch.equal(bits(mine), bits(y)), f"{c.name}: ldo {ldo} co_off {co_off} differs from the dense run"
        if c.pool:
            assert torch.equal(bits(yps), bits(yp)), f"{c.name}: ldo {ldo} co_off {co_off}: y_pool differs"
        print(f"{c.name}: ldo {ldo} co_off {co_off}: bit-identical to the dense run, neighbours untouched")


ALONE = ["conv-3x16x128x7x9-hot-relu1", "conv-2x48x36x10x14-randn-relu0", "conv-9x16x64x14x16-relu-relu1",
         "conv-wino-3x16x32x2x6-randn-relu1", "conv-wino-5x48x20x14x14-relu-relu1", "conv-wino-2x128x64x16x48-relu-relu1",
         "up-2x16x12x7x16-randn-relu0", "c1-3x128x64x12x16-randn-relu0"]


@pytest.mark.parametrize("name", ALONE)
def test_image_alone_gives_the_same_bits(lib, name):
    """masked taps read a zero slot, so neither the tile an image's pixels fall into (tiles straddle images, and the
    tile choice itself depends on the batch) nor its neighbours in the batch change a lane's sum"""
    c = M.BY_NAME[name]
    x, w, scale, shift = M.make_inputs(name)
    xd = x.cuda()
    y, _, path = run(lib, c, xd, w, scale, shift)
    for i in sorted({0, c.n // 2, c.n - 1}):
        yi, _, pathi = run(lib, c, xd[i:i + 1].contiguous(), w, scale, shift, n=1)
        assert pathi[:7] == host_plan(lib, c, n=1)[:7]
        assert torch.equal(bits(yi[0]), bits(y[i])), f"{name}: image {i} alone differs (batch {path}, alone {pathi})"


def test_algo_0_is_the_forward_choice_and_refusals_launch_nothing(lib):
    c = M.BY_NAME["conv-wino-3x16x32x2x6-randn-relu1"]
    x, w, scale, shift = M.make_inputs(c.name)
    xd = x.cuda()
    yw, _, pw = run(lib, c, xd, w, scale, shift, algo=2)
    yd, _, pd = run(lib, c, xd, w, scale, shift, algo=1)
    y0, _, p0 = run(lib, c, xd, w, scale, shift, algo=0)
    assert pw[0] == 2 and pd[0] == 1 and p0 == pw and torch.equal(bits(y0), bits(yw))
    prev = lib.unet_set_winograd(0)
    try:
        y0, _, p0 = run(lib, c, xd, w, scale, shift, algo=0)
        assert p0 == pd and torch.equal(bits(y0), bits(yd))
        _, _, p2 = run(lib, c, xd, w, scale, shift, algo=2)      # a forced Winograd ignores the switch
        assert p2 == pw
    finally:
        lib.unet_set_winograd(prev)
    # odd height, cin % 16 != 0: a forced Winograd is refused and nothing is written
    y = sentinel((1, 3, 6, 32))
    assert lib.unet_op_conv3x3_f32(0, _p(xd), 1, 3, 6, 16, _hp(w), _hp(scale), _hp(shift), 32, 1, 2, 0, 0, _p(y), None, None,
                                   None) == 1
    assert lib.unet_op_conv3x3_f32(0, _p(xd), 1, 2, 6, 12, _hp(w), _hp(scale), _hp(shift), 32, 1, 2, 0, 0, _p(y), None, None,
                                   None) == 1
    torch.cuda.synchronize()
    assert untouched(y)


# ---- elementwise kernels --------------------------------------------------------------------------------------------

def _pool_input(shape, gen):
    """values on a coarse grid (equal maxima inside a window are common), both zeros among them"""
    x = torch.round(torch.randn(shape, generator=gen) * 2.0) / 2.0
    neg = torch.rand(shape, generator=gen) < 0.5
    return torch.where((x == 0) & neg, torch.tensor(-0.0), x).float()


@pytest.mark.parametrize("n,c,h,w", [(2, 4, 2, 2), (1, 12, 6, 10)])
@pytest.mark.parametrize("wide", [0, 1], ids=["ldi=c", "ldi=2c"])
def test_maxpool_bit_exact(lib, n, c, h, w, wide):
    ld = 2 * c if wide else c
    x = _pool_input((n, h, w, ld), torch.Generator().manual_seed(31 + c))
    assert bool(((x == 0) & torch.signbit(x)).any()) and bool(((x == 0) & ~torch.signbit(x)).any())
    y = sentinel((n, h // 2, w // 2, c))
    assert lib.unet_op_maxpool2x2_f32(0, _p(x.cuda()), n, h, w, c, ld if wide else 0, _p(y), None) == 0
    want = M.pool_max(x.numpy()[..., :c].copy())
    assert np.array_equal(y.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("wide", [0, 1], ids=["ldi=c", "ldi=2c"])
def test_maxpool_past_the_grid_cap(lib, wide):
    """n (h/2) (w/2) (c/4) = 3.1 M work items > 8192 blocks x 256 threads: the grid-stride loop runs twice"""
    n, c, h, w = 3, 64, 512, 512
    assert n * (h // 2) * (w // 2) * (c // 4) > 8192 * 256
    ld = 2 * c if wide else c
    x = torch.randn((n, h, w, ld), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(7))
    y = sentinel((n, h // 2, w // 2, c))
    assert lib.unet_op_maxpool2x2_f32(0, _p(x), n, h, w, c, ld, _p(y), None) == 0
    want = x.view(n, h // 2, 2, w // 2, 2, ld)[..., :c].amax(dim=(2, 4))      # the maximum is exact in any order
    assert torch.equal(bits(y), bits(want))


def _head(lib, x, w, bias, thr, label):
    npix, c = x.shape
    logits, probs = sentinel((npix,)), sentinel((npix,))
    mask = torch.full((npix,), 77, dtype=torch.uint8, device="cuda:0")
    assert lib.unet_op_head1x1_f32(0, _p(x.cuda()), 1, 1, npix, c, _hp(w), bias, thr, _p(logits), _p(probs), _p(mask), None) == 0
    z, B = M.head_reference(x.numpy(), w.numpy(), np.float32(bias))
    bound = M.C_ULP * M.ulp32(z) + M.C_ACC * M.U24 * np.sqrt(c) * B
    lg = logits.cpu().double().numpy()
    assert not np.isnan(lg).any(), label
    err = np.abs(lg - z)
    print(f"{label}: worst |logit - z| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (label, float((err / bound).max()))
    assert (np.abs(probs.cpu().double().numpy() - 1.0 / (1.0 + np.exp(-z))) <= 1e-6).all(), label
    m = mask.cpu().numpy()
    assert np.array_equal(m, (logits.cpu().numpy() > np.float32(thr)).astype(np.uint8) * 255), label
    sure = np.abs(z - np.float64(np.float32(thr))) > bound
    assert np.array_equal(m[sure], ((z > np.float32(thr)).astype(np.uint8) * 255)[sure]), label
    # each output alone: the others are optional
    only = sentinel((npix,))
    assert lib.unet_op_head1x1_f32(0, _p(x.cuda()), 1, 1, npix, c, _hp(w), bias, thr, None, _p(only), None, None) == 0
    assert torch.equal(bits(only), bits(probs))


@pytest.mark.parametrize("c", [4, 8, 12, 16, 24, 32, 64, 96, 256])
@pytest.mark.parametrize("thr", [0.0, 0.3])
def test_head(lib, c, thr):
    """all five LPP instances (c 4, 8, 16, 32, >= 64), channel counts that do not fill the last step (12, 24, 96), a pixel
    count that is no multiple of the 256 / LPP pixels of a block, more than one block"""
    g = torch.Generator().manual_seed(50 + c)
    npix = 3 * 13 * 11
    x = (3.0 * torch.relu(torch.randn(npix, c, generator=g)) + 0.5).float()
    w = (torch.randn(c, generator=g) * 0.3 / c ** 0.5).float()
    _head(lib, x, w, 0.17, thr, f"head c {c} thr {thr}")


def test_head_past_the_grid_cap(lib):
    npix = 1450 * 1450
    assert npix > 8192 * 256                      # c = 4: one lane per pixel, 256 pixels per block
    g = torch.Generator().manual_seed(9)
    x = torch.randn(npix, 4, generator=g)
    w = (torch.randn(4, generator=g) * 0.4).float()
    _head(lib, x, w, -0.05, 0.1, "head c 4, 2.1 M pixels")


def test_pack_u8(lib):
    """every byte value in every channel; (u8 - mean) / std with an exact division; pad channel +0.0"""
    g = torch.Generator().manual_seed(12)
    frames = torch.stack([torch.randperm(512, generator=g) % 256 for _ in range(3)], dim=-1).to(torch.uint8).reshape(1, 16, 32, 3)
    frames = torch.cat([frames, torch.randint(0, 256, (2, 16, 32, 3), generator=g, dtype=torch.uint8)])
    for ch in range(3):
        assert len(np.unique(frames[0, ..., ch].numpy())) == 256
    mean = np.array([123.675, 116.28, 103.53], np.float32)
    std = np.array([58.395, 57.12, 57.375], np.float32)
    y = sentinel((3, 16, 32, 4))
    assert lib.unet_op_pack_input_f32(0, _p(frames.cuda()), 1, 3, 16, 32, mean.ctypes.data_as(C.c_void_p),
                                      std.ctypes.data_as(C.c_void_p), _p(y), None) == 0
    got = y.cpu().numpy()
    assert np.array_equal(got.view(np.int32), M.pack_u8_reference(frames.numpy(), mean, std).view(np.int32))
    assert (got[..., 3].view(np.int32) == 0).all()


def test_pack_nchw(lib):
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 3, 5, 7, generator=g)
    x[0, 1, 2, 3] = -0.0
    y = sentinel((2, 5, 7, 4))
    assert lib.unet_op_pack_input_f32(0, _p(x.cuda()), 0, 2, 5, 7, None, None, _p(y), None) == 0
    got = y.cpu().numpy()
    assert np.array_equal(got[..., :3].view(np.int32), x.permute(0, 2, 3, 1).contiguous().numpy().view(np.int32))
    assert (got[..., 3].view(np.int32) == 0).all()
