"""bf16 tier, one operator at a time, against a float64 model of its own arithmetic.

The activations and weights of the tier are exact bf16 values, a bf16 x bf16 product is exact in fp32, so the only
error sources of a layer are the fp32 accumulation and the one final round-to-nearest-even to bf16.  A float64
evaluation of the same formula therefore pins every output to within one bf16 ulp:

  xb = the bf16 input as float64, wb = w rounded to bf16 (torch and the packers' host_f2bf both round to nearest even)
  z = conv(xb, wb), B = sqrt(conv(xb**2, wb**2)) (the L2 size of the terms), r = relu?(z * scale + shift)

  bound:    |got - r| <= ulp_bf16(|r|) + 2**-14 * |scale| * B   for every element.  fp32 accumulation of K terms errs by
            about 2**-24 * sqrt(K) * B (random-walk) and at most K * 2**-24 * sum|terms| <= K**1.5 * 2**-24 * B; for
            K <= 9 * 1024 the wide-margin term 2**-14 * B covers the first by > 10x.  A missing or misplaced term is
            about B / sqrt(K) >= B / 96, i.e. 170x the second term and far above one ulp of a typical output.
  budget:   the fraction of elements with got != bf16_rne(r) is at most 1 % (accumulation noise only flips the rounding
            of values within ~2**-24 * sqrt(K) * B of a rounding boundary; truncation instead of rounding would give
            about 50 %).  The measured fraction is printed for every case.

The kernel under test is forced through the `kernel` argument of the unet_op_*_bf16 entry points and each case asserts
through path_out that it ran (and whether the pool / head were fused), so every case proves the path it names."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from unet_lane_detection_amd import state as S

pytestmark = pytest.mark.gpu

IGEMM, WS, R512 = 1, 2, 3
NAMES = {0: "none", IGEMM: "igemm_bf16", WS: "ws", R512: "r512"}
SENTINEL = 0x7FC1          # a NaN bit pattern no kernel produces: marks elements a kernel must not write
ERR_INVALID_ARG = 1


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _h(a):
    """host float32 array -> pointer (the array must stay alive for the call)"""
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    lib = _lib.load(build_if_missing=False)
    prev = lib.unet_set_bf16_persistent(-1)
    yield lib
    lib.unet_set_bf16_persistent(prev)


# ---- float64 model ------------------------------------------------------------------------------------------------

def bf16_rne(t):
    """float64 -> nearest bf16 (through float32: the double rounding is negligible, see the module docstring)"""
    return t.to(torch.float32).to(torch.bfloat16)


def ulp_bf16(a):
    """one bf16 ulp at |a| (8 significant bits); the smallest normal's ulp at 0"""
    a = a.abs().clamp_min(2.0 ** -126)
    _, e = torch.frexp(a)
    return torch.ldexp(torch.ones_like(a), (e - 8).to(torch.int32))


def sentinel(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def is_sentinel(t):
    return t.view(torch.int16) == SENTINEL


def bf16_input(shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen, dtype=torch.float64) * scale).to(torch.bfloat16)


def conv_params(cin, cout, gen, taps=9):
    w = (torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5).float()
    sign = torch.where(torch.rand(cout, generator=gen) < 0.25, -1.0, 1.0)
    scale = ((torch.rand(cout, generator=gen) + 0.5) * sign).float()
    shift = (torch.randn(cout, generator=gen) * 0.3).float()
    return w, scale, shift


def check(got, z, B, scale, shift, relu, label, ran=None):
    """got (N,C,H,W) bf16 (any device), z / B float64 NCHW, scale / shift (C,) -> (worst error in ulps, mismatch)"""
    s = scale.double()[None, :, None, None]
    v = z * s + shift.double()[None, :, None, None]
    r = torch.relu(v) if relu else v
    g = got.cpu().double()
    assert not torch.isnan(g).any(), f"{label}: elements not written"
    ulp = ulp_bf16(r)
    err = (g - r).abs()
    bound = ulp + 2.0 ** -14 * s.abs() * B
    worst = (err / ulp).max().item()
    mism = (g != bf16_rne(r).double()).double().mean().item()
    print(f"{label} [{NAMES.get(ran, ran)}]: worst |got - r| {worst:.3g} ulp ({(err / bound).max().item():.3f} of the "
          f"bound), mismatch {mism:.2e}")
    bad = err > bound
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{label}: {int(bad.sum())} elements outside the bound; first at {i}: got "
                             f"{g[tuple(i)].item()} want {r[tuple(i)].item()} (bound {bound[tuple(i)].item():.3e})")
    assert mism <= 0.01, (label, mism)
    return worst, mism


def ref_conv(xb, wb):
    """xb (N,H,W,Cin) bf16 -> z, B float64 NCHW"""
    x = xb.cpu().double().permute(0, 3, 1, 2)
    w = wb.double()
    return F.conv2d(x, w, padding=1), F.conv2d(x * x, w * w, padding=1).sqrt()


def ref_upconv(xb, wb):
    """xb (N,H,W,Cin) bf16, wb (Cin,Cout,2,2) -> z, B float64 NCHW at (2H, 2W)"""
    x = xb.cpu().double().permute(0, 3, 1, 2)
    w = wb.double()
    return F.conv_transpose2d(x, w, stride=2), F.conv_transpose2d(x * x, w * w, stride=2).sqrt()


# ---- the entry points ---------------------------------------------------------------------------------------------

def run_conv(lib, xd, w, scale, shift, cout, relu, kernel, ldo=0, co_off=0, pool=False, y=None, expect_rc=0):
    n, h, wd, cin = xd.shape
    if y is None:
        y = sentinel((n, h, wd, ldo or cout))
    yp = sentinel((n, h // 2, wd // 2, cout)) if pool else None
    path = (C.c_int * 3)()
    wn, sn, hn = w.numpy(), scale.numpy(), shift.numpy()
    rc = lib.unet_op_conv3x3_bf16(0, _p(xd), n, h, wd, cin, _h(wn), _h(sn), _h(hn), cout, relu, kernel, ldo, co_off,
                                  _p(y), _p(yp), path, None)
    assert rc == expect_rc, (rc, kernel, xd.shape, cout)
    return y, yp, list(path)


def run_upconv(lib, xd, w, bias, cout, kernel, ldo=0, co_off=0, y=None, expect_rc=0):
    n, h, wd, cin = xd.shape
    if y is None:
        y = sentinel((n, 2 * h, 2 * wd, ldo or cout))
    path = (C.c_int * 3)()
    wn, bn = w.numpy(), bias.numpy()
    rc = lib.unet_op_upconv2x2_bf16(0, _p(xd), n, h, wd, cin, _h(wn), _h(bn), cout, kernel, ldo, co_off, _p(y), path,
                                    None)
    assert rc == expect_rc, (rc, kernel, xd.shape, cout)
    return y, list(path)


def nchw(y, c0=0, c1=None):
    return y[..., c0:c1].permute(0, 3, 1, 2)


# ---- the 2x2-wave kernel's dispatch (run_igemm_bf in csrc/unet_bf16.inc), for labelling and coverage ----------------

def choose_tile(nh, w):
    """csrc/unet_hip.cpp choose_tile(nh, w, 16, halo = true) -> (ms, th, tw)"""
    best, best_cost = (4, 8, 16), 1e30
    for ms in (7, 4):
        bm = 32 * ms
        nld = 6 if ms == 7 else 4
        for tw in range(2, bm + 1):
            if bm % tw:
                continue
            th = bm // tw
            hp = (th + 2) * (tw + 2)
            if hp * 4 > nld * 256:
                continue
            pad_w = ((w + tw - 1) // tw * tw) / w
            pad_h = ((nh + th - 1) // th * th) / nh
            cost = pad_w * pad_h * (1.0 + 0.02 * hp / (th * tw)) * (0.97 if ms == 7 else 1.0)
            if cost < best_cost:
                best_cost, best = cost, (ms, th, tw)
    return best


def igemm_plan(n, h, w, cout):
    ms, th, tw = choose_tile(n * h, w)
    n_total = -(-cout // (128 if cout >= 128 else 64)) * (128 if cout >= 128 else 64)
    ns = 4 if n_total % 128 == 0 else 2
    co_tiles = n_total // (32 * ns)
    group = next((g for g in (8, 4, 2) if co_tiles % g == 0), 1)
    pool = th % 4 == 0 and tw % 2 == 0 and h % 2 == 0 and w % 2 == 0
    return dict(ms=ms, th=th, tw=tw, ns=ns, group=group, pool=pool, head=co_tiles == 1)


# ---- 3x3 convolution: igemm_bf16 ----------------------------------------------------------------------------------

# (n, cin, cout, h, w): one chunk / an odd chunk count / many chunks; coutPad and channel tails; images taller than no
# tile so tiles straddle two images; maps smaller than a tile; both pixel tiles, both channel-tile widths, coGroup 8/4/2/1
IGEMM_CASES = [(2, 32, 32, 10, 12), (1, 96, 96, 9, 20), (1, 1024, 384, 6, 10), (3, 64, 192, 7, 9), (1, 64, 1024, 8, 8),
               (1, 64, 512, 5, 6), (4, 32, 64, 2, 2), (2, 64, 64, 3, 5), (1, 128, 128, 28, 32), (2, 64, 64, 56, 56),
               (3, 96, 32, 13, 30)]


def test_igemm_cases_cover_the_dispatch():
    plans = [igemm_plan(n, h, w, cout) for n, cin, cout, h, w in IGEMM_CASES]
    assert {p["ms"] for p in plans} == {4, 7}
    assert {p["ns"] for p in plans} == {2, 4}
    assert {(p["ms"], p["ns"]) for p in plans} >= {(7, 2), (7, 4), (4, 2), (4, 4)}
    assert {p["group"] for p in plans} == {1, 2, 4, 8}
    # tiles that straddle two images: n > 1 and H not a multiple of the tile height
    assert any(n > 1 and h % p["th"] for (n, _, _, h, _), p in zip(IGEMM_CASES, plans))


@pytest.mark.parametrize("n,cin,cout,h,w", IGEMM_CASES)
def test_conv3x3_igemm_vs_float64(lib, n, cin, cout, h, w):
    g = torch.Generator().manual_seed(n * 1000 + cin + 3 * cout + 7 * h + w)
    xb = bf16_input((n, h, w, cin), g)
    wt, scale, shift = conv_params(cin, cout, g)
    z, B = ref_conv(xb, bf16_rne(wt.double()))
    xd = xb.cuda()
    p = igemm_plan(n, h, w, cout)
    for relu in (1, 0):
        y, _, path = run_conv(lib, xd, wt, scale, shift, cout, relu, IGEMM)
        assert path == [IGEMM, 0, 0]
        check(nchw(y), z, B, scale, shift, relu, f"igemm conv n{n} {cin}->{cout} {h}x{w} relu{relu} ms{p['ms']} "
              f"ns{p['ns']} g{p['group']}", path[0])


# fused pool (relu 0 and 1: the kernel's float max must be exact on negative values too), ldo = 2 cout with
# co_off 0 and cout (the concat buffer's two halves)
IGEMM_POOL_CASES = [(2, 64, 64, 16, 16), (1, 32, 96, 8, 28), (3, 64, 128, 6, 10), (1, 64, 64, 20, 24)]


@pytest.mark.parametrize("n,cin,cout,h,w", IGEMM_POOL_CASES)
def test_conv3x3_igemm_pool_and_concat_half(lib, n, cin, cout, h, w):
    g = torch.Generator().manual_seed(17 * n + cin + cout + h * w)
    xb = bf16_input((n, h, w, cin), g)
    wt, scale, shift = conv_params(cin, cout, g)
    z, B = ref_conv(xb, bf16_rne(wt.double()))
    xd = xb.cuda()
    plan = igemm_plan(n, h, w, cout)
    assert plan["pool"], plan
    for relu in (1, 0):
        for co_off in (0, cout):
            y, yp, path = run_conv(lib, xd, wt, scale, shift, cout, relu, IGEMM, ldo=2 * cout, co_off=co_off, pool=True)
            assert path == [IGEMM, 1, 0], path
            lab = f"igemm conv+pool n{n} {cin}->{cout} {h}x{w} relu{relu} co_off{co_off}"
            check(nchw(y, co_off, co_off + cout), z, B, scale, shift, relu, lab, path[0])
            other = y[..., cout:] if co_off == 0 else y[..., :cout]
            assert is_sentinel(other).all(), lab + ": wrote outside [co_off, co_off + cout)"
            want = F.max_pool2d(nchw(y, co_off, co_off + cout).float(), 2).to(torch.bfloat16)
            assert torch.equal(nchw(yp), want), lab + ": fused pool differs from the 2x2 max of y"


# ---- 3x3 convolution: conv_bf16_ws --------------------------------------------------------------------------------

def ws_work(n, h, w, cout):
    return -(-w // 32) * (n * h // 16) * (cout // 64)


# (n, cin, cout, h, w): w % 32 != 0 (partial last tile), several images, cout 64 / 192 (odd coTiles) / 512 (MAX_COUT),
# cin 64 / 512, work exactly 8 (the smallest persistent grid) and 15 (one block short of a second round: the tail)
WS_CASES = [(2, 64, 64, 32, 40), (3, 64, 192, 16, 48), (1, 64, 512, 16, 32), (8, 512, 64, 16, 4), (1, 64, 64, 240, 20),
            (3, 64, 64, 32, 40), (1, 512, 512, 16, 4), (2, 128, 128, 32, 72)]


@pytest.mark.parametrize("n,cin,cout,h,w", WS_CASES)
def test_conv3x3_ws_vs_float64(lib, n, cin, cout, h, w):
    g = torch.Generator().manual_seed(31 * n + cin + cout + h + 5 * w)
    xb = bf16_input((n, h, w, cin), g)
    wt, scale, shift = conv_params(cin, cout, g)
    z, B = ref_conv(xb, bf16_rne(wt.double()))
    xd = xb.cuda()
    work = ws_work(n, h, w, cout)
    assert work >= 8
    pool_ok = h % 2 == 0 and w % 2 == 0
    for relu in (1, 0):
        # EPI 1 (fused pool) with relu; EPI 0 without - the packed max is only order-preserving on non-negative bf16
        y, yp, path = run_conv(lib, xd, wt, scale, shift, cout, relu, WS, pool=pool_ok)
        fused = 1 if (relu and pool_ok) else 0
        assert path == [WS, fused, 0], path
        lab = f"ws conv n{n} {cin}->{cout} {h}x{w} work{work} relu{relu} pool{fused}"
        check(nchw(y), z, B, scale, shift, relu, lab, path[0])
        if fused:
            want = F.max_pool2d(nchw(y).float(), 2).to(torch.bfloat16)
            assert torch.equal(nchw(yp), want), lab
        elif pool_ok:
            assert is_sentinel(yp).all(), lab + ": pool written although not fused"
        # against the 2x2-wave kernel: each holds the float64 criteria on its own; report where they differ
        y1, _, p1 = run_conv(lib, xd, wt, scale, shift, cout, relu, IGEMM)
        assert p1[0] == IGEMM
        diff = (y.view(torch.int16) != y1.view(torch.int16)).double().mean().item()
        print(f"{lab}: differs from igemm_bf16 in {diff:.2e} of the elements")


def test_conv3x3_ws_concat_half(lib):
    n, cin, cout, h, w = 2, 64, 128, 16, 40
    g = torch.Generator().manual_seed(5)
    xb = bf16_input((n, h, w, cin), g)
    wt, scale, shift = conv_params(cin, cout, g)
    z, B = ref_conv(xb, bf16_rne(wt.double()))
    xd = xb.cuda()
    for co_off in (0, cout):
        y, yp, path = run_conv(lib, xd, wt, scale, shift, cout, 1, WS, ldo=2 * cout, co_off=co_off, pool=True)
        assert path == [WS, 1, 0]
        lab = f"ws conv+pool ldo {2 * cout} co_off {co_off}"
        check(nchw(y, co_off, co_off + cout), z, B, scale, shift, 1, lab, path[0])
        assert is_sentinel(y[..., cout:] if co_off == 0 else y[..., :cout]).all(), lab
        assert torch.equal(nchw(yp), F.max_pool2d(nchw(y, co_off, co_off + cout).float(), 2).to(torch.bfloat16)), lab


# ---- 3x3 convolution: conv_bf16_r512 ------------------------------------------------------------------------------

def r512_plan(n, h, w, cout):
    """conv_bf_r512_plan in csrc/unet_bf16.inc -> (twx, wpx, flat)"""
    twx = 14 if w == 14 else 28
    thx = 224 // twx
    flat = n > 1 and h % thx != 0 and 2 * h >= thx
    tiles = ((n * h + thx - 1) // thx) * (w // twx) if flat else n * ((h + thx - 1) // thx) * (w // twx)

    def bal(items):
        return items / ((items + 255) // 256 * 256)
    wpx = 2
    if cout % 256 == 0:
        wpx = 1 if bal(tiles * (cout // 256)) >= 0.93 * bal(tiles * (cout // 128)) else 2
    return twx, wpx, flat


# (n, cin, cout, h, w, checked images): widths 28 / 56 / 84 (TWX 28) and 14 (TWX 14); cout 128 / 256 / 512; the flat
# tall-image mode with a last tile that ends inside an image; one chunk pair and many chunks; WPX 1 (which takes more
# tiles than a float64 check of every image affords: there a subset of the images, first / middle / last, is checked)
R512_CASES = [(1, 64, 128, 8, 28, None), (2, 128, 256, 8, 56, None), (1, 64, 256, 8, 84, None),
              (3, 64, 128, 14, 14, None), (3, 64, 256, 6, 28, None), (1, 1024, 128, 8, 28, None),
              (2, 64, 512, 10, 28, None), (35, 64, 512, 16, 28, [0, 17, 34]), (74, 64, 512, 14, 14, [0, 1, 36, 73])]


def test_r512_cases_cover_the_dispatch():
    plans = [r512_plan(n, h, w, cout) for n, cin, cout, h, w, _ in R512_CASES]
    assert {(t, p) for t, p, _ in plans} == {(28, 1), (28, 2), (14, 1), (14, 2)}
    assert {f for _, _, f in plans} == {True, False}


@pytest.mark.parametrize("n,cin,cout,h,w,imgs", R512_CASES)
def test_conv3x3_r512_vs_float64(lib, n, cin, cout, h, w, imgs):
    g = torch.Generator().manual_seed(13 * n + cin + cout + h + w)
    xb = bf16_input((n, h, w, cin), g)
    wt, scale, shift = conv_params(cin, cout, g)
    sel = slice(None) if imgs is None else imgs
    z, B = ref_conv(xb[sel], bf16_rne(wt.double()))
    xd = xb.cuda()
    twx, wpx, flat = r512_plan(n, h, w, cout)
    for relu in (1, 0):
        y, _, path = run_conv(lib, xd, wt, scale, shift, cout, relu, R512)
        assert path == [R512, 0, 0], path
        lab = f"r512 conv n{n} {cin}->{cout} {h}x{w} twx{twx} wpx{wpx} flat{int(flat)} relu{relu}"
        check(nchw(y)[sel], z, B, scale, shift, relu, lab, path[0])
        # the same chunk / tap accumulation order as the 2x2-wave kernel, so the same bits
        y1, _, p1 = run_conv(lib, xd, wt, scale, shift, cout, relu, IGEMM)
        assert p1[0] == IGEMM
        assert torch.equal(y.view(torch.int16), y1.view(torch.int16)), lab + ": not bit-identical to igemm_bf16"


def test_conv3x3_r512_concat_half(lib):
    n, cin, cout, h, w = 2, 64, 128, 8, 28
    g = torch.Generator().manual_seed(9)
    xb = bf16_input((n, h, w, cin), g)
    wt, scale, shift = conv_params(cin, cout, g)
    z, B = ref_conv(xb, bf16_rne(wt.double()))
    for co_off in (0, cout):
        y, yp, path = run_conv(lib, xb.cuda(), wt, scale, shift, cout, 1, R512, ldo=2 * cout, co_off=co_off, pool=True)
        assert path == [R512, 0, 0]          # no fused pool: the standalone pass runs in the network
        assert is_sentinel(yp).all()
        check(nchw(y, co_off, co_off + cout), z, B, scale, shift, 1, f"r512 conv co_off {co_off}", path[0])
        assert is_sentinel(y[..., cout:] if co_off == 0 else y[..., :cout]).all()


# ---- the last convolution with the fused 1x1 head ----------------------------------------------------------------

def run_head_conv(lib, xd, w, scale, shift, cout, relu, kernel, hw, hb, thr):
    n, h, wd, cin = xd.shape
    logits = torch.full((n, h, wd), float("nan"), device="cuda")
    probs = torch.full((n, h, wd), float("nan"), device="cuda")
    mask = torch.full((n, h, wd), 7, dtype=torch.uint8, device="cuda")
    path = (C.c_int * 3)()
    wn, sn, hn, hwn = w.numpy(), scale.numpy(), shift.numpy(), hw.numpy()
    rc = lib.unet_op_conv3x3_bf16_head(0, _p(xd), n, h, wd, cin, _h(wn), _h(sn), _h(hn), cout, relu, kernel, _h(hwn),
                                       hb, thr, _p(logits), _p(probs), _p(mask), path, None)
    assert rc == 0, rc
    return logits, probs, mask, list(path)


def check_head(logits, probs, mask, ref, bound, thr, label):
    lg = logits.cpu().double()
    err = (lg - ref).abs()
    print(f"{label}: worst |logit - ref| / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all(), (label, err.max().item())
    pr = probs.cpu().double()
    assert ((pr - torch.sigmoid(lg)).abs() <= 1e-6).all(), label
    assert torch.equal(mask.cpu(), ((logits > thr).to(torch.uint8) * 255).cpu()), label


# (n, cin, cout, h, w, kernel, fused): fused on igemm_bf16 (one channel tile) and on ws (EPI 2, cout 64); the unfused
# fallback to head1x1_bf16 where the kernel cannot fuse it (igemm with two channel tiles, ws with cout 128)
HEAD_CASES = [(2, 64, 64, 12, 20, IGEMM, 1), (2, 128, 64, 32, 40, WS, 1), (4, 64, 64, 16, 64, WS, 1),
              (1, 64, 256, 6, 10, IGEMM, 0), (2, 64, 128, 16, 48, WS, 0), (1, 64, 32, 9, 7, IGEMM, 1)]


@pytest.mark.parametrize("n,cin,cout,h,w,kernel,fused", HEAD_CASES)
def test_conv3x3_head_vs_float64(lib, n, cin, cout, h, w, kernel, fused):
    g = torch.Generator().manual_seed(3 * n + cin + cout + h + w + kernel)
    xb = bf16_input((n, h, w, cin), g)
    wt, scale, shift = conv_params(cin, cout, g)
    hw = (torch.randn(cout, generator=g) * (4.0 / cout) ** 0.5).float()
    hb, thr = -0.25, 0.1
    z, B = ref_conv(xb, bf16_rne(wt.double()))
    s = scale.double()[None, :, None, None]
    for relu in (1, 0):
        v = z * s + shift.double()[None, :, None, None]
        r = torch.relu(v) if relu else v
        a = bf16_rne(r).double()
        # each activation is within ulp + 2**-14 |scale| B of r (the criteria above), so of bf16(r) within twice that;
        # through |hw| that sums to the first term; the fp32 dot of cout terms adds at most (cout + 2) 2**-24 sum|a hw|
        hwd = hw.double()[None, :, None, None]
        ref = (a * hwd).sum(1) + hb
        bound = ((2 * ulp_bf16(r) + 2.0 ** -14 * s.abs() * B) * hwd.abs()).sum(1) + \
            (cout + 2) * 2.0 ** -24 * ((a * hwd).abs().sum(1) + abs(hb))
        xd = xb.cuda()
        logits, probs, mask, path = run_head_conv(lib, xd, wt, scale, shift, cout, relu, kernel, hw, hb, thr)
        assert path == [kernel, 0, fused], path
        lab = f"head conv [{NAMES[kernel]}] fused{fused} n{n} {cin}->{cout} {h}x{w} relu{relu}"
        check_head(logits, probs, mask, ref, bound, thr, lab)
        # sharper: against the activation the same kernel stores (checked against float64 by the tests above), the
        # head's only error is its own fp32 dot product
        y, _, p1 = run_conv(lib, xd, wt, scale, shift, cout, relu, kernel)
        assert p1[0] == kernel
        prod = y.cpu().double() * hw.double()
        check_head(logits, probs, mask, prod.sum(-1) + hb, (cout + 2) * 2.0 ** -24 * (prod.abs().sum(-1) + abs(hb)), thr,
                   lab + " vs its stored activation")


# ---- transposed convolution ---------------------------------------------------------------------------------------

def upconv_params(cin, cout, gen):
    w = (torch.randn(cin, cout, 2, 2, generator=gen) * (1.0 / cin) ** 0.5).float()
    bias = (torch.randn(cout, generator=gen) * 0.1).float()
    return w, bias


def check_upconv(y, z, B, bias, label, ran):
    one = torch.ones_like(bias)
    for a in (0, 1):
        for b in (0, 1):
            check(y[:, :, a::2, b::2], z[:, :, a::2, b::2], B[:, :, a::2, b::2], one, bias, 0,
                  f"{label} (a,b)=({a},{b})", ran)


# (n, cin, cout, h, w, kernel): npix not a multiple of 128 (ws) / 224 (r512); w = 4 (r512's minimum); cin 128 / 1024;
# cout 64 ... 512; the 2x2-wave kernel at cin / cout that are not multiples of 64
UPCONV_CASES = [(2, 128, 128, 10, 30, WS), (1, 1024, 512, 4, 4, WS), (5, 256, 192, 7, 9, WS), (4, 128, 64, 16, 20, WS),
                (1, 128, 64, 4, 4, R512), (3, 256, 128, 7, 10, R512), (1, 1024, 512, 5, 12, R512),
                (2, 128, 256, 9, 13, R512), (2, 32, 32, 5, 7, IGEMM), (1, 96, 96, 6, 6, IGEMM),
                (2, 128, 64, 16, 20, IGEMM), (1, 1024, 64, 3, 5, IGEMM)]


@pytest.mark.parametrize("n,cin,cout,h,w,kernel", UPCONV_CASES)
def test_upconv_vs_float64(lib, n, cin, cout, h, w, kernel):
    g = torch.Generator().manual_seed(7 * n + cin + cout + h + w + kernel)
    xb = bf16_input((n, h, w, cin), g)
    wt, bias = upconv_params(cin, cout, g)
    z, B = ref_upconv(xb, bf16_rne(wt.double()))
    xd = xb.cuda()
    y, path = run_upconv(lib, xd, wt, bias, cout, kernel)
    assert path[0] == kernel, path
    lab = f"upconv n{n} {cin}->{cout} {h}x{w}"
    check_upconv(nchw(y), z, B, bias, lab, kernel)
    # the decoder's write: channels [cout, 2 cout) of a 2 cout concat buffer, the skip half untouched
    y2, path = run_upconv(lib, xd, wt, bias, cout, kernel, ldo=2 * cout, co_off=cout)
    assert path[0] == kernel
    assert is_sentinel(y2[..., :cout]).all(), lab + ": wrote into the skip half"
    assert torch.equal(y2[..., cout:].view(torch.int16), y.view(torch.int16)), lab
    if kernel == R512 and cin % 64 == 0:
        ws_ok = -(-(n * h * w) // 128) * (cout // 64) >= 8
        if ws_ok:   # the two structures accumulate chunk by chunk in the same order: bit-identical
            yw, pw = run_upconv(lib, xd, wt, bias, cout, WS)
            assert pw[0] == WS
            assert torch.equal(yw.view(torch.int16), y.view(torch.int16)), lab + ": r512 differs from ws"


@pytest.mark.parametrize("n,cin,cout,h,w", [(4, 128, 64, 16, 20), (1, 1024, 512, 4, 4), (2, 256, 256, 14, 14)])
def test_upconv_r512_bit_identical_to_ws(lib, n, cin, cout, h, w):
    g = torch.Generator().manual_seed(n + cin + cout)
    xd = bf16_input((n, h, w, cin), g).cuda()
    wt, bias = upconv_params(cin, cout, g)
    yr, pr = run_upconv(lib, xd, wt, bias, cout, R512, ldo=2 * cout, co_off=cout)
    yw, pw = run_upconv(lib, xd, wt, bias, cout, WS, ldo=2 * cout, co_off=cout)
    assert pr[0] == R512 and pw[0] == WS
    assert torch.equal(yr.view(torch.int16), yw.view(torch.int16))


# ---- the first convolution ----------------------------------------------------------------------------------------

def run_first(lib, frames, w, scale, shift, cout, relu, kernel, expect_rc=0):
    n, h, wd, _ = frames.shape
    y = sentinel((n, h, wd, cout))
    path = (C.c_int * 3)()
    mean = np.asarray(S.INPUT_MEAN, dtype=np.float32)
    std = np.asarray(S.INPUT_STD, dtype=np.float32)
    wn, sn, hn = w.numpy(), scale.numpy(), shift.numpy()
    rc = lib.unet_op_conv_first_bf16(0, _p(frames), n, h, wd, _h(wn), _h(sn), _h(hn), cout, relu, _h(mean), _h(std),
                                     kernel, _p(y), path, None)
    assert rc == expect_rc, rc
    return y, list(path)


def split_hi_lo(t32):
    """conv_first_bf16x3.h / pack_first_bf16x3: hi = bf16(v), lo = bf16(v - hi) (v - hi exact in fp32)"""
    hi = t32.to(torch.bfloat16).float()
    lo = (t32 - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


# (n, h, w, cout): w not a multiple of 32, h 8 and 40, cout 64 and 128; the fp32 kernel also where the fused kernel
# cannot run (h % 8, cout % 64)
FIRST_CASES = [(2, 8, 44, 64, 1), (1, 40, 36, 128, 1), (3, 16, 32, 64, 1), (2, 8, 44, 64, 2), (1, 40, 36, 128, 2),
               (2, 12, 20, 96, 2)]


@pytest.mark.parametrize("n,h,w,cout,kernel", FIRST_CASES)
def test_conv_first_vs_float64(lib, n, h, w, cout, kernel):
    g = torch.Generator().manual_seed(n + h + w + cout + kernel)
    frames = torch.from_numpy(S.synthetic_frames(n, h, w, seed=h + w))
    wt = (torch.randn(cout, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5).float()
    scale = ((torch.rand(cout, generator=g) + 0.5) * torch.where(torch.rand(cout, generator=g) < 0.25, -1.0, 1.0)).float()
    shift = (torch.randn(cout, generator=g) * 0.3).float()
    mean = torch.tensor(S.INPUT_MEAN, dtype=torch.float32)[None, :, None, None]
    std = torch.tensor(S.INPUT_STD, dtype=torch.float32)[None, :, None, None]
    # the kernels' normalisation, in fp32 with the same two correctly rounded operations
    xn = (frames.permute(0, 3, 1, 2).float() - mean) / std
    s = scale.double()[None, :, None, None]
    full = F.conv2d(xn.double(), wt.double(), padding=1)
    terms = F.conv2d(xn.double().abs(), wt.double().abs(), padding=1)
    if kernel == 1:
        # emulate the split: wh.xh + wh.xl + wl.xh, every product exact in fp32
        xh, xl = split_hi_lo(xn)
        wh, wl = split_hi_lo(wt)
        z = F.conv2d(xh, wh, padding=1) + F.conv2d(xl, wh, padding=1) + F.conv2d(xh, wl, padding=1)
        B = (F.conv2d(xh * xh, wh * wh, padding=1) + F.conv2d(xl * xl, wh * wh, padding=1) +
             F.conv2d(xh * xh, wl * wl, padding=1)).sqrt()
    else:
        # the fp32 kernel: fp32 input and weights
        z = full
        B = F.conv2d(xn.double() ** 2, wt.double() ** 2, padding=1).sqrt()
    for relu in (1, 0):
        y, path = run_first(lib, frames.cuda(), wt, scale, shift, cout, relu, kernel)
        assert path[0] == kernel, path
        name = "conv_first_bf16x3" if kernel == 1 else "fp32 kernel, bf16 store"
        lab = f"first conv n{n} {h}x{w} ->{cout} relu{relu}"
        check(nchw(y), z, B, scale, shift, relu, lab, name)
        # DESIGN 4.4's accuracy class for the split: the unsplit float64 convolution within ulp + 2**-13 |scale| sum|terms|
        v = full * s + shift.double()[None, :, None, None]
        r = torch.relu(v) if relu else v
        err = (nchw(y).cpu().double() - r).abs()
        assert (err <= ulp_bf16(r) + 2.0 ** -13 * s.abs() * terms).all(), lab + ": outside the split's accuracy class"


# ---- the unfused max-pool and head --------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w,c", [(2, 6, 10, 32), (1, 4, 4, 512), (3, 8, 6, 96), (1, 14, 14, 256)])
def test_maxpool2x2_bf16_exact(lib, n, h, w, c):
    g = torch.Generator().manual_seed(n + h + w + c)
    x = bf16_input((n, h, w, 2 * c), g).cuda()        # ldi = 2c: the concat buffer's skip half
    y = sentinel((n, h // 2, w // 2, c))
    assert lib.unet_op_maxpool2x2_bf16(0, _p(x), n, h, w, c, 2 * c, _p(y), None) == 0
    want = F.max_pool2d(nchw(x, 0, c).float(), 2).to(torch.bfloat16)
    assert torch.equal(nchw(y), want)


@pytest.mark.parametrize("c", [8, 16, 32, 64, 128, 256])      # every LPP instance of head1x1_bf16_kernel (1 ... 16)
def test_head1x1_bf16_vs_float64(lib, c):
    n, h, w = 2, 9, 13
    g = torch.Generator().manual_seed(c)
    x = bf16_input((n, h, w, c), g)
    hw = (torch.randn(c, generator=g) * (4.0 / c) ** 0.5).float()
    hb, thr = -0.25, -0.05
    xd = x.cuda()
    logits = torch.full((n, h, w), float("nan"), device="cuda")
    probs = torch.full((n, h, w), float("nan"), device="cuda")
    mask = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda")
    hwn = hw.numpy()
    assert lib.unet_op_head1x1_bf16(0, _p(xd), n, h, w, c, _h(hwn), hb, thr, _p(logits), _p(probs), _p(mask), None) == 0
    prod = x.double() * hw.double()
    ref = prod.sum(-1) + hb
    bound = (c + 2) * 2.0 ** -24 * (prod.abs().sum(-1) + abs(hb))    # recursive fp32 summation of c + 1 terms
    check_head(logits, probs, mask, ref, bound, thr, f"head1x1_bf16 c{c}")


# ---- rejections ---------------------------------------------------------------------------------------------------

def test_forced_kernels_reject_shapes_they_cannot_take(lib):
    g = torch.Generator().manual_seed(1)
    conv_rejects = [  # (n, cin, cout, h, w, kernel): why
        (1, 64, 64, 8, 32, WS),        # H % 16
        (2, 96, 64, 16, 32, WS),       # Cin % 64: no ws packing
        (1, 64, 64, 16, 32, WS),       # work 1 < 8: the persistent grid would be empty
        (1, 64, 1024, 16, 64, WS),     # Cout > MAX_COUT
        (1, 64, 128, 8, 30, R512),     # W neither a multiple of 28 nor 14
        (1, 64, 64, 8, 28, R512),      # Cout % 128
        (1, 96, 128, 8, 28, R512),     # Cin % 64: no packing
    ]
    for n, cin, cout, h, w, k in conv_rejects:
        xd = bf16_input((n, h, w, cin), g).cuda()
        wt, scale, shift = conv_params(cin, cout, g)
        y, yp, path = run_conv(lib, xd, wt, scale, shift, cout, 1, k, pool=True, expect_rc=ERR_INVALID_ARG)
        assert path == [0, 0, 0], (n, cin, cout, h, w, k, path)
        assert is_sentinel(y).all() and is_sentinel(yp).all()
    up_rejects = [
        (1, 64, 64, 8, 8, R512),       # Cin % 128
        (4, 128, 64, 8, 2, R512),      # w < 4
        (1, 96, 64, 8, 8, WS),         # Cin % 64: no packing
        (1, 128, 64, 8, 16, WS),       # work 1 < 8
    ]
    for n, cin, cout, h, w, k in up_rejects:
        xd = bf16_input((n, h, w, cin), g).cuda()
        wt, bias = upconv_params(cin, cout, g)
        y, path = run_upconv(lib, xd, wt, bias, cout, k, expect_rc=ERR_INVALID_ARG)
        assert path == [0, 0, 0], (n, cin, cout, h, w, k, path)
        assert is_sentinel(y).all()
    for n, h, w, cout in ((1, 12, 32, 64), (1, 8, 32, 96)):   # conv_first_bf16x3: H % 8, Cout % 64
        frames = torch.from_numpy(S.synthetic_frames(n, h, w, seed=0)).cuda()
        wt = torch.randn(cout, 3, 3, 3, generator=g).float()
        y, path = run_first(lib, frames, wt, torch.ones(cout), torch.zeros(cout), cout, 1, 1, expect_rc=ERR_INVALID_ARG)
        assert path == [0, 0, 0] and is_sentinel(y).all()


# ---- the network as the composition of the operators above, bit for bit -------------------------------------------

def fold_bn(sd, prefix, conv_idx, bn_idx):
    """fold_bn_and_build in csrc/unet_hip.cpp, in float32: 1 / sqrt(var + 1e-5f), gamma * inv, beta - mean * scale"""
    bn = f"{prefix}.{bn_idx}."
    g, b, m, v = (sd[bn + k].astype(np.float32) for k in ("weight", "bias", "running_mean", "running_var"))
    inv = np.float32(1.0) / np.sqrt(v + np.float32(1e-5))
    scale = (g * inv).astype(np.float32)
    shift = (b - (m * scale).astype(np.float32)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(sd[f"{prefix}.{conv_idx}.weight"])), torch.from_numpy(scale), \
        torch.from_numpy(shift)


def chain_forward(lib, sd, feats, frames, paths):
    """unet_forward_u8_bf16 (csrc/unet_bf16.inc) as a sequence of unet_op_*_bf16 calls with kernel 0 (the network's
    choice): the skip written into the concat buffer with ldo = 2f, pooled in the epilogue or by the standalone pass as
    path_out says, the transposed convolution at co_off = f, the last convolution with the head."""
    n, h, w, _ = frames.shape
    depth = len(feats)
    w0, s0, b0 = fold_bn(sd, "encoder_blocks.0", 0, 1)
    cur, path = run_first(lib, frames, w0, s0, b0, feats[0], 1, 0)
    paths.append(("first", path))
    ch, cw = h, w
    cats = []
    for l in range(depth):
        f = feats[l]
        p = f"encoder_blocks.{l}"
        if l > 0:
            wt, sc, sh = fold_bn(sd, p, 0, 1)
            cur, _, path = run_conv(lib, cur, wt, sc, sh, f, 1, 0)
            paths.append((f"{p}.0", path))
        wt, sc, sh = fold_bn(sd, p, 3, 4)
        cat = sentinel((n, ch, cw, 2 * f))
        cat, pool, path = run_conv(lib, cur, wt, sc, sh, f, 1, 0, ldo=2 * f, co_off=0, pool=True, y=cat)
        paths.append((f"{p}.3", path))
        if not path[1]:
            assert lib.unet_op_maxpool2x2_bf16(0, _p(cat), n, ch, cw, f, 2 * f, _p(pool), None) == 0
        cats.append(cat)
        cur = pool
        ch //= 2
        cw //= 2
    fb = 2 * feats[-1]
    for conv_idx, bn_idx in ((0, 1), (3, 4)):
        wt, sc, sh = fold_bn(sd, "bottleneck", conv_idx, bn_idx)
        cur, _, path = run_conv(lib, cur, wt, sc, sh, fb, 1, 0)
        paths.append((f"bottleneck.{conv_idx}", path))
    for j in range(depth):
        l = depth - 1 - j
        f = feats[l]
        pu = f"decoder_blocks.{2 * j}"
        wt = torch.from_numpy(np.ascontiguousarray(sd[pu + ".weight"]))
        bias = torch.from_numpy(np.ascontiguousarray(sd[pu + ".bias"]))
        cat, path = run_upconv(lib, cur, wt, bias, f, 0, ldo=2 * f, co_off=f, y=cats[l])
        paths.append((pu, path))
        ch *= 2
        cw *= 2
        pd = f"decoder_blocks.{2 * j + 1}"
        wt, sc, sh = fold_bn(sd, pd, 0, 1)
        cur, _, path = run_conv(lib, cat, wt, sc, sh, f, 1, 0)
        paths.append((f"{pd}.0", path))
        wt, sc, sh = fold_bn(sd, pd, 3, 4)
        if j == depth - 1:
            hw = torch.from_numpy(np.ascontiguousarray(sd["output.weight"].reshape(-1)))
            hb = float(sd["output.bias"][0])
            logits, _, _, path = run_head_conv(lib, cur, wt, sc, sh, f, 1, 0, hw, hb, 0.0)
            paths.append((f"{pd}.3+head", path))
            return logits
        cur, _, path = run_conv(lib, cur, wt, sc, sh, f, 1, 0)
        paths.append((f"{pd}.3", path))


@pytest.mark.parametrize("feats,n,h,w", [(list(S.DEFAULT_FEATURES), 2, 224, 224), ([64, 128], 3, 48, 56)])
def test_network_is_the_composition_of_the_operators(lib, feats, n, h, w):
    from unet_lane_detection_amd.model import UNetHIP
    sd = S.seeded_state_dict(feats, seed=4)
    m = UNetHIP(sd, device=0)
    frames = torch.from_numpy(S.synthetic_frames(n, h, w, seed=8)).cuda()
    try:
        for mode in (-1, 0, 1, 2):
            prev = lib.unet_set_bf16_persistent(mode)
            try:
                net = m.run_u8(frames, precision="bf16")
                paths = []
                got = chain_forward(lib, sd, feats, frames, paths)
            finally:
                lib.unet_set_bf16_persistent(prev)
            torch.cuda.synchronize()
            print(f"mode {mode}: " + ", ".join(f"{k} {NAMES[p[0]] if k != 'first' else p[0]}"
                                               f"{'+pool' if p[1] else ''}{'+head' if p[2] else ''}" for k, p in paths))
            assert all(p[0] != 0 for _, p in paths)
            assert torch.equal(got, net[:, 0]), f"mode {mode}: max |d| {(got - net[:, 0]).abs().max().item()}"
    finally:
        m.release()


def test_every_kernel_appears():
    """Coverage of section 1's kernels by the cases above (a static check of the case tables)."""
    assert any(k == IGEMM for *_, k in UPCONV_CASES) and any(k == WS for *_, k in UPCONV_CASES)
    assert any(k == R512 for *_, k in UPCONV_CASES)
    assert {k for *_, k, _ in HEAD_CASES} == {IGEMM, WS} and {f for *_, f in HEAD_CASES} == {0, 1}
    assert {k for *_, k in FIRST_CASES} == {1, 2}
    assert math.isfinite(float(ulp_bf16(torch.tensor([0.0], dtype=torch.float64))[0]))
