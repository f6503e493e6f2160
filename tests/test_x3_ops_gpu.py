"""f16x3 tier, one kernel at a time on the network's own paths, against the float64 model of tests/x3_model.py.

Every case builds its operand planes itself (exact fp16 hi / lo bit patterns), calls a plane-level entry point
(unet_op_*_x3_planes: the network's packing, dispatch and kernels), asserts through path_out that the path it names ran,
and holds EVERY output element to

    |got - r| <= 2^-21 |r| + 2^-24 + 2^-15 |s| B            (tests/x3_model.py; tests/test_x3_model_cpu.py shows on the
                                                             CPU that a faithful emulation passes it and what fails it)

Output planes are views into a larger allocation filled with an fp16 NaN pattern no kernel produces: one image row of
sentinels before and after each plane, plus the channels outside [co_off, co_off + cout).  Every element inside must be
written, every sentinel outside untouched.  Each case prints its path, max(err / bound) and the part of the error the
accumulation term covers in units of |s| B (profiles/r08/x3_ops.md keeps the measured values)."""
import ctypes as C
import functools
import math

import pytest
import torch

import x3_model as M
from x3_dispatch_queries import PATH, VALID, ask, conv_query, switches_from_env
from x3_gpu_helpers import (ERR_HIP, ERR_INVALID_ARG, R512, SENTINEL, T448, WS, Planes, _h, _p, path_str, seed_of,  # noqa: F401
                            to_dev)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    lib = _lib.load(build_if_missing=False)
    prev = lib.unet_set_x3_upconv_r512(-1)
    prev_q8 = lib.unet_set_x3_cross_fp8(0)
    yield lib
    lib.unet_set_x3_upconv_r512(prev)
    lib.unet_set_x3_cross_fp8(prev_q8)


def conv_params(cin, cout, gen):
    w = (torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5).float()
    sign = torch.where(torch.rand(cout, generator=gen) < 0.25, -1.0, 1.0)
    scale = ((torch.rand(cout, generator=gen) + 0.5) * sign).float()
    shift = (torch.randn(cout, generator=gen) * 0.3).float()
    return w.contiguous(), scale.contiguous(), shift.contiguous()


def upconv_params(cin, cout, gen):
    w = (torch.randn(cin, cout, 2, 2, generator=gen) * (1.0 / cin) ** 0.5).float()
    return w.contiguous(), (torch.randn(cout, generator=gen) * 0.3).float().contiguous()


def rand_planes(shape, gen, mag=1.0):
    return M.split_f16(torch.randn(*shape, generator=gen) * mag)


def edge_planes(shape, gen):
    """operand edge values, built directly in the planes: channels 0-3 subnormal lo parts, 4-7 lo parts all zero, 8 all +0,
    9 all -0, 10 / 11 hi = +-65504, 32-63 a whole chunk of zeros"""
    hi, lo = rand_planes(shape, gen)
    hi[..., 0:4], lo[..., 0:4] = M.split_f16(torch.randn(*shape[:-1], 4, generator=gen) * 0.01)
    assert (lo[..., 0:4].float().abs() < 2.0 ** -14).all()
    lo[..., 4:8] = 0.0
    hi[..., 8], lo[..., 8] = 0.0, 0.0
    hi[..., 9], lo[..., 9] = -0.0, -0.0
    hi[..., 10], lo[..., 10] = M.F16_MAX, 0.0
    hi[..., 11], lo[..., 11] = -M.F16_MAX, 0.0
    hi[..., 32:64], lo[..., 32:64] = 0.0, 0.0
    return hi, lo


def act_scales(c, gen):
    """per-channel powers of two from 2^-12 .. 2^12, one channel at each clamp end (2^+-40), a dead channel's 1"""
    a = torch.ldexp(torch.ones(c), torch.randint(-12, 13, (c,), generator=gen).to(torch.int32))
    a[1], a[2], a[3] = 2.0 ** 40, 2.0 ** -40, 1.0
    return a.contiguous()


# ---- the 3x3 convolution ------------------------------------------------------------------------------------------

def run_conv(lib, hi, lo, w, scale, shift, relu, tw, *, ldo=0, co_off=0, pool=False, split_k=0, in_act=None, out_act=None,
             head=None, thr=0.0, expect_rc=0):
    """-> dict(out Planes, pool Planes, logits / probs / mask, path, range)"""
    n, h, wd, cin = hi.shape
    cout = w.shape[0]
    x, xlo = to_dev(hi, lo)
    y = Planes(n, h, wd, ldo or cout) if head is None else None
    yp = Planes(n, h // 2, wd // 2, cout) if pool else None
    logits = probs = mask = None
    if head is not None:
        logits = torch.full((n, h, wd), float("nan"), device="cuda")
        probs = torch.full((n, h, wd), float("nan"), device="cuda")
        mask = torch.full((n, h, wd), 7, dtype=torch.uint8, device="cuda")
    path = (C.c_int * 8)()
    rng = C.c_int(-1)
    rc = lib.unet_op_conv3x3_x3_planes(
        0, _p(x), xlo, n, h, wd, cin, _h(w), _h(scale), _h(shift), cout, relu, tw, _h(in_act), _h(out_act), split_k,
        y.ptr if y else None, y.lo_off if y else 0, ldo, co_off, yp.ptr if yp else None, yp.lo_off if yp else 0,
        _h(head[0]) if head else None, head[1] if head else 0.0, thr, _p(logits), _p(probs), _p(mask), path, C.byref(rng), None)
    assert rc == expect_rc, (rc, tw, tuple(hi.shape), cout)
    torch.cuda.synchronize()
    if rc == 0:     # the host-side plan for the same query is what the launch reported
        plan, _ = ask(lib, "conv", conv_query(n, h, wd, cin, cout, 2 if head is not None else (1 if pool else 0), tile_width=tw,
                                              co_off=co_off, split=1 if split_k else 0, switches=switches_from_env()))
        assert plan[VALID] == 1 and tuple(plan[PATH]) == tuple(path)[:7], (plan, tuple(path))
    return dict(out=y, pool=yp, logits=logits, probs=probs, mask=mask, path=tuple(path)[:7], range=rng.value)


def pool_model(r):
    """MaxPool2d(2,2) of an NHWC float64 tensor"""
    n, h, w, c = r.shape
    return r.reshape(n, h // 2, 2, w // 2, 2, c).amax(dim=(2, 4))


def check_pool(yp, out_hi, out_lo, label, bitwise=False):
    """the pooled planes stand for exactly the max of the stored activation: the split is monotonic, so this holds for
    the fused epilogue, which pools the fp32 values before the split, and for the pooling pass, which pools hi + lo; and
    they are a rounded split.  bitwise (the pooling kernel on its own): they ARE the split of that max."""
    yp.assert_written_only(0, yp.shape[3], label + " pool")
    want = pool_model(M.merged(out_hi, out_lo))
    got_hi, got_lo = yp.halves()
    assert torch.equal(M.merged(got_hi, got_lo), want), f"{label}: pooled planes are not the max of the stored activation"
    assert (got_lo.double().abs() <= M.ulp_f16(got_hi) / 2).all(), f"{label}: pooled planes are not a rounded split"
    if bitwise:
        want_hi, want_lo = M.split_f16(want.float())
        assert torch.equal(got_hi.view(torch.int16), want_hi.view(torch.int16)), f"{label}: pooled hi plane differs"
        assert torch.equal(got_lo.view(torch.int16), want_lo.view(torch.int16)), f"{label}: pooled lo plane differs"


@functools.lru_cache(maxsize=4)
def conv_case(n, h, w, cin, cout, relu, seed, kind="randn"):
    """inputs and float64 model of a case, shared between the tests that run it through different paths"""
    gen = torch.Generator().manual_seed(seed)
    wt, scale, shift = conv_params(cin, cout, gen)
    ia = oa = None
    if kind == "edge":
        hi, lo = edge_planes((n, h, w, cin), gen)
        scale = (scale * 2.0 ** -6).contiguous()       # the +-65504 channels' terms stay inside the fp16 range
    elif kind == "scaled":
        ia, oa = act_scales(cin, gen), act_scales(cout, gen)
        hi, lo = rand_planes((n, h, w, cin), gen, 200.0)
        hi[..., 3], lo[..., 3] = 0.0, 0.0              # the dead channel
        wt = (wt * ia[None, :, None, None]).contiguous()     # the consumer's true weights are O(1) per unit of T
        scale = (scale / oa).contiguous()                    # the producer's true output is O(200 / out_act)
        shift = (shift * 100.0 / oa).contiguous()
    else:
        hi, lo = rand_planes((n, h, w, cin), gen)
    m = M.model_conv(hi, lo, wt, scale, shift, relu, ia, oa, device="cuda")
    return dict(hi=hi, lo=lo, w=wt, scale=scale, shift=shift, ia=ia, oa=oa, m=m, kind=kind)


def conv_and_check(lib, case, relu, tw, want_path, label, *, ldo_mode=0, pool=False, split_k=0):
    """ldo_mode 0: dense; 1: ldo = 2 cout, co_off 0; 2: ldo = 2 cout, co_off = cout"""
    cout = case["w"].shape[0]
    ldo, co_off = ((0, 0), (2 * cout, 0), (2 * cout, cout))[ldo_mode]
    res = run_conv(lib, case["hi"], case["lo"], case["w"], case["scale"], case["shift"], relu, tw, ldo=ldo, co_off=co_off,
                   pool=pool, split_k=split_k, in_act=case["ia"], out_act=case["oa"])
    label = f"{label} ldo_mode {ldo_mode} [{path_str(res['path'])}]"
    assert res["path"] == tuple(want_path), f"{label}: expected {path_str(want_path)}"
    m = case["m"]
    res["out"].assert_written_only(co_off, co_off + cout, label)
    gh, gl = res["out"].halves(co_off, co_off + cout)
    M.check(gh, gl, m["r"], m["s"], m["B"], label)
    print(f"  three-product model vs true product: 2^{math.log2(max(m['dev'], 1e-30)):.1f} B")
    if case["kind"] == "randn":
        assert m["dev"] < 2.0 ** -20, (label, m["dev"])
    assert res["range"] == 0, f"{label}: range reported for in-range values"
    if pool:
        check_pool(res["pool"], gh, gl, label)
    return res


# (id, n, h, w, cin, cout, forced tile width, pool, ldo modes, expected path (structure, tile width, epilogue, flat,
#  kSplit, waves, separate pooling pass)).  Shapes: the smallest that reach the path with ragged tiles and > 1 block.
WS_CASES = [
    ("ws32", 1, 9, 33, 64, 64, 32, False, (0, 1, 2), (WS, 32, 0, 0, 1, 0, 0)),
    ("ws32-flat-pool", 2, 6, 34, 64, 128, 32, True, (0, 1), (WS, 32, 1, 1, 1, 0, 0)),
    ("ws32-pool", 1, 10, 34, 128, 64, 32, True, (1, 2), (WS, 32, 1, 0, 1, 0, 0)),
    ("ws32-flat", 3, 5, 17, 64, 64, 32, False, (1, 2), (WS, 32, 0, 1, 1, 0, 0)),
    ("ws16-pool", 1, 18, 20, 128, 64, 16, True, (0, 1, 2), (WS, 16, 1, 0, 1, 0, 0)),
    ("ws16-flat", 3, 5, 17, 64, 192, 16, False, (0, 2), (WS, 16, 0, 1, 1, 0, 0)),
    ("ws16", 1, 17, 18, 192, 128, 16, False, (1,), (WS, 16, 0, 0, 1, 0, 0)),
    ("ws16-flat-pool", 2, 6, 18, 64, 64, 16, True, (1, 2), (WS, 16, 1, 1, 1, 0, 0)),
]
# second structure: every case with ldo = 2 cout and followed by the pooling pass (the structure has no fused pooling)
R512_CASES = [
    ("r28-w1", 1, 10, 28, 64, 256, 28, True, (1, 2), (R512, 28, 0, 0, 1, 1, 1)),
    ("r28-w1-flat", 2, 6, 28, 128, 256, 28, True, (1,), (R512, 28, 0, 1, 1, 1, 1)),
    ("r28-w2", 1, 10, 56, 64, 128, 28, True, (1, 2), (R512, 28, 0, 0, 1, 2, 1)),
    ("r228", 1, 10, 28, 64, 256, 228, True, (2,), (R512, 28, 0, 0, 1, 2, 1)),
    ("r228-flat", 2, 6, 28, 64, 256, 228, True, (1,), (R512, 28, 0, 1, 1, 2, 1)),
    ("r14-w1", 1, 6, 14, 64, 256, 14, True, (1,), (R512, 14, 0, 0, 1, 1, 1)),
    ("r14-w1-flat", 3, 10, 14, 64, 256, 14, True, (2,), (R512, 14, 0, 1, 1, 1, 1)),
    ("r214", 1, 18, 14, 128, 256, 214, True, (1,), (R512, 14, 0, 0, 1, 2, 1)),
    ("r214-flat", 3, 10, 14, 64, 128, 214, True, (2,), (R512, 14, 0, 1, 1, 2, 1)),
    ("r332", 1, 8, 32, 64, 256, 332, True, (1, 2), (R512, 32, 0, 0, 1, 1, 1)),
    ("r332-flat", 2, 8, 64, 64, 256, 332, True, (1,), (R512, 32, 0, 1, 1, 1, 1)),
    ("r316", 1, 6, 16, 64, 256, 316, True, (2,), (R512, 16, 0, 0, 1, 1, 1)),
    ("r316-flat", 2, 8, 32, 64, 256, 316, True, (1,), (R512, 16, 0, 1, 1, 1, 1)),
    ("r308", 1, 6, 8, 64, 256, 308, True, (1,), (R512, 8, 0, 0, 1, 1, 1)),
    ("r308-flat", 2, 16, 24, 64, 256, 308, True, (2,), (R512, 8, 0, 1, 1, 1, 1)),
    ("r532", 1, 8, 32, 64, 128, 532, True, (1, 2), (R512, 32, 0, 0, 1, 2, 1)),
    ("r532-flat", 2, 8, 32, 64, 256, 532, True, (1,), (R512, 32, 0, 1, 1, 2, 1)),
]
# third structure: 628 / 632 (16-row tiles; 64 or 128 channels per block), 728 (8-row tiles, 256 channels per block)
T448_CASES = [
    ("t628-c1", 1, 18, 28, 64, 64, 628, False, (0, 1), (T448, 28, 0, 0, 1, 1, 0)),
    ("t628-c1-pool", 2, 10, 56, 64, 64, 628, True, (1, 2), (T448, 28, 1, 0, 1, 1, 0)),
    ("t628-c2", 1, 18, 28, 128, 128, 628, False, (1,), (T448, 28, 0, 0, 1, 2, 0)),
    ("t628-c2-pool", 1, 18, 28, 64, 128, 628, True, (1, 2), (T448, 28, 1, 0, 1, 2, 0)),
    ("t632", 1, 18, 32, 64, 64, 632, False, (1, 2), (T448, 32, 0, 0, 1, 1, 0)),
    ("t632-pool", 2, 10, 64, 64, 128, 632, True, (0, 1), (T448, 32, 1, 0, 1, 1, 0)),
    ("t728", 1, 10, 28, 64, 256, 728, False, (1, 2), (T448, 28, 0, 0, 1, 4, 0)),
    ("t728-pool", 1, 10, 56, 64, 256, 728, True, (1,), (T448, 28, 1, 0, 1, 4, 0)),
    ("t728-flat", 2, 6, 28, 64, 256, 728, False, (1,), (T448, 28, 0, 1, 1, 4, 0)),
    ("t728-flat-pool", 3, 6, 28, 128, 256, 728, True, (1, 2), (T448, 28, 1, 1, 1, 4, 0)),
]
# split-K (tile_width 0, the forward's scratch): one frame; run_conv_x3's rule doubles kSplit while the work items stay
# <= 256, every item keeps >= 2 chunks and the chunk count divides: 14 x 14 -> 512 (8 channel tiles) gives kSplit
# chunks / 2, i.e. 2 / 4 / 8 / 16 for cin 128 / 256 / 512 / 1024 (path_out is what proves it)
SPLITK_CASES = [
    ("sk2", 1, 14, 14, 128, 512, 0, False, (0, 1), (WS, 16, 0, 0, 2, 0, 0)),
    ("sk4", 1, 14, 14, 256, 512, 0, False, (2,), (WS, 16, 0, 0, 4, 0, 0)),
    ("sk8", 1, 14, 14, 512, 512, 0, False, (1,), (WS, 16, 0, 0, 8, 0, 0)),
    ("sk16", 1, 14, 14, 1024, 512, 0, False, (0,), (WS, 16, 0, 0, 16, 0, 0)),
    # the encoder's second convolution for a single frame: pooled, into the concat buffer
    ("sk-enc-pool", 1, 28, 28, 512, 512, 0, True, (1,), (WS, 32, 0, 0, 8, 0, 1)),
    # pooled with a channel offset: the pooling pass must read the channels the finish kernel wrote (out + co_off)
    ("sk-pool-cooff", 1, 14, 14, 128, 512, 0, True, (2,), (WS, 16, 0, 0, 2, 0, 1)),
]
# model A's layers for one frame, 56 x 56 and below, as the forward dispatches them (tile_width 0, split-K scratch)
AUTO_CASES = [
    ("enc3.conv1", 1, 56, 56, 128, 256, 0, False, (0,), (WS, 32, 0, 0, 2, 0, 0)),
    ("enc3.conv2", 1, 56, 56, 256, 256, 0, True, (1,), (WS, 32, 0, 0, 4, 0, 1)),
    ("enc4.conv1", 1, 28, 28, 256, 512, 0, False, (0,), (WS, 32, 0, 0, 4, 0, 0)),
    ("enc4.conv2", 1, 28, 28, 512, 512, 0, True, (1,), (WS, 32, 0, 0, 8, 0, 1)),
    ("dec1.conv1", 1, 28, 28, 1024, 512, 0, False, (0,), (WS, 32, 0, 0, 8, 0, 0)),
    ("bott.conv1", 1, 14, 14, 512, 1024, 0, False, (0,), (WS, 16, 0, 0, 8, 0, 0)),
    ("bott.conv2", 1, 14, 14, 1024, 1024, 0, False, (0,), (WS, 16, 0, 0, 16, 0, 0)),
    ("dec2.conv1", 1, 56, 56, 512, 256, 0, False, (0,), (WS, 32, 0, 0, 4, 0, 0)),
]
# fused head (cout 64): first structure both tile widths (no flat instance: n > 1 stays per image), third structure
HEAD_CASES = [
    ("head-ws32", 2, 9, 33, 64, 32, (WS, 32, 2, 0, 1, 0, 0)),
    ("head-ws16", 1, 17, 18, 128, 16, (WS, 16, 2, 0, 1, 0, 0)),
    ("head-t628", 1, 18, 28, 64, 628, (T448, 28, 2, 0, 1, 1, 0)),
    ("head-t632", 2, 10, 32, 64, 632, (T448, 32, 2, 0, 1, 1, 0)),
]


def test_cases_cover_the_dispatch():
    """the tables above reach every structure x epilogue x flat / per-image x kSplit x {ldo = cout, ldo = 2 cout} the
    network can launch in this tier (each case then asserts its row's path through path_out)"""
    rows = WS_CASES + R512_CASES + T448_CASES + SPLITK_CASES + AUTO_CASES
    seen = {(r[9][0], r[9][1], r[9][2], r[9][3]) for r in rows} | {(r[6][0], r[6][1], 2, 0) for r in HEAD_CASES}
    for tw in (16, 32):
        for epi in (0, 1):
            for flat in (0, 1):
                assert (WS, tw, epi, flat) in seen, (tw, epi, flat)
        assert (WS, tw, 2, 0) in seen
    for tw in (28, 14, 32, 16, 8):
        for flat in (0, 1):
            assert (R512, tw, 0, flat) in seen, (tw, flat)
    for tw in (28, 14, 32):       # the two-wave forms
        for flat in (0, 1):
            assert any(r[9][:2] == (R512, tw) and r[9][3] == flat and r[9][5] == 2 for r in R512_CASES), (tw, flat)
    assert all(r[7] and 0 not in r[8] and r[9][6] == 1 for r in R512_CASES)      # ldo = 2 cout + the pooling pass
    for tw, epis in ((28, (0, 1, 2)), (32, (0, 1, 2))):
        for epi in epis:
            assert (T448, tw, epi, 0) in seen, (tw, epi)
    for waves in (1, 2, 4):
        for epi in (0, 1):
            assert any(r[9][5] == waves and r[9][2] == epi for r in T448_CASES), (waves, epi)
    assert (T448, 28, 0, 1) in seen and (T448, 28, 1, 1) in seen
    assert {r[9][4] for r in rows} >= {1, 2, 4, 8, 16}
    for st in (WS, R512, T448):
        modes = set().union(*[set(r[8]) for r in rows if r[9][0] == st])
        assert modes >= ({0, 1, 2} if st != R512 else {1, 2}), (st, modes)
    assert any(r[7] and 2 in r[8] and r[9][4] > 1 for r in SPLITK_CASES)         # split-K, pooled, co_off != 0


def _run_rows(lib, row, split_k, kind="randn", seed=0):
    name, n, h, w, cin, cout, tw, pool, modes, want = row
    case = conv_case(n, h, w, cin, cout, 1, seed_of(name, seed), kind)
    for mode in modes:
        conv_and_check(lib, case, 1, tw, want, name, ldo_mode=mode, pool=pool, split_k=split_k)


@pytest.mark.parametrize("row", WS_CASES, ids=[r[0] for r in WS_CASES])
def test_conv_first_structure(lib, row):
    _run_rows(lib, row, 0)


@pytest.mark.parametrize("row", R512_CASES, ids=[r[0] for r in R512_CASES])
def test_conv_second_structure(lib, row):
    _run_rows(lib, row, 0)


@pytest.mark.parametrize("row", T448_CASES, ids=[r[0] for r in T448_CASES])
def test_conv_third_structure(lib, row):
    _run_rows(lib, row, 0)


@pytest.mark.parametrize("row", SPLITK_CASES, ids=[r[0] for r in SPLITK_CASES])
def test_conv_split_k(lib, row):
    _run_rows(lib, row, 1)


@pytest.mark.parametrize("row", AUTO_CASES, ids=[r[0] for r in AUTO_CASES])
def test_conv_automatic_dispatch_single_frame(lib, row):
    _run_rows(lib, row, 1)


def test_conv_without_scratch_does_not_split(lib):
    """the same 14 x 14 layer without the split-K scratch (the plain operator entry points' call): one pass, kSplit 1"""
    name, n, h, w, cin, cout, tw, pool, modes, want = SPLITK_CASES[0]
    case = conv_case(n, h, w, cin, cout, 1, seed_of(name, 0), "randn")
    conv_and_check(lib, case, 1, 0, (WS, 16, 0, 0, 1, 0, 0), "14x14 without scratch", ldo_mode=1)


SCALED_ROWS = [WS_CASES[4], R512_CASES[0], T448_CASES[3], SPLITK_CASES[1]]


@pytest.mark.parametrize("row", SCALED_ROWS, ids=[r[0] for r in SCALED_ROWS])
def test_conv_activation_scales(lib, row):
    """in_act / out_act folded into the weights and into scale / shift by build_conv_x3; the bound holds in the scaled
    units the planes hold"""
    _run_rows(lib, row, 1 if row in SPLITK_CASES else 0, kind="scaled", seed=1)


EDGE_ROWS = [WS_CASES[0], WS_CASES[4], R512_CASES[0], T448_CASES[0], SPLITK_CASES[0]]


@pytest.mark.parametrize("row", EDGE_ROWS, ids=[r[0] for r in EDGE_ROWS])
def test_conv_operand_edge_values(lib, row):
    _run_rows(lib, row, 1 if row in SPLITK_CASES else 0, kind="edge", seed=2)


# ---- fused head and the head kernel -------------------------------------------------------------------------------

def check_head(logits, probs, mask, ref, allow, thr, label):
    """logits against the float64 reference within `allow`; mask and probs from the kernel's own logits"""
    z = logits.cpu().double()
    assert torch.isfinite(z).all(), f"{label}: logits not written"
    err = (z - ref).abs()
    print(f"{label}: logits max err/bound {(err / allow).max().item():.4f}")
    assert (err <= allow).all(), (label, (err / allow).max().item())
    assert torch.equal(mask.cpu(), ((logits.cpu() > torch.tensor(thr, dtype=torch.float32)).to(torch.uint8) * 255)), f"{label}: mask != (logit > {thr})"
    perr = (probs.cpu().double() - torch.sigmoid(z)).abs().max().item()
    print(f"  probs vs float64 sigmoid of the kernel's logits: {perr:.2e}")
    assert perr <= 1e-6, (label, perr)


@pytest.mark.parametrize("row", HEAD_CASES, ids=[r[0] for r in HEAD_CASES])
def test_conv_fused_head(lib, row):
    name, n, h, w, cin, tw, want = row
    case = conv_case(n, h, w, cin, 64, 1, seed_of(name))
    gen = torch.Generator().manual_seed(5)
    hw = (torch.randn(64, generator=gen) * 0.2).float().contiguous()
    hb = 0.11
    m = case["m"]
    ref = (m["r"] * hw.double()).sum(-1) + hb
    terms = torch.cat([m["r"] * hw.double(), torch.full_like(ref, hb)[..., None]], dim=-1)
    allow = (M.bound(m["r"], m["s"], m["B"]) * hw.double().abs()).sum(-1) + 2.0 ** -20 * terms.pow(2).sum(-1).sqrt()
    for thr in (0.0, 0.37, -0.37):
        res = run_conv(lib, case["hi"], case["lo"], case["w"], case["scale"], case["shift"], 1, tw, head=(hw, hb), thr=thr)
        label = f"{name} thr {thr} [{path_str(res['path'])}]"
        assert res["path"] == tuple(want), label
        assert res["range"] == 0
        check_head(res["logits"], res["probs"], res["mask"], ref, allow, thr, label)


def test_head_kernel(lib):
    gen = torch.Generator().manual_seed(11)
    n, h, w, c = 2, 9, 13, 64
    hi, lo = rand_planes((n, h, w, c), gen, 3.0)
    hw = (torch.randn(c, generator=gen) * 0.2).float().contiguous()
    hb = -0.07
    x, xlo = to_dev(hi, lo)
    terms = torch.cat([M.merged(hi, lo) * hw.double(), torch.full((n, h, w, 1), hb, dtype=torch.float64)], dim=-1)
    ref = terms.sum(-1)
    allow = 2.0 ** -20 * terms.pow(2).sum(-1).sqrt()
    for thr in (0.0, 0.37, -0.37):
        logits = torch.full((n, h, w), float("nan"), device="cuda")
        probs = torch.full((n, h, w), float("nan"), device="cuda")
        mask = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda")
        assert lib.unet_op_head1x1_x3_planes(0, _p(x), xlo, n, h, w, c, _h(hw), hb, thr, _p(logits), _p(probs), _p(mask),
                                             None) == 0
        check_head(logits, probs, mask, ref, allow, thr, f"head1x1_planes thr {thr}")


# ---- transposed convolution ---------------------------------------------------------------------------------------

def run_upconv(lib, hi, lo, w, bias, *, ldo=0, co_off=0, in_act=None, expect_rc=0):
    n, h, wd, cin = hi.shape
    cout = w.shape[1]
    x, xlo = to_dev(hi, lo)
    y = Planes(n, 2 * h, 2 * wd, ldo or cout)
    path = (C.c_int * 8)()
    rng = C.c_int(-1)
    rc = lib.unet_op_upconv2x2_x3_planes(0, _p(x), xlo, n, h, wd, cin, _h(w), _h(bias), cout, _h(in_act), y.ptr, y.lo_off, ldo,
                                         co_off, path, C.byref(rng), None)
    assert rc == expect_rc, (rc, tuple(hi.shape), cout)
    torch.cuda.synchronize()
    return dict(out=y, path=tuple(path)[:7], range=rng.value)


# (id, n, h, w, cin, cout, unet_set_x3_upconv_r512 mode, expected structure, expected items per (a,b) split)
UPCONV_CASES = [
    ("up-ws-absplit", 1, 7, 14, 64, 64, 0, WS, 4),          # 98 pixels: one ragged 128-pixel tile, four (a,b) items
    ("up-ws", 1, 33, 35, 64, 512, 0, WS, 1),                # 1155 pixels: ten tiles, the last ragged
    ("up-r512", 1, 7, 14, 128, 64, 1, R512, 1),             # 98 pixels: one ragged 224-pixel tile
    ("up-r512-2tiles", 2, 9, 14, 256, 128, 1, R512, 1),     # 252 pixels: a full and a ragged tile, two images
]


@pytest.mark.parametrize("row", UPCONV_CASES, ids=[r[0] for r in UPCONV_CASES])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "in_act"])
def test_upconv(lib, row, scaled):
    """both structures, into the upper channel half of a concat buffer (ldo = 2 cout, co_off = cout: the skip half's
    sentinels stay), w = 14 and ragged last tiles"""
    name, n, h, w, cin, cout, mode, want_st, want_ab = row
    gen = torch.Generator().manual_seed(seed_of(name))
    wt, bias = upconv_params(cin, cout, gen)
    ia = None
    hi, lo = rand_planes((n, h, w, cin), gen, 200.0 if scaled else 1.0)
    if scaled:
        ia = act_scales(cin, gen)
        hi[..., 3], lo[..., 3] = 0.0, 0.0
        wt = (wt * ia[:, None, None, None] / 200.0).contiguous()
    m = M.model_conv(hi, lo, wt, torch.ones(cout), bias, 0, ia, None, transposed=True, device="cuda")
    prev = lib.unet_set_x3_upconv_r512(mode)
    try:
        res = run_upconv(lib, hi, lo, wt, bias, ldo=2 * cout, co_off=cout, in_act=ia)
    finally:
        lib.unet_set_x3_upconv_r512(prev)
    label = f"{name}{' in_act' if scaled else ''} [{'ws' if res['path'][0] == WS else 'r512'} abSplit {res['path'][5]}]"
    assert res["path"][0] == want_st and res["path"][5] == want_ab, (label, res["path"])
    res["out"].assert_written_only(cout, 2 * cout, label)
    gh, gl = res["out"].halves(cout, 2 * cout)
    M.check(gh, gl, m["r"], m["s"], m["B"], label)
    if not scaled:
        assert m["dev"] < 2.0 ** -20
    assert res["range"] == 0


# ---- the first convolution ----------------------------------------------------------------------------------------

MEAN = torch.tensor([123.675, 116.28, 103.53])
STD = torch.tensor([58.395, 57.12, 57.375])


def run_first(lib, inp, is_u8, n, h, w, wt, scale, shift, relu, out_act=None, ldo=0):
    cout = wt.shape[0]
    y = Planes(n, h, w, ldo or cout)
    rng = C.c_int(-1)
    mean, std = MEAN.contiguous(), STD.contiguous()
    rc = lib.unet_op_conv_first_x3_planes(0, _p(inp), 1 if is_u8 else 0, n, h, w, _h(wt), _h(scale), _h(shift), cout, relu,
                                          _h(mean), _h(std), _h(out_act), y.ptr, y.lo_off, ldo, C.byref(rng), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y, rng.value


def first_case(n, h, w, cout, gen, scaled):
    """frames: random, random, all 0, all 255 -> the normalised fp32 tensor (zero padding applies to it), its planes as
    the kernel splits them, and the K = 27 model"""
    frames = torch.randint(0, 256, (n, h, w, 3), generator=gen, dtype=torch.uint8)
    frames[-2] = 0
    frames[-1] = 255
    x32 = (frames.float() - MEAN) / STD
    wt = (torch.randn(cout, 3, 3, 3, generator=gen) * (2.0 / 27) ** 0.5).float().contiguous()
    _, scale, shift = conv_params(64, cout, gen)
    oa = act_scales(cout, gen) if scaled else None
    if scaled:       # the layer's true output is O(1 / out_act): the planes hold O(1)
        scale, shift = (scale / oa).contiguous(), (shift / oa).contiguous()
    hi, lo = M.split_f16(x32)
    m = M.model_conv(hi, lo, wt, scale, shift, 1, None, oa)
    return frames, x32, wt, scale, shift, oa, m


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", [(4, 11, 37, 64, 0), (4, 8, 32, 128, 256), (4, 21, 70, 128, 0)],
                         ids=["11x37", "8x32-ldo256", "21x70"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "out_act"])
def test_conv_first(lib, u8, shape, scaled):
    """the entry point launches through run_first_x3 (csrc/unet_x3.inc), the function forward_x3 calls for the network's
    first layer: its argument fill, its u8 / fp32 switch and its profiler label are the ones under test here"""
    n, h, w, cout, ldo = shape
    gen = torch.Generator().manual_seed(h * 100 + w)
    frames, x32, wt, scale, shift, oa, m = first_case(n, h, w, cout, gen, scaled)
    inp = frames.cuda() if u8 else x32.permute(0, 3, 1, 2).contiguous().cuda()
    y, rng = run_first(lib, inp, u8, n, h, w, wt, scale, shift, 1, oa, ldo)
    label = f"conv_first {'u8' if u8 else 'f32'} {n}x{h}x{w} -> {cout}{' out_act' if scaled else ''}"
    y.assert_written_only(0, cout, label)
    gh, gl = y.halves(0, cout)
    M.check(gh, gl, m["r"], m["s"], m["B"], label)
    assert m["dev"] < 2.0 ** -20 and rng == 0


# ---- pooling and the plane split ----------------------------------------------------------------------------------

def test_maxpool_planes_kernel(lib):
    """exact: the stored planes are the split of the float64 max of the merged inputs; pixel stride ldi = 2 c, windows
    of negative values only"""
    gen = torch.Generator().manual_seed(13)
    n, h, w, c = 2, 6, 10, 66
    hi, lo = rand_planes((n, h, w, 2 * c), gen, 5.0)
    neg = M.split_f16(-torch.rand(n, h, w, 8, generator=gen) * 3.0 - 1e-3)
    hi[..., 0:8], lo[..., 0:8] = neg
    x, xlo = to_dev(hi, lo)
    y = Planes(n, h // 2, w // 2, c)
    assert lib.unet_op_maxpool2x2_x3_planes(0, _p(x), xlo, n, h, w, c, 2 * c, y.ptr, y.lo_off, None) == 0
    torch.cuda.synchronize()
    check_pool(y, hi[..., :c], lo[..., :c], "maxpool2x2_planes", bitwise=True)
    assert (M.merged(*y.halves())[..., 0:8] < 0).all()


def run_split(lib, x32):
    x = x32.contiguous().cuda()
    y = Planes(1, 1, 1, x.numel())
    rng = C.c_int(-1)
    assert lib.unet_op_split_planes_x3(0, _p(x), x.numel(), y.ptr, y.lo_off, C.byref(rng), None) == 0
    torch.cuda.synchronize()
    y.assert_written_only(0, x.numel(), "split_planes")
    hi, lo = y.halves()
    return hi.reshape(-1), lo.reshape(-1), rng.value


def test_split_planes_kernel(lib):
    """fp32 -> planes is bit-for-bit the rounded split (both conversions round to nearest even); the merge, checked on
    the host as float64 hi + lo, returns the value to 2^-21 |v| + 2^-24"""
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(70002, generator=gen) * torch.ldexp(torch.ones(70002), torch.randint(-30, 16, (70002,), generator=gen).to(torch.int32))
    x[:8] = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, 2.0 ** -25, 1e-40, -3e-39])
    x = x.clamp(-65504.0, 65504.0)
    hi, lo, rng = run_split(lib, x)
    want_hi, want_lo = M.split_f16(x)
    assert torch.equal(hi.view(torch.int16), want_hi.view(torch.int16)), "hi plane is not f16_rne(v)"
    assert torch.equal(lo.view(torch.int16), want_lo.view(torch.int16)), "lo plane is not f16_rne(v - hi)"
    err = (M.merged(hi, lo) - x.double()).abs()
    assert (err <= 2.0 ** -21 * x.double().abs() + 2.0 ** -24).all()
    assert rng == 0


# ---- the range watch, once per plane-writing epilogue -------------------------------------------------------------

def _range_pair(base, model_for, run, label):
    """base: the case's model at factor 1 (v = z s + t, ordinary finite inputs).  model_for(f) / run(f): the model and the
    kernel's (hi, lo, range flag) with the case's affine part multiplied by f.  With the single largest |v| brought to
    65504 * 1.002 the call must report the range and store exactly +-65504 there; at 65504 * 0.998 it must not report.
    Either way every element meets the bound against the clamped model."""
    vmax = base["v"].abs().max().item()
    for factor, want in ((1.002, 1), (0.998, 0)):
        f = M.F16_MAX * factor / vmax
        mf = model_for(f)
        hi, lo, rng = run(f)
        v = mf["v"]
        i = tuple((v.abs() == v.abs().max()).nonzero()[0].tolist())
        assert (v.abs().max().item() > M.F16_MAX) == bool(want), (label, factor)
        assert rng == want, f"{label}: largest |r| = 65504 * {factor}: range_out {rng}"
        if want:
            assert hi[i].item() == math.copysign(M.F16_MAX, v[i].item()) and lo[i].item() == 0.0, \
                f"{label}: the out-of-range element is not stored as +-65504"
        M.check(hi, lo, mf["r"], mf["s"], mf["B"], f"{label} x{factor}")


RANGE_CONV = [("ws", WS_CASES[0], 0), ("r512", R512_CASES[0], 0), ("t448", T448_CASES[0], 0), ("split-K finish", SPLITK_CASES[0], 1)]


@pytest.mark.parametrize("which", RANGE_CONV, ids=[r[0] for r in RANGE_CONV])
def test_range_watch_conv(lib, which):
    """every convolution structure's plane epilogue and the split-K finish.  The second and third structure used to store
    -inf / +inf here (their split_pk_f16_mix had no clamp) while reporting the range; they clamp now, as conv_x3_ws.h
    promises."""
    label, (name, n, h, w, cin, cout, tw, pool, modes, want), split_k = which
    case = conv_case(n, h, w, cin, cout, 0, seed_of(name, "range"))

    def scaled(f):
        return (case["scale"] * f).contiguous(), (case["shift"] * f).contiguous()

    def model_for(f):
        return M.model_conv(case["hi"], case["lo"], case["w"], *scaled(f), 0, device="cuda")

    def run(f):
        res = run_conv(lib, case["hi"], case["lo"], case["w"], *scaled(f), 0, tw, split_k=split_k)
        assert res["path"][0] == want[0] and res["path"][4] == want[4], res["path"]
        return (*res["out"].halves(), res["range"])
    _range_pair(case["m"], model_for, run, f"range watch {label}")


@pytest.mark.parametrize("mode", [0, 1], ids=["upconv ws", "upconv r512"])
def test_range_watch_upconv(lib, mode):
    """both transposed-convolution structures (upconv_x3_r512.h shares split_pk_f16_mix with the convolution's second
    structure and stored +inf before that split clamped)"""
    name, n, h, w, cin, cout, _, want_st, _ = UPCONV_CASES[0 if mode == 0 else 2]
    gen = torch.Generator().manual_seed(23 + mode)
    wt, bias = upconv_params(cin, cout, gen)
    hi, lo = rand_planes((n, h, w, cin), gen)
    ones = torch.ones(cout)
    m = M.model_conv(hi, lo, wt, ones, bias, 0, transposed=True)

    def scaled(f):     # the transposed convolution has no scale: the factor goes into the weights and the bias
        return (wt * f).contiguous(), (bias * f).contiguous()

    def model_for(f):
        wf, bf = scaled(f)
        return M.model_conv(hi, lo, wf, ones, bf, 0, transposed=True)

    def run(f):
        prev = lib.unet_set_x3_upconv_r512(mode)
        try:
            res = run_upconv(lib, hi, lo, *scaled(f))
        finally:
            lib.unet_set_x3_upconv_r512(prev)
        assert res["path"][0] == want_st
        return (*res["out"].halves(), res["range"])
    _range_pair(m, model_for, run, f"range watch upconv {'r512' if mode else 'ws'}")


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
def test_range_watch_first_conv(lib, u8):
    n, h, w, cout = 4, 11, 37, 64
    gen = torch.Generator().manual_seed(29)
    frames, x32, wt, scale, shift, _, _ = first_case(n, h, w, cout, gen, False)
    hi, lo = M.split_f16(x32)
    m = M.model_conv(hi, lo, wt, scale, shift, 0)
    inp = frames.cuda() if u8 else x32.permute(0, 3, 1, 2).contiguous().cuda()

    def scaled(f):
        return (scale * f).contiguous(), (shift * f).contiguous()

    def run(f):
        y, rng = run_first(lib, inp, u8, n, h, w, wt, *scaled(f), 0)
        return (*y.halves(), rng)
    _range_pair(m, lambda f: M.model_conv(hi, lo, wt, *scaled(f), 0), run, f"range watch first conv {'u8' if u8 else 'f32'}")


def test_range_watch_split_kernel(lib):
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(4098, generator=gen) * 1000.0
    for top, want in ((65504.0 * 1.002, 1), (-65504.0 * 1.002, 1), (65519.0, 1), (65504.0, 0), (65504.0 * 0.998, 0)):
        x[1234] = top
        hi, lo, rng = run_split(lib, x)
        assert rng == want, (top, rng)
        want_hi, want_lo = M.split_f16(x)
        assert torch.equal(hi.view(torch.int16), want_hi.view(torch.int16)) and torch.equal(lo.view(torch.int16), want_lo.view(torch.int16))
        if want:
            assert hi[1234].item() == math.copysign(65504.0, top) and lo[1234].item() == 0.0


# ---- argument checks ----------------------------------------------------------------------------------------------

def test_entry_point_rejects_what_it_cannot_run(lib):
    gen = torch.Generator().manual_seed(37)
    hi, lo = rand_planes((1, 8, 28, 64), gen)
    w, scale, shift = conv_params(64, 128, gen)
    run_conv(lib, hi, lo, w, scale, shift, 1, 428, expect_rc=ERR_INVALID_ARG)                 # the f16q8 tier is not this file's
    run_conv(lib, hi, lo, w, scale, shift, 1, 32, ldo=128, co_off=64, expect_rc=ERR_INVALID_ARG)   # co_off + cout > ldo
    run_conv(lib, hi, lo, w, scale, shift, 1, 332, expect_rc=ERR_HIP)                          # 7 x 32 tiles need W % 32 == 0
