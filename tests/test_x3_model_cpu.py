"""f16x3 tier, no GPU: the bound of tests/x3_model.py discriminates.

A torch-CPU emulation of the kernels' arithmetic (x3_model.emulate_conv: fp16 split operands, three products, fp32
accumulation chunk by chunk and tap by tap, fp32 epilogue, rounded output split) must pass check() at K = 576, 2304 and
9216, with the operand edge values and the activation scales of tests/test_x3_ops_gpu.py, and every mutation a kernel or
a packer could plausibly carry must fail it.  This is where the bound's constants are held without a GPU."""
import math

import pytest
import torch

import x3_model as M

KS = [576, 2304, 9216]


def params(cin, cout, gen):
    w = (torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5).float()
    sign = torch.where(torch.rand(cout, generator=gen) < 0.25, -1.0, 1.0)
    scale = ((torch.rand(cout, generator=gen) + 0.5) * sign).float()
    shift = (torch.randn(cout, generator=gen) * 0.3).float()
    return w, scale, shift


def planes(shape, gen, scale=1.0):
    return M.split_f16(torch.randn(*shape, generator=gen) * scale)


def edge_planes(shape, gen):
    """the operand edge values of the GPU tests, built directly in the planes (see test_x3_ops_gpu.edge_planes)"""
    hi, lo = planes(shape, gen)
    c = shape[-1]
    hi[..., 0:4], lo[..., 0:4] = M.split_f16(torch.randn(*shape[:-1], 4, generator=gen) * 0.01)   # subnormal lo parts
    assert (lo[..., 0:4].float().abs() < 2.0 ** -14).all()
    lo[..., 4:8] = 0.0                                                                           # lo parts all zero
    hi[..., 8], lo[..., 8] = 0.0, 0.0                                                            # +0
    hi[..., 9], lo[..., 9] = -0.0, -0.0                                                          # -0
    hi[..., 10], lo[..., 10] = M.F16_MAX, 0.0
    hi[..., 11], lo[..., 11] = -M.F16_MAX, 0.0
    if c >= 64:
        hi[..., 32:64], lo[..., 32:64] = 0.0, 0.0                                                # a whole chunk of zeros
    return hi, lo


def act_scales(c, gen):
    """per-channel powers of two from 2^-12 .. 2^12, one channel at each clamp end (2^+-40), a dead channel at 1"""
    a = torch.ldexp(torch.ones(c), torch.randint(-12, 13, (c,), generator=gen).to(torch.int32))
    a[1], a[2], a[3] = 2.0 ** 40, 2.0 ** -40, 1.0
    return a


def scaled_case(cin, cout, gen):
    """planes hold T[c] * in_act[c] at the tier's working magnitude; channel 3 is dead (all zero, scale 1)"""
    ia, oa = act_scales(cin, gen), act_scales(cout, gen)
    hi, lo = planes((1, 6, 7, cin), gen, 200.0)
    hi[..., 3], lo[..., 3] = 0.0, 0.0
    w, scale, shift = params(cin, cout, gen)
    w = w * ia[None, :, None, None]          # the consumer's true weights are O(1) per unit of T
    scale = scale / oa                       # the producer's true output is O(200 / out_act)
    shift = shift * 100.0 / oa
    return hi, lo, w, scale, shift, ia, oa


def run(hi, lo, w, scale, shift, relu, label, ia=None, oa=None, ksplit=1, mut=None, quiet=False):
    m = M.model_conv(hi, lo, w, scale, shift, relu, ia, oa)
    gh, gl = M.emulate_conv(hi, lo, w, scale, shift, relu, ia, oa, ksplit=ksplit, mut=mut)
    ratio, acc = M.check(gh, gl, m["r"], m["s"], m["B"], label, quiet=quiet)
    return ratio, acc, m["dev"]


@pytest.mark.parametrize("K", KS)
def test_emulation_passes_and_constants_hold(K):
    cin = K // 9
    gen = torch.Generator().manual_seed(K)
    w, scale, shift = params(cin, 64, gen)
    hi, lo = planes((1, 8, 9, cin), gen)
    for relu in (0, 1):
        ratio, acc, dev = run(hi, lo, w, scale, shift, relu, f"K={K} relu={relu}")
        print(f"  three-product model vs true product: 2^{math.log2(dev):.1f} B")
        # fp32 accumulation: the worst element of a tensor stays within 4x the random-walk rms 2^-24 sqrt(K) B, below 2^-15 B
        assert acc <= 4 * 2.0 ** -24 * math.sqrt(K), (K, acc)
        # normal-lo inputs: the tier's "22 bits"
        assert dev < 2.0 ** -20, (K, dev)


@pytest.mark.parametrize("K", KS)
def test_edge_values_and_scales_pass(K):
    cin = K // 9
    gen = torch.Generator().manual_seed(100 + K)
    w, scale, shift = params(cin, 64, gen)
    hi, lo = edge_planes((1, 6, 7, cin), gen)
    scale_small = scale * 2.0 ** -6               # keeps the +-65504 channels' contributions inside the fp16 range
    _, _, dev = run(hi, lo, w, scale_small, shift, 0, f"K={K} edge values")
    print(f"  three-product model vs true product (subnormal lo parts present): 2^{math.log2(dev):.1f} B")
    hi, lo, w, scale, shift, ia, oa = scaled_case(cin, 64, gen)
    run(hi, lo, w, scale, shift, 1, f"K={K} activation scales", ia, oa)
    run(hi, lo, w, scale, shift, 0, f"K={K} split-K 4", ia, oa, ksplit=4)


def test_subnormal_lo_degrades_to_an_absolute_floor():
    """csrc/conv_x3_ws.h: fp32 inputs at 0.01 of the scale get subnormal lo parts (quantum 2^-24), so the planes no longer
    hold 22 bits of them: against the product of the fp32 values the planes were split from, the model leaves the 22-bit
    claim (about 2^-17 B) but the loss stays an absolute, bounded one; with normal lo parts it is below 2^-20 B"""
    gen = torch.Generator().manual_seed(7)
    w, scale, shift = params(256, 64, gen)
    for mag, lo_subnormal in ((1.0, False), (0.01, True)):
        x32 = torch.randn(1, 8, 9, 256, generator=gen) * mag
        hi, lo = M.split_f16(x32)
        assert bool((lo.float().abs() < 2.0 ** -14).all()) == lo_subnormal
        m = M.model_conv(hi, lo, w, scale, shift, 0)
        gh, gl = M.emulate_conv(hi, lo, w, scale, shift, 0)
        M.check(gh, gl, m["r"], m["s"], m["B"], f"inputs at {mag}")
        pre = M.fold(w, scale, shift)[4].double()
        src = M.conv3(x32.double(), w.double() * pre[:, None, None, None])
        dev = ((m["z"] - src).abs() / m["B"]).max().item()
        print(f"  three-product model vs the product of the fp32 source: 2^{math.log2(dev):.1f} B")
        assert (2.0 ** -20 < dev < 2.0 ** -15) if lo_subnormal else dev < 2.0 ** -20


MUTATIONS = [
    ("cross term x_hi w_lo dropped, all taps", dict(drop_xhwl="all")),
    ("cross term x_lo w_hi dropped, all taps", dict(drop_xlwh="all")),
    ("cross term x_hi w_lo dropped, one tap", dict(drop_xhwl=4)),
    ("cross term x_lo w_hi dropped, one tap", dict(drop_xlwh=7)),
    ("lo planes of two input channels swapped", dict(swap_lo=(5, 37))),
    ("weight pre-scale left out of s", dict(no_prescale=True)),
    ("output split truncated", dict(truncate=True)),
    ("one 32-channel chunk skipped", dict(skip_chunk=1)),
]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name,mut", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_fails_the_bound(K, name, mut):
    cin = K // 9
    gen = torch.Generator().manual_seed(K)
    w, scale, shift = params(cin, 64, gen)
    hi, lo = planes((1, 8, 9, cin), gen)
    run(hi, lo, w, scale, shift, 0, f"K={K} unmutated", quiet=True)
    with pytest.raises(AssertionError):
        run(hi, lo, w, scale, shift, 0, f"K={K} {name}", mut=mut)


@pytest.mark.parametrize("K", KS)
def test_in_act_on_the_wrong_axis_fails(K):
    cin = K // 9
    gen = torch.Generator().manual_seed(200 + K)
    hi, lo, w, scale, shift, ia, oa = scaled_case(cin, cin, gen)     # cin == cout: the wrong axis has the right length
    run(hi, lo, w, scale, shift, 0, f"K={K} scaled, unmutated", ia, oa, quiet=True)
    with pytest.raises(AssertionError):
        run(hi, lo, w, scale, shift, 0, f"K={K} in_act along cout", ia, oa, mut=dict(in_act_axis=0))


@pytest.mark.parametrize("ksplit", [2, 4, 8])
def test_dropped_split_k_slab_fails(ksplit):
    gen = torch.Generator().manual_seed(300 + ksplit)
    w, scale, shift = params(1024, 64, gen)
    hi, lo = planes((1, 5, 6, 1024), gen)
    run(hi, lo, w, scale, shift, 1, f"kSplit {ksplit}", ksplit=ksplit)
    with pytest.raises(AssertionError):
        run(hi, lo, w, scale, shift, 1, f"kSplit {ksplit}, last slab dropped", ksplit=ksplit, mut=dict(drop_slab=ksplit - 1))
