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


# ---- the training step's operators (tests/test_train_x3_ops_gpu.py holds the kernels to the same functions) ----------

TRAIN_KS = [576, 1152, 2304]         # 9 cin of the GPU shapes (cin 64, 128, 256)
G_MAGS = [1.0, 3e-8]


def train_w(cout, cin, gen, std=0.05):
    return (torch.randn(cout, cin, 3, 3, generator=gen) * std).float()


def run_train(g, w, mode, label, mut=None, quiet=False, k=None):
    """g: fp32 operand (scaled path) -> (ratio, acc) of the emulation against the model"""
    hi, lo, kk = M.scaled_split(g)
    m = M.model_train_conv(hi, lo, w, mode, kk)
    got = M.emulate_train_conv(hi, lo, w, mode, kk, mut=mut)
    return M.check_f32(got, m["r"], m["s"], m["B"], label, quiet=quiet)


def test_scale_exponent_is_the_kernels():
    """k = 13 - exponent(max |g|): the maximum lands in [2^13, 2^14); 0 for zero / subnormal / non-finite; clamped"""
    for v, k in ((1.0, 13), (1.999, 13), (2.0, 12), (3e-8, 38), (2.0 ** -126, 100), (2.0 ** 120, -100), (0.0, 0),
                 (1e-40, 0), (float("inf"), 0), (float("nan"), 0), (65504.0, -2)):
        assert M.scale_exponent(torch.tensor([0.0, v])) == k, (v, M.scale_exponent(torch.tensor([0.0, v])), k)
    hi, lo, k = M.scaled_split(torch.tensor([3e-8, -1e-8]))
    assert 2.0 ** 13 <= hi.float().abs().max() < 2.0 ** 14


@pytest.mark.parametrize("K", TRAIN_KS)
@pytest.mark.parametrize("mode", [0, 1])
def test_train_conv_emulation_passes(K, mode):
    cin = K // 9
    gen = torch.Generator().manual_seed(400 + K + mode)
    for mag in G_MAGS:
        for std in (0.05, 1e-3):
            w = train_w(64, cin, gen, std) if mode == 0 else train_w(cin, 64, gen, std)
            g = torch.randn(1, 8, 9, cin, generator=gen) * mag
            ratio, acc = run_train(g, w, mode, f"K={K} mode {mode} g~{mag} w~{std}")
            assert ratio <= 0.5 and acc <= 4 * 2.0 ** -24 * math.sqrt(K), (K, ratio, acc)
    # an outlier 2^10 above the rest sets the scale (the rest sits 10 bits lower in the planes); and the all-zero operand
    g = torch.randn(1, 8, 9, cin, generator=gen) * 1e-6
    g[0, 3, 4, 5] = 1e-6 * 2.0 ** 10
    assert M.scaled_split(g)[0].float().abs().median() < 2.0 ** 4
    run_train(g, w, mode, f"K={K} mode {mode} outlier")
    z = torch.zeros(1, 8, 9, cin)
    hi, lo, k = M.scaled_split(z)
    assert k == 0 and not M.emulate_train_conv(hi, lo, w, mode, k).any()


TRAIN_MUTATIONS = [
    ("inv not applied", 1, dict(no_inv=True)),
    ("inv applied twice", 1, dict(inv_twice=True)),
    ("taps not flipped in mode 1", 1, dict(no_flip=True)),
    ("one cross term dropped in one tap (x_hi w_lo)", 0, dict(drop_xhwl=4)),
    ("one cross term dropped in one tap (x_lo w_hi)", 1, dict(drop_xlwh=7)),
]


@pytest.mark.parametrize("K", TRAIN_KS)
@pytest.mark.parametrize("name,mode,mut", TRAIN_MUTATIONS, ids=[m[0] for m in TRAIN_MUTATIONS])
def test_train_conv_mutation_fails(K, name, mode, mut):
    cin = K // 9
    gen = torch.Generator().manual_seed(500 + K)
    w = train_w(64, cin, gen) if mode == 0 else train_w(cin, 64, gen)
    g = torch.randn(1, 8, 9, cin, generator=gen) * 3e-8
    run_train(g, w, mode, f"K={K} unmutated", quiet=True)
    with pytest.raises(AssertionError):
        run_train(g, w, mode, f"K={K} {name}", mut=mut, quiet=True)


def test_colsum_chain_is_read_from_the_code():
    """the four transposed-convolution shapes of the GPU test: hi-res pixels, f channels -> the longest chain"""
    for (n, h, w, f), chain in (((2, 14, 14, 64), 10), ((1, 7, 12, 128), 13), ((3, 4, 4, 256), 19), ((1, 28, 28, 64), 9)):
        assert M.colsum_chain(n * 4 * h * w, f) == chain, (n, h, w, f, M.colsum_chain(n * 4 * h * w, f))


def test_channels_not_swapped_in_mode_1_fails():
    """cin != cout: the forward weight (cout, cin) = (64, 128); its input-gradient operator takes the 64-channel gradient to
    128 channels and reads w[(k * 128 + n) * 9 + 8 - t].  Unswapped, the packer indexes the same memory as
    w[(n * 64 + k) * 9 + 8 - t]: every shape still matches, every weight is a wrong one"""
    gen = torch.Generator().manual_seed(77)
    w = train_w(64, 128, gen)
    g = torch.randn(1, 6, 7, 64, generator=gen)
    run_train(g, w, 1, "mode 1, cin != cout", quiet=True)
    with pytest.raises(AssertionError):
        run_train(g, w, 1, "mode 1, cin != cout, channels not swapped", mut=dict(no_swap=True), quiet=True)


def test_prescaled_model_against_unprescaled_packer_fails():
    """the host packers pre-scale (a normal lo part for every weight), the device packers do not: with small weights the lo
    parts are fp16 subnormals (quantum 2^-24) and a model that pre-scales is a different function.  At weights ~ 1e-4 the
    lost bits are ~ 2^-12 of a weight, eight times the bound's 2^-15"""
    gen = torch.Generator().manual_seed(78)
    w = train_w(64, 64, gen, 1e-4)
    assert (M.split_f16(w)[1].float().abs() < 2.0 ** -14).all()
    hi, lo = M.split_f16(torch.randn(1, 8, 9, 64, generator=gen))
    got = M.emulate_train_conv(hi, lo, w, 0)
    m = M.model_train_conv(hi, lo, w, 0)
    M.check_f32(got, m["r"], m["s"], m["B"], "un-prescaled model", quiet=True)
    pm = M.model_conv(hi, lo, w, torch.ones(64), torch.zeros(64), 0)       # the inference tier's model: pre-scaled
    err = (got.double() - pm["v"]).abs()
    assert (err > M.bound_f32(pm["v"], 1.0, m["B"])).float().mean() > 0.5      # not a thin margin: most elements are outside
    with pytest.raises(AssertionError):
        M.check_f32(got, pm["v"], 1.0, m["B"], "pre-scaled model", quiet=True)


WGRAD_SHAPES = [(1, 8, 20, 64, 64), (2, 16, 40, 64, 128), (1, 28, 28, 64, 64)]


def wgrad_case(shape, mag, seed):
    n, h, w, cin, cout = shape
    gen = torch.Generator().manual_seed(seed)
    dzh, dzl, k = M.scaled_split(torch.randn(n, h, w, cout, generator=gen) * mag)
    xh, xl = M.split_f16(torch.randn(n, h, w, cin, generator=gen))
    return dzh, dzl, xh, xl, k


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=str)
def test_wgrad_emulation_passes(shape):
    for mag in G_MAGS:
        dzh, dzl, xh, xl, k = wgrad_case(shape, mag, 600)
        m = M.model_wgrad3(dzh, dzl, xh, xl, k)
        ratio, acc = M.check_f32(M.emulate_wgrad3(dzh, dzl, xh, xl, k), m["r"], m["s"], m["B"], f"wgrad {shape} dz~{mag}")
        assert ratio <= 0.5, (shape, ratio)


WGRAD_MUTATIONS = [
    ("one K-step of pixels dropped", dict(skip_step=3)),
    ("last ragged strip not zero-filled", dict(ragged_strip_reads_on=True)),
    ("inv not applied", dict(no_inv=True)),
    ("one cross term dropped in one tap", dict(drop_cross=4)),
]


@pytest.mark.parametrize("name,mut", WGRAD_MUTATIONS, ids=[m[0] for m in WGRAD_MUTATIONS])
def test_wgrad_mutation_fails(name, mut):
    dzh, dzl, xh, xl, k = wgrad_case(WGRAD_SHAPES[0], 3e-8, 601)       # width 20: a ragged second strip
    m = M.model_wgrad3(dzh, dzl, xh, xl, k)
    M.check_f32(M.emulate_wgrad3(dzh, dzl, xh, xl, k), m["r"], m["s"], m["B"], "unmutated", quiet=True)
    with pytest.raises(AssertionError):
        M.check_f32(M.emulate_wgrad3(dzh, dzl, xh, xl, k, mut=mut), m["r"], m["s"], m["B"], name, quiet=True)


UPBWD_SHAPES = [(2, 14, 14, 64), (1, 7, 12, 128), (3, 4, 4, 256), (1, 28, 28, 64)]


def upbwd_case(shape, mag, seed):
    n, h, w, f = shape
    gen = torch.Generator().manual_seed(seed)
    g = (torch.randn(n, 2 * h, 2 * w, f, generator=gen) * mag).float()
    xh, xl = M.split_f16(torch.randn(n, h, w, 2 * f, generator=gen).abs())
    wt = (torch.randn(2 * f, f, 2, 2, generator=gen) * (1.0 / (2 * f)) ** 0.5).float()
    return g, xh, xl, wt


@pytest.mark.parametrize("shape", UPBWD_SHAPES, ids=str)
def test_upconv_bwd_emulation_passes(shape):
    for mag in G_MAGS:
        g, xh, xl, wt = upbwd_case(shape, mag, 700)
        m = M.model_upconv_bwd(g, xh, xl, wt)
        assert m["inv"] == 2.0 ** -m["k"] and 2.0 ** 13 <= g.abs().max().item() / m["inv"] < 2.0 ** 14
        dw, din = M.emulate_upconv_bwd(g, xh, xl, wt)
        r1, _ = M.check_f32(dw, m["dW"], m["inv"], m["dW_B"], f"upconv bwd {shape} g~{mag} dW")
        r2, _ = M.check_f32(din, m["dIn"], m["inv"], m["dIn_B"], f"upconv bwd {shape} g~{mag} dIn")
        assert max(r1, r2) <= 0.5
        db32 = g.reshape(-1, shape[3]).sum(0)                                     # an fp32 column sum in some order
        assert ((db32.double() - m["db"]).abs() <= m["db_bound"]).all()


UPBWD_MUTATIONS = [
    ("ab and co exchanged in the mode-1 reduction index", dict(ab_co_exchanged=True)),
    ("one K-step of pixels dropped", dict(skip_step=1)),
    ("inv not applied", dict(no_inv=True)),
]


@pytest.mark.parametrize("name,mut", UPBWD_MUTATIONS, ids=[m[0] for m in UPBWD_MUTATIONS])
def test_upconv_bwd_mutation_fails(name, mut):
    g, xh, xl, wt = upbwd_case(UPBWD_SHAPES[1], 3e-8, 701)
    m = M.model_upconv_bwd(g, xh, xl, wt)
    dw, din = M.emulate_upconv_bwd(g, xh, xl, wt, mut=mut)
    with pytest.raises(AssertionError):
        M.check_f32(dw, m["dW"], m["inv"], m["dW_B"], name + " dW", quiet=True)
        M.check_f32(din, m["dIn"], m["inv"], m["dIn_B"], name + " dIn", quiet=True)
        raise RuntimeError("neither output left the bound")


def test_integer_statistics_are_exact_and_see_one_extra_pixel():
    """the fused BatchNorm statistics' check: integer z, every fp32 partial sum exact, the rows' float64 sum bit-exact; a row
    that counts one out-of-image pixel (the convolution's value one row below the image) fails it"""
    gen = torch.Generator().manual_seed(79)
    xh, xl, wt = M.integer_case(2, 28, 28, 64, 128, gen)
    z = M.model_train_conv(xh, xl, wt, 0)["r"]
    s1, s2 = M.stat_reference(z)
    print(f"  mean z^2 {float((z * z).mean()):.0f}, largest channel sum of z^2 {float(s2.max()):.0f}")
    for th, tw in ((8, 28), (16, 28), (16, 14)):          # ragged tile grids included (28 = 16 + 12)
        M.check_stat_rows(M.emulate_stat_rows(z, th, tw), z, f"tiles {th}x{tw}")
    below = M.conv3(torch.nn.functional.pad(xh.double(), (0, 0, 0, 0, 0, 1)), M.split_w(wt)[0])[1, 28, 27]
    assert below.abs().sum() > 0
    with pytest.raises(AssertionError):
        M.check_stat_rows(M.emulate_stat_rows(z, 8, 28, mut=dict(extra_pixel=below)), z, "one out-of-image pixel")
    with pytest.raises(AssertionError):                   # the exactness condition is asserted, not assumed
        M.stat_reference(z * 8)
