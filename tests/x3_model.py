"""Float64 model of the split-operand (f16x3) tier's arithmetic, shared by tests/test_x3_model_cpu.py (which proves on
the CPU that the bound below passes a faithful emulation and fails every listed mutation) and tests/test_x3_ops_gpu.py
(which holds every kernel of the tier to it).  Restated from csrc/conv_x3_ws.h and build_conv_x3 (csrc/unet_x3.inc):

  operand planes are exact:  x~ = x_hi + x_lo, read from the planes the test built
  weights, host steps:       w' = w / in_act[ci]; pre[co] = the power of two taking max |w'| into [512, 1024);
                             w_hi = f16(w' pre), w_lo = f16(w' pre - w_hi)   (round to nearest even, as torch's .half())
  z = conv(x_hi, w_hi) + conv(x_hi, w_lo) + conv(x_lo, w_hi)                  (w_lo x_lo is left out, as in the kernels)
  B = sqrt(conv(x~^2, w~^2)),  s = scale / pre * out_act,  t = shift * out_act  (exact in fp32)
  r = relu?(z s + t) clamped to +-65504; the output is hi + lo of the stored planes

  bound, every element:      |got - r| <= 2^-21 |r| + 2^-24 + 2^-15 |s| B

The first two terms are the output split (22 bits while lo is normal, an absolute 2^-25 once it is subnormal, a factor
2 on each); the third is fp32 accumulation: a random walk over K <= 9 * 1024 terms gives 2^-24 sqrt(K) B <= 2^-17.4 B, the
emulation below measures 2^-19.5 B .. 2^-20 B, while one dropped cross term moves the result by a median 2^-12.8 B.

The magnitude bound cannot see a split that truncates instead of rounding (two truncations err by < 2^-21 |r|, inside
the first term), so check() also asserts the form a rounded split has: |lo| <= ulp_f16(hi) / 2 for every element (hi is
the nearest fp16 and lo what is left; a truncated hi leaves a lo of up to a whole ulp on about half of the elements).

All tensors are NHWC; planes are torch.float16, models float64."""
import torch
import torch.nn.functional as F

F16_MAX = 65504.0
ACC = 2.0 ** -15          # the accumulation term's constant (see above; never fitted to a kernel)


def split_f16(v):
    """fp32 -> (hi, lo) fp16 planes as split_pk_f16 on the device: clamp, hi = rn(v), lo = rn(v - hi)"""
    v = v.float().clamp(-F16_MAX, F16_MAX)
    hi = v.half()
    return hi, (v - hi.float()).half()


def merged(hi, lo):
    return hi.double() + lo.double()


def prescale_pow2(maxabs):
    """csrc/unet_x3.inc prescale_pow2, elementwise on an fp32 tensor"""
    _, e = torch.frexp(maxabs)
    p = torch.ldexp(torch.ones_like(maxabs), 10 - e)
    return torch.where((maxabs > 0) & torch.isfinite(maxabs), p, torch.ones_like(maxabs))


def fold(w, scale, shift, in_act=None, out_act=None, transposed=False, in_act_axis=None):
    """The host steps of build_conv_x3 (w (co,ci,3,3)) / build_upconv_x3 (transposed: w (ci,co,2,2)) ->
    w_hi, w_lo (float64, w's layout, pre-scaled units), s, t (float64 per output channel), pre"""
    w = w.float()
    ci_ax, co_ax = (0, 1) if transposed else (1, 0)
    if in_act_axis is not None:     # mutation hook of the CPU model test: divide along the wrong axis
        ci_ax_div = in_act_axis
    else:
        ci_ax_div = ci_ax

    def along(v, ax):
        shape = [1] * w.dim()
        shape[ax] = -1
        return v.view(shape)
    if in_act is not None:
        w = w * along(1.0 / in_act.float(), ci_ax_div)
    pre = prescale_pow2(w.abs().amax(dim=[d for d in range(w.dim()) if d != co_ax]))
    wp = w * along(pre, co_ax)
    w_hi = wp.half()
    w_lo = (wp - w_hi.float()).half()
    o = out_act.float() if out_act is not None else torch.ones_like(pre)
    s = scale.float() / pre * o
    t = shift.float() * o
    return w_hi.double(), w_lo.double(), s.double(), t.double(), pre


def im2col3(x):
    """x (N,H,W,C) -> (N,H,W,9C), tap-major (k = (ky*3 + kx) * C + ci), zero padding 1"""
    n, h, w, c = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return torch.cat([xp[:, ky:ky + h, kx:kx + w, :] for ky in range(3) for kx in range(3)], dim=-1)


def wmat3(w):
    """w (co,ci,3,3) -> (9 ci, co) in im2col3's order"""
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0])


def conv3(x, w):
    return im2col3(x) @ wmat3(w)


def upconv2(x, w):
    """ConvTranspose2d k2 s2 without bias: x (N,H,W,ci), w (ci,co,2,2) -> (N,2H,2W,co)"""
    n, h, wd, ci = x.shape
    co = w.shape[1]
    y = (x.reshape(-1, ci) @ w.reshape(ci, co * 4)).reshape(n, h, wd, co, 2, 2)
    return y.permute(0, 1, 4, 2, 5, 3).reshape(n, 2 * h, 2 * wd, co)


def three_products(xh, xl, w_hi, w_lo, op):
    """z, B of the module docstring; xh / xl float64 planes, op = conv3 or upconv2"""
    z = op(xh, w_hi + w_lo) + op(xl, w_hi)        # x_hi w_hi + x_hi w_lo + x_lo w_hi (float64: the sum order is immaterial)
    xt, wt = xh + xl, w_hi + w_lo
    return z, op(xt * xt, wt * wt).sqrt()


def epilogue(z, s, t, relu):
    r = z * s + t
    if relu:
        r = torch.relu(r)
    return r.clamp(-F16_MAX, F16_MAX)


def model_conv(xh, xl, w, scale, shift, relu, in_act=None, out_act=None, transposed=False, device="cpu"):
    """planes (fp16 or float64, NHWC) + fp32 host parameters -> dict(r, v, z, B, s, t, dev) on the CPU: v = z s + t before
    ReLU and clamp; dev = |z - conv(x~, w')| / B, the distance of the three-product model from the true product
    (reported; asserted < 2^-20 for normal-lo inputs only).  device: where the float64 products are formed"""
    xh, xl = xh.double().to(device), xl.double().to(device)
    w_hi, w_lo, s, t, pre = (v.to(device) for v in fold(w, scale, shift, in_act, out_act, transposed))
    op = upconv2 if transposed else conv3
    z, B = three_products(xh, xl, w_hi, w_lo, op)
    wd = w.double().to(device)
    if in_act is not None:
        in_act = in_act.to(device)
        shape = [-1, 1, 1, 1] if transposed else [1, -1, 1, 1]
        wd = wd / in_act.double().view(shape)
    wd = wd * (pre.double().view([1, -1, 1, 1] if transposed else [-1, 1, 1, 1]))
    ztrue = op(xh + xl, wd)
    dev = ((z - ztrue).abs() / B.clamp_min(1e-300)).max().item()
    return dict(r=epilogue(z, s, t, relu).cpu(), v=(z * s + t).cpu(), z=z.cpu(), B=B.cpu(), s=s.cpu(), t=t.cpu(), dev=dev)


def ulp_f16(hi):
    """one fp16 ulp at |hi| (11 significant bits; 2^-24 for subnormals and zero), float64"""
    a = hi.double().abs().clamp_min(2.0 ** -14)
    _, e = torch.frexp(a)
    return torch.ldexp(torch.ones_like(a), (e - 11).to(torch.int32))


def bound(r, s, B, acc=ACC):
    return 2.0 ** -21 * r.abs() + 2.0 ** -24 + acc * s.abs() * B


def check(hi, lo, r, s, B, label, extra=None, quiet=False):
    """hi / lo: the stored fp16 planes (N,H,W,C) of the channels under test; r, B (N,H,W,C) float64, s (C,).  `extra`:
    an additional float64 allowance per element (the head's dot product).  Prints max(err / bound) and the part of the
    error the accumulation term has to cover in units of |s| B, then asserts every element.  -> (ratio, acc_ratio)"""
    hi, lo = hi.cpu(), lo.cpu()
    assert torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all(), f"{label}: non-finite plane elements"
    got = merged(hi, lo)
    err = (got - r).abs()
    sB = s.abs() * B
    bnd = bound(r, s, B) + (extra if extra is not None else 0.0)
    ratio = (err / bnd).max().item()
    rest = (err - 2.0 ** -21 * r.abs() - 2.0 ** -24 - (extra if extra is not None else 0.0))
    acc_ratio = (rest / sB.clamp_min(1e-300)).max().item()
    form = (lo.double().abs() / ulp_f16(hi)).max().item()
    if not quiet:
        print(f"{label}: max err/bound {ratio:.4f}, accumulation part {acc_ratio:.3e} |s|B "
              f"(2^{torch.log2(torch.tensor(max(acc_ratio, 1e-30))).item():.1f}), |lo|/ulp(hi) {form:.3f}")
    bad = err > bnd
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {i}: got "
                             f"{got[i].item()!r} want {r[i].item()!r} (bound {bnd[i].item():.3e})")
    if form > 0.5:
        raise AssertionError(f"{label}: not a rounded split: |lo| reaches {form:.3f} ulp of hi")
    return ratio, acc_ratio


# ---- fp32 emulation of the kernels' arithmetic (CPU): chunk by chunk, tap by tap, three products each ----------------

def emulate_conv(xh, xl, w, scale, shift, relu, in_act=None, out_act=None, ksplit=1, mut=None):
    """The 3x3 convolution as the kernels compute it: fp16 operands, per 32-channel chunk and tap the three products
    x_hi w_hi, x_hi w_lo, x_lo w_hi added to an fp32 accumulator, fp32 scale / shift / ReLU, clamp, rounded split.
    ksplit > 1: the chunks are divided over ksplit partial sums that are added at the end (split-K).
    mut: None or one of the mutations of tests/test_x3_model_cpu.py.  -> (hi, lo) fp16 planes (N,H,W,cout)"""
    mut = mut or {}
    xh, xl = xh.float(), xl.float()
    if mut.get("swap_lo"):
        a, b = mut["swap_lo"]
        xl = xl.clone()
        xl[..., [a, b]] = xl[..., [b, a]]
    w_hi, w_lo, s, t, pre = fold(w, scale, shift, in_act, out_act, in_act_axis=mut.get("in_act_axis"))
    if mut.get("no_prescale"):
        s = s * pre.double()
    w_hi, w_lo = w_hi.float(), w_lo.float()
    n, h, wd, cin = xh.shape
    cout = w.shape[0]
    xhp, xlp = F.pad(xh, (0, 0, 1, 1, 1, 1)), F.pad(xl, (0, 0, 1, 1, 1, 1))
    nch = cin // 32
    parts = []
    for ks in range(ksplit):
        acc = torch.zeros(n, h, wd, cout, dtype=torch.float32)
        for kc in range(ks * nch // ksplit, (ks + 1) * nch // ksplit):
            if mut.get("skip_chunk") == kc:
                continue
            c0, c1 = kc * 32, kc * 32 + 32
            for ky in range(3):
                for kx in range(3):
                    ah = xhp[:, ky:ky + h, kx:kx + wd, c0:c1]
                    al = xlp[:, ky:ky + h, kx:kx + wd, c0:c1]
                    bh = w_hi[:, c0:c1, ky, kx].t()
                    bl = w_lo[:, c0:c1, ky, kx].t()
                    tap = ky * 3 + kx
                    if not (mut.get("drop_xhwl") == "all" or mut.get("drop_xhwl") == tap):
                        acc = acc + ah @ bl
                    if not (mut.get("drop_xlwh") == "all" or mut.get("drop_xlwh") == tap):
                        acc = acc + al @ bh
                    acc = acc + ah @ bh
        parts.append(acc)
    if mut.get("drop_slab") is not None:
        parts.pop(mut["drop_slab"])
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    v = acc * s.float() + t.float()
    if relu:
        v = torch.relu(v)
    v = v.clamp(-F16_MAX, F16_MAX)
    if mut.get("truncate"):
        def trunc16(a):      # fp32 -> fp16 towards zero (the 13 low mantissa bits cut; exact for normal fp16 results)
            return (a.contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32).half()
        hi = trunc16(v)
        return hi, trunc16(v - hi.float())
    return split_f16(v)
