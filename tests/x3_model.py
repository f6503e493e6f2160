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

The training step (csrc/unet_train.inc) runs the same kernels through other doors, modelled in the second half of this file:

  weights, device packers:   w_hi = f16(w), w_lo = f16(w - w_hi), fp16 subnormals kept; no pre-scale, no activation scales;
                             input-gradient operator (mode 1): W_d[n][k][t] = w[k][n][8 - t]
  scaled operand:            k = 13 - exponent(max |g|) (clamped to +-100; 0 for a zero, subnormal or non-finite maximum),
                             planes = split_f16(g 2^k), the three products are multiplied by s = 2^-k
  fp32 output, per element:  |got - r| <= 2^-23 |r| + 2^-15 |s| B         (two fp32 roundings; no absolute floor)
  weight gradients:          dW = s sum_p (dz_hi x_hi + dz_hi x_lo + dz_lo x_hi), B over the pixel sum, the same bound
  bias gradient:             an fp32 column sum: 2^-24 (additions of the longest chain) sum |g|

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

def emulate_conv(xh, xl, w, scale, shift, relu, in_act=None, out_act=None, ksplit=1, mut=None, folded=None, f32_out=False):
    """The 3x3 convolution as the kernels compute it: fp16 operands, per 32-channel chunk and tap the three products
    x_hi w_hi, x_hi w_lo, x_lo w_hi added to an fp32 accumulator, fp32 scale / shift / ReLU, clamp, rounded split.
    ksplit > 1: the chunks are divided over ksplit partial sums that are added at the end (split-K).
    mut: None or one of the mutations of tests/test_x3_model_cpu.py.  -> (hi, lo) fp16 planes (N,H,W,cout)
    folded: (w_hi, w_lo, s, t) to use instead of the host steps (the training step's device-packed operators);
    f32_out: the fp32 epilogue - return acc * s + t as fp32, no clamp, no split"""
    mut = mut or {}
    xh, xl = xh.float(), xl.float()
    if mut.get("swap_lo"):
        a, b = mut["swap_lo"]
        xl = xl.clone()
        xl[..., [a, b]] = xl[..., [b, a]]
    if folded is not None:
        w_hi, w_lo, s, t = folded
        pre = torch.ones_like(s)
    else:
        w_hi, w_lo, s, t, pre = fold(w, scale, shift, in_act, out_act, in_act_axis=mut.get("in_act_axis"))
    if mut.get("no_prescale"):
        s = s * pre.double()
    w_hi, w_lo = w_hi.float(), w_lo.float()
    n, h, wd, cin = xh.shape
    cout = w_hi.shape[0]
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
    if f32_out:
        return v
    if relu:
        v = torch.relu(v)
    v = v.clamp(-F16_MAX, F16_MAX)
    if mut.get("truncate"):
        def trunc16(a):      # fp32 -> fp16 towards zero (the 13 low mantissa bits cut; exact for normal fp16 results)
            return (a.contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32).half()
        hi = trunc16(v)
        return hi, trunc16(v - hi.float())
    return split_f16(v)


# ---- the training step's operators ----------------------------------------------------------------------------------

def split_w(w):
    """the device packers' split (pack_x3_kernel, pack_upconv_*_x3_kernel): no pre-scale -> (w_hi, w_lo) float64"""
    hi, lo = split_f16(w)
    return hi.double(), lo.double()


def dgrad_operator(w):
    """forward weight (cout, cin, 3, 3) -> the input-gradient operator's (cin, cout, 3, 3): channels swapped, taps flipped"""
    return w.permute(1, 0, 2, 3).flip(2, 3)


def scale_exponent(g):
    """k of split_planes_scaled_kernel / space_to_depth_planes_kernel from max |g| (an fp32 tensor)"""
    m = g.float().abs().max()
    if not bool(torch.isfinite(m)) or m.item() < 2.0 ** -126:
        return 0
    _, e = torch.frexp(m)                  # m = f 2^e, f in [0.5, 1): exponent(m) = e - 1
    return max(-100, min(100, 13 - (int(e) - 1)))


def scaled_split(g):
    """-> (hi, lo, k): planes of g 2^k (exact scaling)"""
    k = scale_exponent(g)
    hi, lo = split_f16(torch.ldexp(g.float(), torch.tensor(k, dtype=torch.int32)))
    return hi, lo, k


def bound_f32(r, s, B, acc=ACC):
    return 2.0 ** -23 * r.abs() + acc * abs(s) * B


def check_f32(got, r, s, B, label, quiet=False):
    """got: the fp32 output; r, B float64 of its shape, s the power-of-two output scale -> (ratio, accumulation part in |s| B)"""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == r.shape, (label, got.dtype, tuple(got.shape), tuple(r.shape))
    assert torch.isfinite(got).all(), f"{label}: non-finite output elements"
    err = (got.double() - r).abs()
    sB = abs(s) * B
    bnd = bound_f32(r, s, B)
    ratio = (err / bnd.clamp_min(1e-300)).max().item() if bool((bnd > 0).any()) else 0.0
    acc_ratio = ((err - 2.0 ** -23 * r.abs()) / sB.clamp_min(1e-300)).max().item()
    if not quiet:
        print(f"{label}: max err/bound {ratio:.4f}, accumulation part {acc_ratio:.3e} |s|B "
              f"(2^{torch.log2(torch.tensor(max(acc_ratio, 1e-30))).item():.1f})")
    bad = err > bnd
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {i}: got "
                             f"{got[i].item()!r} want {r[i].item()!r} (bound {bnd[i].item():.3e})")
    return ratio, acc_ratio


def model_train_conv(xh, xl, w, mode, k=0, device="cpu"):
    """the training step's 3x3 convolution: planes (fp16 / float64, NHWC) of the operand (scaled by 2^k), w the forward
    layer's fp32 weight (cout, cin, 3, 3); mode 0: forward (planes have cin channels), mode 1: input gradient (planes
    have cout channels) -> dict(r, B, s) on the CPU"""
    xh, xl = xh.double().to(device), xl.double().to(device)
    w_hi, w_lo = (v.to(device) for v in split_w(dgrad_operator(w) if mode else w))
    z, B = three_products(xh, xl, w_hi, w_lo, conv3)
    s = 2.0 ** -k
    return dict(r=(z * s).cpu(), B=B.cpu(), s=s)


def emulate_train_conv(xh, xl, w, mode, k=0, mut=None):
    """fp32 emulation of the same (emulate_conv with the device packers' operands and the fp32 epilogue) -> fp32 (N,H,W,co)"""
    mut = dict(mut or {})
    wop = w
    if mode:
        # no_swap: the same memory indexed (co, ci) instead of (ci, co) - shapes still match for cin != cout
        wop = w.permute(1, 0, 2, 3) if not mut.get("no_swap") else w.reshape(w.shape[1], w.shape[0], 3, 3)
        if not mut.get("no_flip"):
            wop = wop.flip(2, 3)
    w_hi, w_lo = split_w(wop)
    s = 2.0 ** -k
    if mut.get("no_inv"):
        s = 1.0
    if mut.get("inv_twice"):
        s = s * s
    co = wop.shape[0]
    return emulate_conv(xh, xl, None, None, None, 0, mut=mut,
                        folded=(w_hi, w_lo, torch.full((co,), s, dtype=torch.float64), torch.zeros(co, dtype=torch.float64)),
                        f32_out=True)


def shifted3(x):
    """x (N,H,W,C) -> the 9 tap-shifted copies xs[t][n,y,x,c] = xpad[n, y + ky, x + kx, c], t = ky * 3 + kx"""
    n, h, w, c = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return [xp[:, ky:ky + h, kx:kx + w, :] for ky in range(3) for kx in range(3)]


def model_wgrad3(dzh, dzl, xh, xl, k=0, device="cpu"):
    """dW (cout, cin, 3, 3) = 2^-k sum_p (dz_hi x_hi + dz_hi x_lo + dz_lo x_hi) -> dict(r, B, s)"""
    dzh, dzl, xh, xl = (v.double().to(device) for v in (dzh, dzl, xh, xl))
    co, ci = dzh.shape[-1], xh.shape[-1]
    a_h, a_l, a_t = dzh.reshape(-1, co).t(), dzl.reshape(-1, co).t(), (dzh + dzl).reshape(-1, co).t()
    r, B = [], []
    for sh, sl in zip(shifted3(xh), shifted3(xl)):
        bh, bl = sh.reshape(-1, ci), sl.reshape(-1, ci)
        r.append(a_h @ (bh + bl) + a_l @ bh)
        B.append(((a_t * a_t) @ ((bh + bl) * (bh + bl))).sqrt())
    s = 2.0 ** -k
    return dict(r=(torch.stack(r, -1).reshape(co, ci, 3, 3) * s).cpu(), B=torch.stack(B, -1).reshape(co, ci, 3, 3).cpu(), s=s)


def wgrad_splits(tiles, steps):
    """csrc/unet_train.inc wgrad_x3_splits"""
    splits = (max(8, (512 + tiles - 1) // tiles) + 7) // 8 * 8
    return min(splits, max(8, steps // 8 // 8 * 8))


def emulate_wgrad3(dzh, dzl, xh, xl, k=0, mut=None):
    """the pixel-K twin of emulate_conv (csrc/wgrad_x3_ws.h): a K-step is 2 image rows x 16 columns (columns past the image
    edge zero-filled), the steps are divided over split-K blocks with fp32 accumulators (three products per step and tap),
    the splits are added in double, multiplied by 2^-k and rounded to fp32 (wgrad_reduce_kernel) -> fp32 (cout,cin,3,3)"""
    mut = mut or {}
    dzh, dzl, xh, xl = (v.float() for v in (dzh, dzl, xh, xl))
    n, h, w, co = dzh.shape
    ci = xh.shape[-1]
    strips = (w + 15) // 16
    wp = strips * 16

    def padw(v):        # columns up to the strip grid: zeros - or, mutated, what lies behind the row in memory
        if wp == w:
            return v
        if mut.get("ragged_strip_reads_on"):
            flat = torch.cat([v.reshape(-1, v.shape[-1]), torch.zeros(wp, v.shape[-1])])
            idx = (torch.arange(n * h)[:, None] * w + torch.arange(wp)[None, :]).reshape(-1)
            return flat[idx].reshape(n, h, wp, v.shape[-1])
        return F.pad(v, (0, 0, 0, wp - w))
    dh, dl = padw(dzh), padw(dzl)
    xsh = [padw(t) for t in shifted3(xh)]
    xsl = [padw(t) for t in shifted3(xl)]
    steps = [(i, y, sx) for i in range(n) for y in range(h // 2) for sx in range(strips)]
    splits = wgrad_splits((co // 64) * (ci // 64), len(steps))
    per = (len(steps) + splits - 1) // splits
    total = torch.zeros(9, co, ci, dtype=torch.float64)
    for sp in range(splits):
        acc = torch.zeros(9, co, ci, dtype=torch.float32)
        for si in range(sp * per, min(len(steps), (sp + 1) * per)):
            if mut.get("skip_step") == si:
                continue
            i, y, sx = steps[si]
            sl_ = (i, slice(2 * y, 2 * y + 2), slice(16 * sx, 16 * sx + 16))
            ah, al = dh[sl_].reshape(32, co).t(), dl[sl_].reshape(32, co).t()
            for t in range(9):
                bh, bl = xsh[t][sl_].reshape(32, ci), xsl[t][sl_].reshape(32, ci)
                if not mut.get("drop_cross") == t:
                    acc[t] = acc[t] + ah @ bl
                acc[t] = acc[t] + al @ bh
                acc[t] = acc[t] + ah @ bh
        total += acc.double()
    v = total.float() * (1.0 if mut.get("no_inv") else 2.0 ** -k)
    return v.permute(1, 2, 0).reshape(co, ci, 3, 3).contiguous()


def space_to_depth(g):
    """g (N,2h,2w,f) -> S (N,h,w,4f), S[n,y,x,(a*2+b)*f + co] = g[n,2y+a,2x+b,co]"""
    n, h2, w2, f = g.shape
    return g.reshape(n, h2 // 2, 2, w2 // 2, 2, f).permute(0, 1, 3, 2, 4, 5).reshape(n, h2 // 2, w2 // 2, 4 * f)


def colsum_chain(pixels, c):
    """additions on the longest fp32 path of colsum_partial_kernel + colsum_finalize_kernel (csrc/train_kernels.h) over
    `pixels` rows of `c` channels: a block is rows x cols threads (col_geom: cols = min(c / 4, 256) float4 columns, rows the
    largest power of two <= 256 / cols) and takes per = ceil(P / grid) pixels (grid = red_blocks(P) = min(1024, max(1, P /
    64))); a thread walks the pixels r, r + rows, ...: at most ceil(per / rows) additions (fewer in depth: it adds four at a
    time pairwise); block_reduce_store adds log2(rows) tree levels; the blocks' partial sums are added in double and
    rounded to fp32 once"""
    grid = min(1024, max(1, pixels // 64))
    per = (pixels + grid - 1) // grid
    cols = min(c // 4, 256)
    rows = 1
    while rows * 2 <= 256 // cols:
        rows *= 2
    return (per + rows - 1) // rows + rows.bit_length() - 1 + 1


def model_upconv_bwd(g, xh, xl, w, device="cpu"):
    """ConvTranspose2d(2f -> f, k2 s2) backward on the f16x3 kernels: g (N,2h,2w,f) fp32 gradient, xh / xl planes of the
    input (N,h,w,2f), w (2f, f, 2, 2) fp32 -> dict(k, inv, dW, dW_B, dIn, dIn_B, db, db_bound), r / B float64 on the CPU"""
    sh, sl, k = scaled_split(space_to_depth(g.float()))
    inv = 2.0 ** -k
    f = g.shape[-1]
    cin = 2 * f
    sh, sl, xh, xl = (v.double().to(device) for v in (sh, sl, xh, xl))
    a_h, a_l = sh.reshape(-1, 4 * f).t(), sl.reshape(-1, 4 * f).t()
    bh, bl = xh.reshape(-1, cin), xl.reshape(-1, cin)
    dw = (a_h @ (bh + bl) + a_l @ bh) * inv                                     # rows (ab, co), columns ci
    dw_B = (((a_h + a_l) ** 2) @ ((bh + bl) ** 2)).sqrt()

    def to_w(m):                                                                   # [(ab, co)][ci] -> (ci, co, 2, 2)
        return m.reshape(4, f, cin).permute(2, 1, 0).reshape(cin, f, 2, 2).cpu()
    w_hi, w_lo = (v.to(device) for v in split_w(w))

    def to_k(m):                                                                   # (ci, co, 2, 2) -> [(ab, co)][ci]
        return m.reshape(cin, f, 4).permute(2, 1, 0).reshape(4 * f, cin)
    wd_h, wd_l = to_k(w_hi), to_k(w_lo)
    s_h, s_l = sh.reshape(-1, 4 * f), sl.reshape(-1, 4 * f)
    din = (s_h @ (wd_h + wd_l) + s_l @ wd_h) * inv
    din_B = (((s_h + s_l) ** 2) @ ((wd_h + wd_l) ** 2)).sqrt()
    shape = tuple(xh.shape)
    gd = g.double().reshape(-1, f)
    return dict(k=k, inv=inv, dW=to_w(dw), dW_B=to_w(dw_B), dIn=din.reshape(shape).cpu(), dIn_B=din_B.reshape(shape).cpu(),
                db=gd.sum(0), db_bound=2.0 ** -24 * colsum_chain(gd.shape[0], f) * gd.abs().sum(0))


def emulate_upconv_bwd(g, xh, xl, w, mut=None):
    """fp32 emulation of the two GEMMs of the transposed convolution's backward: the weight gradient over 32-pixel K-steps
    (zero-filled past the last pixel) and split-K blocks, added in double and written through the mode-1 index of
    wgrad_reduce_kernel; the input gradient chunk by chunk (32 of the 4f rows) -> (dW (2f,f,2,2), dIn (N,h,w,2f)) fp32"""
    mut = mut or {}
    sh, sl, k = scaled_split(space_to_depth(g.float()))
    inv = 1.0 if mut.get("no_inv") else 2.0 ** -k
    f = g.shape[-1]
    cin = 2 * f
    P = sh.shape[0] * sh.shape[1] * sh.shape[2]
    a_h, a_l = sh.float().reshape(P, 4 * f), sl.float().reshape(P, 4 * f)
    b_h, b_l = xh.float().reshape(P, cin), xl.float().reshape(P, cin)
    steps = (P + 31) // 32
    splits = wgrad_splits((4 * f // 128) * (cin // 128), steps)
    per = (steps + splits - 1) // splits
    total = torch.zeros(4 * f, cin, dtype=torch.float64)
    for sp in range(splits):
        acc = torch.zeros(4 * f, cin, dtype=torch.float32)
        for st in range(sp * per, min(steps, (sp + 1) * per)):
            if mut.get("skip_step") == st:
                continue
            q = slice(32 * st, min(P, 32 * st + 32))
            acc = acc + a_h[q].t() @ b_l[q]
            acc = acc + a_l[q].t() @ b_h[q]
            acc = acc + a_h[q].t() @ b_h[q]
        total += acc.double()
    v = total.float() * inv
    dw = torch.empty(cin * f * 4, dtype=torch.float32)
    row = torch.arange(4 * f)
    if mut.get("ab_co_exchanged"):
        ab, co = row % 4, row // 4
    else:
        ab, co = row // f, row % f
    idx = (torch.arange(cin)[None, :] * f + co[:, None]) * 4 + ab[:, None]
    dw[idx.reshape(-1)] = v.reshape(-1)
    w_hi, w_lo = split_w(w)
    wd_h = w_hi.float().reshape(cin, f, 4).permute(2, 1, 0).reshape(4 * f, cin)
    wd_l = w_lo.float().reshape(cin, f, 4).permute(2, 1, 0).reshape(4 * f, cin)
    acc = torch.zeros(P, cin, dtype=torch.float32)
    for kc in range(4 * f // 32):
        q = slice(32 * kc, 32 * kc + 32)
        acc = acc + a_h[:, q] @ wd_l[q]
        acc = acc + a_l[:, q] @ wd_h[q]
        acc = acc + a_h[:, q] @ wd_h[q]
    return dw.reshape(cin, f, 2, 2), (acc * inv).reshape(tuple(xh.shape))


# ---- fused BatchNorm statistics: an integer-exact check ------------------------------------------------------------

def integer_case(n, h, w, cin, cout, gen):
    """x_hi integers in [-2, 2], x_lo = 0, weights in {-1, 0, 1}: every z is an integer and, while a channel's sum of z^2
    stays below 2^24 (asserted by stat_reference), every partial sum in any order is exact in fp32"""
    xh = torch.randint(-2, 3, (n, h, w, cin), generator=gen).half()
    wt = torch.randint(-1, 2, (cout, cin, 3, 3), generator=gen).float()
    return xh, torch.zeros_like(xh), wt


def stat_reference(z):
    """z (N,H,W,C) float64 integers -> (sum z, sum z^2) per channel; fails where the exactness argument does not hold"""
    assert torch.equal(z, z.round()), "z is not integer-valued"
    s1, s2 = z.sum(dim=(0, 1, 2)), (z * z).sum(dim=(0, 1, 2))
    assert s2.max().item() < 2.0 ** 24, f"a channel's sum of z^2 reaches {s2.max().item():.0f} >= 2^24: partial sums may round"
    return s1, s2


def check_stat_rows(rows, z, label):
    """rows (R, 2, C) fp32 partial rows [row][sum, sum of squares][channel] -> bit-exact agreement of their float64 sum"""
    s1, s2 = stat_reference(z)
    got = rows.detach().cpu().double().sum(0)
    assert torch.equal(got[0], s1), f"{label}: per-channel sum differs in {int((got[0] != s1).sum())} channels"
    assert torch.equal(got[1], s2), f"{label}: per-channel sum of squares differs in {int((got[1] != s2).sum())} channels"


def emulate_stat_rows(z, tile_h, tile_w, mut=None):
    """the epilogues' rows: one row per pixel tile, its pixels' z and z^2 added in fp32 (z float64 integers, NHWC)"""
    mut = mut or {}
    n, h, w, c = z.shape
    rows = []
    for i in range(n):
        for y0 in range(0, h, tile_h):
            for x0 in range(0, w, tile_w):
                t = z[i, y0:y0 + tile_h, x0:x0 + tile_w].reshape(-1, c).float()
                rows.append(torch.stack([t.sum(0), (t * t).sum(0)]))
    if mut.get("extra_pixel") is not None:      # a tile that ran over the image edge counted one out-of-image pixel
        e = mut["extra_pixel"].float()
        rows[-1] = rows[-1] + torch.stack([e, e * e])
    return torch.stack(rows)
