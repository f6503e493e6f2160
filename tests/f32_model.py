"""Float64 model of the exact-fp32 tier's operators (csrc/igemm_f32.h, csrc/wino_f32.h, csrc/elementwise.h), the bound
tests/test_f32_ops_gpu.py holds the kernels to, and two fp32 emulations of the kernels' own arithmetic order that
tests/test_f32_model_cpu.py uses to size that bound.  Nothing here touches the library: the emulations are plain numpy.

The bound, per output element, with r the float64 result from the fp32 inputs held exactly:

    |got - r| <= C_ULP * ulp32(|r|) + C_ACC * 2^-24 * sqrt(K) * |scale| * B

K: terms per output (9 Cin for the 3x3 convolution, Cin for the transposed and the plain 1x1 convolution),
B = sqrt(conv(x^2, w^2)): the root of the sum of the squared terms, so 2^-24 sqrt(K) B is the size a random walk of K
roundings of partial sums of that magnitude reaches.  One dropped term has the size |scale| B / sqrt(K) on average, which
C_ACC * 2^-24 * K <= 1/64 keeps at least 64 bounds away (asserted in test_f32_model_cpu.py at the largest K tested).

C_ACC and C_ULP are 4 x the worst ratios the two emulations reach over the case table below (measured on the CPU by
test_f32_model_cpu.py::test_emulations_inside_a_quarter_of_the_bound, which prints them):
    accumulators, every case:  |acc_emulated - z| / (2^-24 sqrt(K) B)  <= 2.57  (direct order; Winograd order 1.64)
                               -> C_ACC = 10.5
    outputs, the small-K cases (K <= 144), on the elements where the ulp term is the larger of the two
    (ulp32(|r|) >= 2^-24 sqrt(K) |scale| B):  |out_emulated - r| / ulp32(|r|)  <= 1.81  -> C_ULP = 7.5
The margin of 4 covers what an emulation cannot know: the order in which one MFMA adds its four products.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

C_ACC = 10.5
C_ULP = 7.5
U24 = 2.0 ** -24

Case = collections.namedtuple("Case", "name kind n cin cout h w algo relu family slices pool want")
# kind: "conv" 3x3 | "up" transposed 2x2 | "c1" plain 1x1;  algo: 1 direct, 2 Winograd (conv only)
# family: input family (make_inputs);  slices: the (ldo, co_off) runs beside the dense one;  pool: y_pool requested
# want: what the host code has to select for the case: ck, ms, ns, tile (th, tw), grid, cg (coGroup), chunks


def _c(kind, shape, algo=1, relu=1, family="randn", slices=(), pool=None, **want):
    n, cin, cout, h, w = shape
    if kind != "conv":
        relu = 0          # the transposed and the plain 1x1 convolution have none
    if pool is None:
        pool = kind == "conv" and h % 2 == 0 and w % 2 == 0
    name = f"{kind}{'-wino' if algo == 2 else ''}-{n}x{cin}x{cout}x{h}x{w}-{family}-relu{relu}"
    return Case(name, kind, n, cin, cout, h, w, algo, relu, family, tuple(slices), pool, want)


def _cat(cout):
    return ((2 * cout, 0), (2 * cout, cout))


CASES = [
    # ---- direct 3x3: every (CK, MS, NS) instance, ragged / straddling / tiny maps, 64 chunks
    _c("conv", (1, 4, 128, 7, 16), relu=1, family="randn", ck=4, ms=4, ns=4),
    _c("conv", (1, 16, 128, 8, 16), relu=0, family="relu", ck=16, ms=4, ns=4),
    _c("conv", (3, 16, 128, 7, 9), relu=1, family="hot", ck=16, ms=4, ns=4),
    _c("conv", (1, 4, 64, 8, 28), relu=0, family="hot", ck=4, ms=7, ns=2),
    _c("conv", (2, 4, 128, 14, 14), relu=1, family="relu", ck=4, ms=7, ns=2, grid=4),
    _c("conv", (2, 48, 36, 10, 14), relu=0, family="randn", ck=16, ms=4, ns=2, chunks=3),
    _c("conv", (2, 48, 36, 10, 14), relu=1, family="relu", ck=16, ms=4, ns=2, chunks=3),
    _c("conv", (2, 48, 36, 10, 14), relu=1, family="hot", ck=16, ms=4, ns=2, chunks=3),
    _c("conv", (1, 4, 4, 1, 1), relu=0, family="randn", ck=4, ms=4, ns=2),
    _c("conv", (1, 8, 8, 3, 5), relu=1, family="hot", ck=4, ms=4, ns=2),
    _c("conv", (1, 1024, 64, 4, 4), relu=1, family="relu", ck=16, ms=4, ns=2, chunks=64),
    _c("conv", (2, 64, 32, 12, 36), relu=0, family="randn", ck=16, ms=7, ns=2, tile=(28, 8)),
    _c("conv", (9, 16, 64, 14, 16), relu=1, family="relu", ck=16, ms=7, ns=2, grid=9),   # XCD remap tail (bid >= 8)
    # ---- Winograd with the fused pool
    _c("conv", (1, 16, 4, 2, 2), algo=2, relu=0, family="hot", chunks=1, cg=2),
    _c("conv", (3, 16, 32, 2, 6), algo=2, relu=1, family="randn", chunks=1, grid=2),
    _c("conv", (5, 48, 20, 14, 14), algo=2, relu=1, family="relu", chunks=3, tile=(18, 7)),
    _c("conv", (5, 48, 20, 14, 14), algo=2, relu=0, family="hot", chunks=3, tile=(18, 7)),
    _c("conv", (1, 1024, 64, 4, 4), algo=2, relu=1, family="relu", chunks=64),
    _c("conv", (1, 32, 64, 16, 32), algo=2, relu=0, family="randn", chunks=2, tile=(8, 16), grid=2),
    _c("conv", (2, 128, 64, 16, 48), algo=2, relu=1, family="relu", tile=(16, 8), grid=6),
    _c("conv", (7, 512, 96, 14, 14), algo=2, relu=1, family="randn", grid=12, cg=4),     # XCD remap tail
    _c("conv", (1, 64, 128, 56, 56), algo=2, relu=1, family="relu", grid=28, cg=4),
    _c("conv", (1, 16, 256, 8, 8), algo=2, relu=0, family="randn", cg=8, grid=8),
    # ---- transposed convolution
    _c("up", (1, 4, 32, 8, 16), family="randn", ck=4, ms=4, ns=4),
    _c("up", (1, 16, 32, 8, 16), family="relu", ck=16, ms=4, ns=4),
    _c("up", (1, 4, 8, 4, 56), family="hot", ck=4, ms=7, ns=2),
    _c("up", (1, 4, 20, 7, 8), family="relu", ck=4, ms=4, ns=4),      # cout % 16 != 0: padded (a,b) groups
    _c("up", (2, 16, 12, 7, 16), family="randn", ck=16, ms=7, ns=2),
    _c("up", (1, 4, 4, 1, 1), family="randn", ck=4, ms=4, ns=2),
    _c("up", (1, 16, 4, 8, 16), family="hot", ck=16, ms=4, ns=2),
    _c("up", (1, 1024, 512, 4, 4), family="relu", ck=16, ms=4, ns=4, chunks=64, cg=8),
    # ---- plain 1x1 (the training step's input gradient of the transposed convolution)
    _c("c1", (1, 4, 128, 8, 16), family="randn", ck=4, ms=4, ns=4),
    _c("c1", (1, 16, 128, 8, 16), family="relu", ck=16, ms=4, ns=4),
    _c("c1", (1, 4, 64, 8, 28), family="relu", ck=4, ms=7, ns=2),
    _c("c1", (1, 16, 64, 8, 28), family="randn", ck=16, ms=7, ns=2),
    _c("c1", (1, 4, 32, 8, 16), family="hot", ck=4, ms=4, ns=2),
    _c("c1", (3, 128, 64, 12, 16), family="randn", ck=16, ms=4, ns=2, slices=_cat(64)),
    # ---- concat halves and strides: dense, lower half, upper half (and an unaligned slice)
    _c("conv", (2, 32, 64, 28, 28), algo=1, relu=1, family="relu", slices=_cat(64) + ((68, 4),), ck=16, ms=7, ns=2),
    _c("conv", (2, 32, 64, 28, 28), algo=2, relu=1, family="relu", slices=_cat(64) + ((68, 4),), chunks=2),
    _c("conv", (5, 48, 20, 14, 14), algo=1, relu=1, family="randn", slices=_cat(20), ck=16, ms=7, ns=2),
    _c("conv", (5, 48, 20, 14, 14), algo=2, relu=1, family="randn", slices=_cat(20), chunks=3),
    _c("up", (3, 64, 32, 14, 14), family="randn", slices=_cat(32), ck=16, ms=7, ns=2),
]
assert len({c.name for c in CASES}) == len(CASES)
BY_NAME = {c.name: c for c in CASES}


def terms(c):
    return 9 * c.cin if c.kind == "conv" else c.cin


def plan_query(c):
    """the query of unet_host_plan_conv_f32 for a case"""
    return [{"conv": 9, "up": 1, "c1": 2}[c.kind], c.n, c.h, c.w, c.cin, c.cout, c.algo if c.kind == "conv" else 0]


def check_plan(c, plan):
    """plan: the 8 integers of path_out / unet_host_plan_conv_f32 -> a description; asserts what the case was written for"""
    algo, ms, ns, th, tw, grid, cg, _ = plan
    assert algo == c.algo, (c.name, plan)
    ck = 16 if c.cin % 16 == 0 else 4
    want = dict(c.want)
    chunks = c.cin // (16 if algo == 2 else ck)
    got = {"ck": ck, "ms": ms, "ns": ns, "tile": (th, tw), "grid": grid, "cg": cg, "chunks": chunks}
    for k, v in want.items():
        assert got[k] == v, (c.name, k, got[k], v, plan)
    if algo == 2:
        return f"wino_f32_kernel<2> tile grid {th}x{tw}, {chunks} chunks, grid {grid}, coGroup {cg}"
    taps, mode = {"conv": (9, 0), "up": (1, 1), "c1": (1, 0)}[c.kind]
    nld = {(16, 7): 6, (16, 4): 4, (4, 7): 2, (4, 4): 1}[(ck, ms)]
    return f"igemm_f32_kernel<{ck},{taps},{ms},{ns},{nld},{mode}> tile {th}x{tw}, {chunks} chunks, grid {grid}, coGroup {cg}"


# ---- inputs ----------------------------------------------------------------------------------------------------------

def _family(shape, family, gen):
    n, h, w, c = shape
    x = torch.randn(shape, generator=gen)
    if family == "relu":      # what a layer behind a ReLU sees: half the samples at a constant, half shifted up
        x = 3.0 * torch.relu(x) + 0.5
    elif family == "hot":     # exact-zero border ring, one hot pixel per image at each corner: separates every border tap
        hot = 4.0 * torch.randn((n, 2, 2, c), generator=gen) + 1.0 / 3.0
        ring = torch.zeros(h, w, dtype=torch.bool)
        ring[0, :] = ring[-1, :] = True
        ring[:, 0] = ring[:, -1] = True
        x[:, ring] = 0.0
        for i, yy in enumerate((0, h - 1)):
            for j, xx in enumerate((0, w - 1)):
                x[:, yy, xx] = hot[:, i, j]
    else:
        assert family == "randn"
    return x.float().contiguous()


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """-> x (N,H,W,Cin) fp32 NHWC, w in PyTorch layout, scale, shift (cout,) fp32; seeded by the case"""
    c = BY_NAME[name]
    gen = torch.Generator().manual_seed(1000 + CASES.index(c))
    x = _family((c.n, c.h, c.w, c.cin), c.family, gen)
    if c.kind == "conv":
        w = torch.randn(c.cout, c.cin, 3, 3, generator=gen) * (2.0 / (9 * c.cin)) ** 0.5
        sign = torch.where(torch.rand(c.cout, generator=gen) < 0.25, -1.0, 1.0)   # a quarter of the channels negative
        scale = (torch.rand(c.cout, generator=gen) + 0.5) * sign
        shift = torch.randn(c.cout, generator=gen) * 0.3
    elif c.kind == "up":
        w = torch.randn(c.cin, c.cout, 2, 2, generator=gen) * (1.0 / c.cin) ** 0.5
        scale = torch.ones(c.cout)
        shift = torch.randn(c.cout, generator=gen) * 0.2      # the bias
    else:
        w = torch.randn(c.cout, c.cin, generator=gen) * (1.0 / c.cin) ** 0.5
        scale, shift = torch.ones(c.cout), torch.zeros(c.cout)
    return x, w.float().contiguous(), scale.float().contiguous(), shift.float().contiguous()


# ---- the float64 model -----------------------------------------------------------------------------------------------

def ulp32(v):
    """spacing of fp32 at |v| (float64 array in, float64 out)"""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def reference_zb(kind, x, w):
    """x NHWC fp32, w PyTorch layout -> z, B float64 NHWC numpy (the transposed convolution at 2H x 2W)"""
    xd = x.double().permute(0, 3, 1, 2)
    wd = w.double()
    if kind == "conv":
        z, b2 = F.conv2d(xd, wd, padding=1), F.conv2d(xd * xd, wd * wd, padding=1)
    elif kind == "up":
        z, b2 = F.conv_transpose2d(xd, wd, stride=2), F.conv_transpose2d(xd * xd, wd * wd, stride=2)
    else:
        z, b2 = F.conv2d(xd, wd[:, :, None, None]), F.conv2d(xd * xd, (wd * wd)[:, :, None, None])
    return z.permute(0, 2, 3, 1).contiguous().numpy(), b2.clamp_min(0).sqrt().permute(0, 2, 3, 1).contiguous().numpy()


def result(z, scale, shift, relu):
    r = z * scale.double().numpy() + shift.double().numpy()
    return np.maximum(r, 0.0) if relu else r


def bound(r, B, scale, k):
    return C_ULP * ulp32(r) + C_ACC * U24 * np.sqrt(k) * np.abs(scale.double().numpy()) * B


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> r, bound, z, B (float64 NHWC numpy) of a case: computed once, shared, never written to"""
    c = BY_NAME[name]
    x, w, scale, shift = make_inputs(name)
    z, B = reference_zb(c.kind, x, w)
    r = result(z, scale, shift, c.relu)
    out = (r, bound(r, B, scale, terms(c)), z, B)
    for a in out:
        a.setflags(write=False)
    return out


def pool_max(y):
    """MaxPool2d(2,2) of an NHWC numpy array; -0.0 < +0.0 as the hardware's maximum orders them"""
    n, h, w, c = y.shape
    v = y.reshape(n, h // 2, 2, w // 2, 2, c)
    m = v.max(axis=(2, 4))
    if m.dtype == np.float32:     # numpy's max may return either zero: +0.0 wherever one of the four is +0.0
        poszero = ((v == 0) & ~np.signbit(v)).any(axis=(2, 4))
        m = np.where((m == 0) & poszero, np.float32(0.0), m)
    return m


def head_reference(x, w, bias):
    """x (P,C) fp32, w (C,) fp32 -> z, B float64"""
    xd, wd = x.astype(np.float64), w.astype(np.float64)
    return xd @ wd + float(bias), np.sqrt((xd * xd) @ (wd * wd))


def pack_u8_reference(frames, mean, std):
    """(N,H,W,3) uint8 -> (N,H,W,4) fp32: np.float32((np.float32(u8) - m) / s), pad channel +0.0"""
    out = np.zeros(frames.shape[:3] + (4,), np.float32)
    out[..., :3] = (frames.astype(np.float32) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return out


# ---- fp32 emulations of the kernels' arithmetic order ------------------------------------------------------------------

def _rnd32(a):
    return a.astype(np.float32).astype(np.float64)


def _ident(a):
    return a


def round_mantissa(x, bits):
    """round fp32 values to `bits` explicit mantissa bits (a mutation: operands of a narrower format)"""
    u = x.contiguous().view(torch.int32).numpy().astype(np.int64)
    drop = 23 - bits
    u = ((u + (1 << (drop - 1))) >> drop) << drop
    return torch.from_numpy(u.astype(np.int32)).view(torch.float32).reshape(x.shape)


def sample(c, budget=4_000_000, max_ch=32, seed=0):
    """output pixels (n, y, x) and channels to emulate: everything where that is cheap, else the 2x2 corner blocks of the
    first and the last image (every border tap), the last pixel and a seeded choice, `budget` multiply-adds in all"""
    ho, wo = (2 * c.h, 2 * c.w) if c.kind == "up" else (c.h, c.w)
    rng = np.random.RandomState(seed)
    ch = np.arange(c.cout)
    if c.cout > max_ch:
        rest = rng.permutation(np.arange(2, c.cout - 2))[:max_ch - 4]
        ch = np.sort(np.concatenate([[0, 1, c.cout - 2, c.cout - 1], rest]))
    allpix = np.stack(np.meshgrid(np.arange(c.n), np.arange(ho), np.arange(wo), indexing="ij"), -1).reshape(-1, 3)
    npix = max(16, budget // (terms(c) * len(ch)))
    if len(allpix) <= npix:
        return allpix, ch
    ys = sorted({0, min(1, ho - 1), max(ho - 2, 0), ho - 1})
    xs = sorted({0, min(1, wo - 1), max(wo - 2, 0), wo - 1})
    must = [(n, y, x) for n in sorted({0, c.n - 1}) for y in ys for x in xs]
    pick = allpix[rng.permutation(len(allpix))[:max(npix - len(must), 0)]]
    pix = np.unique(np.concatenate([np.array(must), pick]), axis=0)
    return pix, ch


def _gather(x, n, y, xx, wrap):
    """x (N,H,W,C) float64 numpy; pixel coordinates (arrays) -> (P,C); outside the image: zero, or with `wrap` (a
    mutation: border taps not masked) whatever lies there in memory - the neighbouring row or image"""
    N, H, W, _ = x.shape
    ok = (y >= 0) & (y < H) & (xx >= 0) & (xx < W)
    if wrap:
        flat = ((n * H + y) * W + xx) % (N * H * W)
        return x.reshape(N * H * W, -1)[flat]
    v = x[n, np.clip(y, 0, H - 1), np.clip(xx, 0, W - 1)]
    return v * ok[:, None]


def emulate_direct(c, x, w, pix, ch, exact=False, wrap=False):
    """igemm_f32.h:191-229: one accumulator per output, terms added one by one in the kernel's order - chunk of CK
    channels, tap, then the k of each MFMA (channel kc*CK + lq*KPL + e for e outermost, lq = 0..3 inside one MFMA).
    -> accumulators (P, len(ch)) as float64 (holding fp32 values unless `exact`)"""
    rnd = _ident if exact else _rnd32
    xd = x.double().numpy()
    wd = w.double().numpy()
    ck = 16 if c.cin % 16 == 0 else 4
    kpl = ck // 4
    n, y, xx = pix[:, 0], pix[:, 1], pix[:, 2]
    acc = np.zeros((len(pix), len(ch)))
    if c.kind == "up":
        src = _gather(xd, n, y // 2, xx // 2, False)
        ab = (y % 2) * 2 + (xx % 2)
        wk = wd[:, ch].reshape(c.cin, len(ch), 4)      # (ci, co, ab)
        taps = [None]
    elif c.kind == "c1":
        src = _gather(xd, n, y, xx, False)
        taps = [None]
    else:
        taps = [(t // 3, t % 3) for t in range(9)]
        srcs = [_gather(xd, n, y + ky - 1, xx + kx - 1, wrap) for ky, kx in taps]
    for kc in range(c.cin // ck):
        for ti, t in enumerate(taps):
            for e in range(kpl):
                for lq in range(4):
                    ci = kc * ck + lq * kpl + e
                    if c.kind == "conv":
                        term = srcs[ti][:, ci, None] * wd[ch, ci, t[0], t[1]][None, :]
                    elif c.kind == "up":
                        term = src[:, ci, None] * wk[ci][:, ab].T
                    else:
                        term = src[:, ci, None] * wd[ch, ci][None, :]
                    acc = rnd(acc + term)      # float64 holds the product of two fp32 exactly: one rounding, as an FMA
    return acc


_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)


def emulate_wino(c, x, w, pix, ch, exact=False, wrap=False):
    """wino_f32.h:270-367: U = G g G^T in float64 rounded to fp32; per chunk of 16 channels the input transform in the
    kernel's form (rows d0-d2, d1+d2, d2-d1, d1-d3, then the same on the columns), 16 point accumulators per output tile
    over the chunks (channel order of the MFMAs as in emulate_direct), output transform A^T = [1 1 1 0; 0 1 -1 -1].
    -> the value at each requested pixel (P, len(ch)) before scale / shift"""
    rnd = _ident if exact else _rnd32
    xd = x.double().numpy()
    g = w.double().numpy()[ch]                                     # (C', Cin, 3, 3)
    U = np.einsum("pa,ocab,qb->pqco", _G, g, _G)                   # (4, 4, Cin, C')
    U = rnd(U)
    n, ty, tx = pix[:, 0], pix[:, 1] // 2, pix[:, 2] // 2
    d = np.stack([np.stack([_gather(xd, n, 2 * ty - 1 + i, 2 * tx - 1 + j, wrap) for j in range(4)], 1)
                  for i in range(4)], 1)                           # (P, 4, 4, Cin)
    m = np.zeros((len(pix), 4, 4, len(ch)))
    for kc in range(c.cin // 16):
        dc = d[..., kc * 16:kc * 16 + 16]
        t = np.stack([rnd(dc[:, 0] - dc[:, 2]), rnd(dc[:, 1] + dc[:, 2]), rnd(dc[:, 2] - dc[:, 1]),
                      rnd(dc[:, 1] - dc[:, 3])], 1)                # rows
        v = np.stack([rnd(t[:, :, 0] - t[:, :, 2]), rnd(t[:, :, 1] + t[:, :, 2]), rnd(t[:, :, 2] - t[:, :, 1]),
                      rnd(t[:, :, 1] - t[:, :, 3])], 2)            # columns: (P, 4, 4, 16)
        for e in range(4):
            for lq in range(4):
                k = lq * 4 + e
                m = rnd(m + v[..., k, None] * U[None, :, :, kc * 16 + k, :])
    s0 = rnd(rnd(m[:, :, 0] + m[:, :, 1]) + m[:, :, 2])            # (P, 4, C'): columns of the output tile
    s1 = rnd(rnd(m[:, :, 1] - m[:, :, 2]) - m[:, :, 3])
    s = np.stack([s0, s1], 2)                                      # (P, 4, 2, C')
    y0 = rnd(rnd(s[:, 0] + s[:, 1]) + s[:, 2])
    y1 = rnd(rnd(s[:, 1] - s[:, 2]) - s[:, 3])
    yy = np.stack([y0, y1], 1)                                     # (P, 2, 2, C')
    return yy[np.arange(len(pix)), pix[:, 1] % 2, pix[:, 2] % 2]


def epilogue(acc, scale, shift, ch, relu, fused, exact=False):
    """acc * scale + shift (+ ReLU) in fp32: one rounding (fmaf, wino_f32.h:366; what the compiler may make of
    igemm_f32.h:263) or two"""
    rnd = _ident if exact else _rnd32
    sc, sh = scale.double().numpy()[ch], shift.double().numpy()[ch]
    v = rnd(acc * sc + sh) if fused else rnd(rnd(acc * sc) + sh)
    return np.maximum(v, 0.0) if relu else v


def emulate(c, x, w, pix, ch, exact=False, wrap=False):
    return (emulate_wino if c.algo == 2 else emulate_direct)(c, x, w, pix, ch, exact=exact, wrap=wrap)


def at(a, pix, ch):
    """the sampled elements of an NHWC array"""
    return a[pix[:, 0], pix[:, 1], pix[:, 2]][:, ch]
