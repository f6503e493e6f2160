"""The training step's MFMA operators, one at a time on the step's own launch sequences, against the float64 model of
tests/x3_model.py ("The training step's operators" there; tests/test_x3_model_cpu.py proves on the CPU that a faithful
emulation passes the bounds and that the listed mutations fail them).

Entry points (include/unet_hip.h): unet_op_train_conv3x3_x3 (forward and input-gradient 3x3 convolution with the fp32
epilogue of all three structures, both device packers, the power-of-two operand scaling, the fused BatchNorm statistics),
unet_op_upconv_bwd_x3 (column sum + maximum, space-to-depth planes, the 1x1 weight gradient with its mode-1 reduction, the
input-gradient GEMM on both structures), unet_op_upconv_fwd_train_x3 (the un-prescaled transposed-convolution packer) and
unet_op_wgrad3x3_x3.  Every fp32 output element is held to

    |got - r| <= 2^-23 |r| + 2^-15 |s| B                    (s the power-of-two output scale, B = sqrt(sum x~^2 w~^2))

every case asserts the path that ran, and outputs live in allocations filled with a NaN pattern: what is declared must be
written, everything else untouched.  The statistics are checked bit-exactly on integer-valued inputs.
profiles/r09/train_x3_ops.md keeps the measured ratios."""
import ctypes as C
import functools

import pytest
import torch

import x3_model as M
from x3_dispatch_queries import PATH, STAT_ROWS, VALID, ask, conv_query, switches_from_env
from x3_gpu_helpers import ERR_HIP, ERR_INVALID_ARG, R512, T448, WS, GuardedF32, Planes, _p, path_str, seed_of, to_dev

pytestmark = pytest.mark.gpu

REJECTED_WIDTHS = [428, 414]      # the f16q8 forms have no fp32 epilogue: every other tile width of the tier accepts it


@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    lib = _lib.load(build_if_missing=False)
    prev = lib.unet_set_x3_upconv_r512(-1)
    prev_q8 = lib.unet_set_x3_cross_fp8(0)
    yield lib
    lib.unet_set_x3_upconv_r512(prev)
    lib.unet_set_x3_cross_fp8(prev_q8)


def stop_on_hip_error(lib, rc):
    """a HIP error ends the session: nothing that runs on the device after it means anything"""
    if rc == ERR_HIP:
        pytest.exit("HIP error from an operator entry point", returncode=3)


# ---- forward and input-gradient 3x3 convolution -------------------------------------------------------------------------

def run_tconv(lib, w_dev, mode, packer, tw, shape, cout_op, *, planes=None, x32=None, scaled=0, ldo=0, off=0, stat_cap=0,
              expect_rc=0):
    """shape: (n, h, w, cin_op) of the operand -> dict(out GuardedF32 (n,h,w,ldo), path, inv, rows, stat, range)"""
    n, h, wd, cin_op = shape
    out = GuardedF32(n, h, wd, ldo or cout_op)
    stat = GuardedF32(stat_cap, 2, cout_op) if stat_cap else None
    path = (C.c_int * 8)()
    rows, rng, inv = C.c_int(-1), C.c_int(-1), C.c_float(-1.0)
    xp = xlo = None
    if planes is not None:
        xp, xlo = to_dev(*planes)       # [hi | lo]: the lo plane directly behind the hi plane
    rc = lib.unet_op_train_conv3x3_x3(0, _p(xp), _p(x32), scaled, n, h, wd, cin_op, cout_op, _p(w_dev), mode, packer, tw, out.ptr,
                                      ldo, off, stat.ptr if stat else None, stat_cap, C.byref(rows) if stat else None,
                                      C.byref(inv), path, C.byref(rng), None)
    stop_on_hip_error(lib, rc)
    assert rc == expect_rc, (rc, expect_rc, tw, shape, cout_op, mode)
    torch.cuda.synchronize()
    if rc == 0:     # the host-side plan for the same query is what the launch reported
        plan, _ = ask(lib, "conv", conv_query(n, h, wd, cin_op, cout_op, 3, tile_width=tw, co_off=off, stats=1 if stat else 0,
                                              switches=switches_from_env()))
        assert plan[VALID] == 1 and tuple(plan[PATH]) == tuple(path)[:7], (plan, tuple(path))
        assert not stat or plan[STAT_ROWS] == rows.value, (plan, rows.value)
    return dict(out=out, path=tuple(path)[:7], inv=inv.value, rows=rows.value, stat=stat, range=rng.value)


def operand(kind, shape, gen):
    if kind == "zero":
        return torch.zeros(*shape)
    mag = {"one": 1.0, "tiny": 3e-8, "outlier": 1e-5}[kind]
    g = (torch.randn(*shape, generator=gen) * mag).float()
    if kind == "outlier":               # one element 2^10 times the rest sets the scale
        g.view(-1)[g.numel() // 3] = mag * 2.0 ** 10
    return g


@functools.lru_cache(maxsize=2)
def tconv_case(n, h, w, cin, cout, mode, g_kind, w_std, as_planes, seed):
    """the layer's weight (cout, cin, 3, 3), the operand of the operator `mode` selects and the float64 model, computed once"""
    gen = torch.Generator().manual_seed(seed)
    wt = (torch.randn(cout, cin, 3, 3, generator=gen) * w_std).float().contiguous()
    cin_op, cout_op = (cout, cin) if mode else (cin, cout)
    g = operand(g_kind, (n, h, w, cin_op), gen)
    if as_planes:
        hi, lo = M.split_f16(g)
        k = 0
    else:
        hi, lo, k = M.scaled_split(g)
    m = M.model_train_conv(hi, lo, wt, mode, k, device="cuda")
    return dict(w=wt, g=g, hi=hi, lo=lo, k=k, m=m, cin_op=cin_op, cout_op=cout_op)


# (id, n, h, w, cin, cout of the LAYER, mode, forced tile width, expected (structure, tile width, flat, waves)).  mode 1 runs
# the input-gradient operator cout -> cin over the same (cout, cin, 3, 3) tensor.  First the issue's shapes, as the
# dispatch takes them by itself (small batches: the first structure) and on the forms their widths allow; then the
# smallest shapes (tests/test_x3_ops_gpu.py) that reach every remaining form with ragged tiles and more than one block.
A, B, Cc, D, E, Fs, G = ((2, 28, 28, 64, 128), (2, 28, 28, 64, 256), (1, 56, 56, 128, 64), (3, 14, 14, 256, 256),
                         (1, 20, 36, 64, 64), (2, 6, 10, 64, 64), (1, 32, 64, 128, 64))
TCONV_CASES = [
    ("A-m0-auto", *A, 0, 0, (WS, 32, 1, 0)),
    ("A-m0-r28", *A, 0, 28, (R512, 28, 1, 2)),
    ("A-m0-t628", *A, 0, 628, (T448, 28, 0, 2)),
    ("A-m1-auto", *A, 1, 0, (WS, 32, 1, 0)),
    ("A-m1-t628", *A, 1, 628, (T448, 28, 0, 1)),
    ("A-m1-ws16", *A, 1, 16, (WS, 16, 1, 0)),
    ("B-m0-auto", *B, 0, 0, (WS, 32, 1, 0)),
    ("B-m0-t728-flat", *B, 0, 728, (T448, 28, 1, 4)),
    ("B-m0-r28-flat", *B, 0, 28, (R512, 28, 1, 1)),
    ("B-m0-r228-flat", *B, 0, 228, (R512, 28, 1, 2)),
    ("B-m1-auto", *B, 1, 0, (WS, 32, 1, 0)),
    ("B-m1-t628", *B, 1, 628, (T448, 28, 0, 1)),
    ("C-m0-auto", *Cc, 0, 0, (WS, 32, 0, 0)),
    ("C-m0-t628", *Cc, 0, 628, (T448, 28, 0, 1)),
    ("C-m1-r28", *Cc, 1, 28, (R512, 28, 0, 2)),
    ("C-m1-t628", *Cc, 1, 628, (T448, 28, 0, 2)),
    ("D-m0-auto", *D, 0, 0, (WS, 16, 1, 0)),
    ("D-m0-r14-flat", *D, 0, 14, (R512, 14, 1, 1)),
    ("D-m1-r214-flat", *D, 1, 214, (R512, 14, 1, 2)),
    ("D-m1-auto", *D, 1, 0, (WS, 16, 1, 0)),
    ("E-m0-auto", *E, 0, 0, (WS, 32, 0, 0)),
    ("E-m0-ws16", *E, 0, 16, (WS, 16, 0, 0)),
    ("E-m1-ws32", *E, 1, 32, (WS, 32, 0, 0)),
    ("E-m1-ws16", *E, 1, 16, (WS, 16, 0, 0)),
    ("F-m0-auto", *Fs, 0, 0, (WS, 16, 1, 0)),
    ("F-m1-ws32", *Fs, 1, 32, (WS, 32, 1, 0)),
    ("G-m0-auto", *G, 0, 0, (WS, 32, 0, 0)),
    ("G-m0-t632", *G, 0, 632, (T448, 32, 0, 1)),
    ("G-m1-r532", *G, 1, 532, (R512, 32, 0, 2)),
    ("r28-w1", 1, 10, 28, 64, 256, 0, 28, (R512, 28, 0, 1)),
    ("r228", 1, 10, 28, 64, 256, 0, 228, (R512, 28, 0, 2)),
    ("r14-w1", 1, 6, 14, 64, 256, 0, 14, (R512, 14, 0, 1)),
    ("r214-m1", 1, 18, 14, 256, 128, 1, 214, (R512, 14, 0, 2)),
    ("r332", 1, 8, 32, 64, 256, 0, 332, (R512, 32, 0, 1)),
    ("r332-flat", 2, 8, 64, 64, 256, 0, 332, (R512, 32, 1, 1)),
    ("r316-m1", 1, 6, 16, 256, 64, 1, 316, (R512, 16, 0, 1)),
    ("r316-flat", 2, 8, 32, 64, 256, 0, 316, (R512, 16, 1, 1)),
    ("r308", 1, 6, 8, 64, 256, 0, 308, (R512, 8, 0, 1)),
    ("r308-flat-m1", 2, 16, 24, 256, 64, 1, 308, (R512, 8, 1, 1)),
    ("r532-flat", 2, 8, 32, 64, 256, 0, 532, (R512, 32, 1, 2)),
    ("t728-m1", 1, 10, 28, 256, 64, 1, 728, (T448, 28, 0, 4)),
    ("t632-n2", 2, 10, 64, 64, 128, 0, 632, (T448, 32, 0, 1)),
]
G_KINDS = ("one", "tiny", "outlier")
W_STDS = (0.05, 1e-3)


def test_cases_cover_the_dispatch():
    """the table reaches every form of the three structures that has an fp32 epilogue (run_conv_x3), flat and per image, in
    both modes; each case then asserts its row's path through path_out"""
    seen = {r[8] for r in TCONV_CASES}
    for tw in (16, 32):
        for flat in (0, 1):
            assert (WS, tw, flat, 0) in seen, (tw, flat)
    for tw, waves in ((28, 1), (28, 2), (14, 1), (14, 2), (32, 1), (32, 2), (16, 1), (8, 1)):
        for flat in (0, 1):
            assert (R512, tw, flat, waves) in seen, (tw, waves, flat)
    for key in ((T448, 28, 0, 1), (T448, 28, 0, 2), (T448, 28, 0, 4), (T448, 28, 1, 4), (T448, 32, 0, 1)):
        assert key in seen, key
    for structure in (WS, R512, T448):
        assert {r[6] for r in TCONV_CASES if r[8][0] == structure} == {0, 1}, structure
    for shape in (A, B, Cc, D, E, Fs, G):
        assert {r[6] for r in TCONV_CASES if tuple(r[1:6]) == shape} == {0, 1}, shape
    assert not set(REJECTED_WIDTHS) & {r[7] for r in TCONV_CASES}


@pytest.mark.parametrize("row", TCONV_CASES, ids=[r[0] for r in TCONV_CASES])
def test_train_conv3x3(lib, row):
    """both packers (bit-identical), ldo = 2 cout at off = cout and off = 0 with the other half and the guards intact; the
    forward rows alternate between caller-owned planes (the step's planes mode) and the scaled fp32 path, the
    input-gradient rows take the scaled path; magnitudes and weight scales rotate through the table"""
    name, n, h, w, cin, cout, mode, tw, want = row
    i = [r[0] for r in TCONV_CASES].index(name)
    as_planes = mode == 0 and i % 2 == 0
    g_kind = "one" if as_planes else G_KINDS[i % 3]
    case = tconv_case(n, h, w, cin, cout, mode, g_kind, W_STDS[(i // 2) % 2], as_planes, seed_of(name))
    cin_op, cout_op, m = case["cin_op"], case["cout_op"], case["m"]
    w_dev = case["w"].cuda()
    kw = dict(planes=(case["hi"], case["lo"])) if as_planes else dict(x32=case["g"].cuda(), scaled=1)
    shape = (n, h, w, cin_op)
    want_path = (want[0], want[1], 3, want[2], 1, want[3], 0)
    res = run_tconv(lib, w_dev, mode, 0, tw, shape, cout_op, ldo=2 * cout_op, off=cout_op, **kw)
    label = f"{name} mode {mode} g {g_kind}{' planes' if as_planes else ' scaled'} [{path_str(res['path'])}]"
    assert res["path"] == want_path, f"{label}: expected {path_str(want_path)}"
    assert res["inv"] == 2.0 ** -case["k"], (label, res["inv"], case["k"])
    res["out"].assert_written_only(label, cout_op, 2 * cout_op)
    M.check_f32(res["out"].values()[..., cout_op:], m["r"], m["s"], m["B"], label)
    assert res["range"] == 0, f"{label}: range reported"
    res1 = run_tconv(lib, w_dev, mode, 1, tw, shape, cout_op, ldo=2 * cout_op, off=0, **kw)
    assert res1["path"] == want_path, f"{label}: the LDS packer's run took {path_str(res1['path'])}"
    res1["out"].assert_written_only(label + " off 0", 0, cout_op)
    assert torch.equal(res1["out"].bits()[..., :cout_op], res["out"].bits()[..., cout_op:]), \
        f"{label}: the two packers' outputs differ"


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("w_std", W_STDS)
@pytest.mark.parametrize("g_kind", G_KINDS + ("zero",))
def test_train_conv3x3_magnitudes(lib, mode, w_std, g_kind):
    """every operand magnitude against both weight scales on one shape with two channel tiles (cin != cout): g ~ 1, ~ 3e-8,
    an outlier 2^10 above the rest, and all zeros (k = 0, the output exactly zero)"""
    n, h, w, cin, cout = 2, 6, 10, 64, 128
    case = tconv_case(n, h, w, cin, cout, mode, g_kind, w_std, False, seed_of("mag", mode, w_std, g_kind))
    if w_std == 1e-3:
        assert (M.split_f16(case["w"])[1].float().abs() < 2.0 ** -14).all()       # subnormal lo parts
    res = run_tconv(lib, case["w"].cuda(), mode, 0, 0, (n, h, w, case["cin_op"]), case["cout_op"], x32=case["g"].cuda(), scaled=1)
    label = f"magnitudes mode {mode} w~{w_std} g {g_kind} [{path_str(res['path'])}]"
    assert res["path"][0] == WS and res["path"][2] == 3, label
    assert res["inv"] == 2.0 ** -case["k"], (label, res["inv"], case["k"])
    res["out"].assert_written_only(label)
    if g_kind == "zero":
        assert case["k"] == 0 and not res["out"].values().any(), f"{label}: the output of a zero operand is not zero"
    else:
        M.check_f32(res["out"].values(), case["m"]["r"], case["m"]["s"], case["m"]["B"], label)


# ---- fused BatchNorm statistics: integer-exact -----------------------------------------------------------------------

# (id, n, h, w, cout, forced tile width, expected (structure, tile width, flat, waves), expected rows or None = any > 0)
STAT_CASES = [
    ("t628-c2-ragged", 2, 28, 28, 128, 628, (T448, 28, 0, 2), None),
    ("t628-c1-ragged", 1, 18, 28, 64, 628, (T448, 28, 0, 1), None),
    ("t632-c1", 1, 18, 32, 64, 632, (T448, 32, 0, 1), None),
    ("t728-c4-flat", 2, 28, 28, 256, 728, (T448, 28, 1, 4), None),
    ("t728-c4-ragged", 1, 10, 28, 256, 728, (T448, 28, 0, 4), None),
    # 3 x 2 x 2 pixel tiles x 3 channel groups = 36 items: the grid of 32 shrinks to 24, a multiple of the groups' count
    ("t628-grid-shrunk", 3, 32, 56, 192, 628, (T448, 28, 0, 1), 24 * 4),
    ("r28-w1-flat", 2, 28, 28, 256, 28, (R512, 28, 1, 1), None),
    ("r228-w2-flat", 2, 28, 28, 256, 228, (R512, 28, 1, 2), None),
    ("r28-w2-ragged", 1, 10, 56, 128, 28, (R512, 28, 0, 2), None),
    ("r14-w1-flat", 3, 14, 14, 256, 14, (R512, 14, 1, 1), None),
    ("r214-w2", 1, 18, 14, 128, 214, (R512, 14, 0, 2), None),
    ("ws32-no-fusion", 1, 20, 36, 64, 32, (WS, 32, 0, 0), 0),
    ("ws16-flat-no-fusion", 2, 6, 10, 64, 16, (WS, 16, 1, 0), 0),
]
STAT_CAP = 1100      # rows of the caller's buffer: the entry point asks for room for the largest grid (256 blocks x 4)


@pytest.mark.parametrize("row", STAT_CASES, ids=[r[0] for r in STAT_CASES])
def test_fused_statistics_are_exact(lib, row):
    """x_hi integers in [-2, 2], x_lo = 0, weights in {-1, 0, 1}, cin = 64: every z is an integer and every channel's sum
    of z^2 stays below 2^24 (asserted on the float64 reference), so every fp32 partial sum in any order is exact: the rows
    the epilogue left, added in float64, must EQUAL sum z and sum z^2 per channel.  The epilogue writes into the test's
    own guarded buffer (the entry point hands it over as the step hands over its scratch): rows beyond the reported count
    and the guards stay untouched, z with the statistics is bit-identical to z without, and a structure that does not fuse
    reports 0 rows and leaves the buffer alone."""
    name, n, h, w, cout, tw, want, want_rows = row
    gen = torch.Generator().manual_seed(seed_of(name))
    xh, xl, wt = M.integer_case(n, h, w, 64, cout, gen)
    z = M.model_train_conv(xh, xl, wt, 0, device="cuda")["r"]
    M.stat_reference(z)                                      # fails (does not skip) where the exactness argument breaks
    w_dev = wt.cuda()
    want_path = (want[0], want[1], 3, want[2], 1, want[3], 0)
    res = run_tconv(lib, w_dev, 0, 1, tw, (n, h, w, 64), cout, planes=(xh, xl), stat_cap=STAT_CAP)
    label = f"{name} [{path_str(res['path'])}] rows {res['rows']}"
    print(label)
    assert res["path"] == want_path, f"{label}: expected {path_str(want_path)}"
    res["out"].assert_written_only(label)
    assert torch.equal(res["out"].values().cpu().double(), z), f"{label}: z is not the exact integer result"
    plain = run_tconv(lib, w_dev, 0, 1, tw, (n, h, w, 64), cout, planes=(xh, xl))
    assert plain["path"] == want_path and torch.equal(plain["out"].bits(), res["out"].bits()), \
        f"{label}: z with the statistics differs from z without"
    if want[0] == WS:
        assert res["rows"] == 0, label
        res["stat"].assert_untouched(label)
        return
    assert 0 < res["rows"] <= STAT_CAP and (want_rows is None or res["rows"] == want_rows), label
    st = res["stat"]
    assert (st.bits()[res["rows"]:] == st.PATTERN).all(), f"{label}: rows beyond the reported count written"
    assert (st.buf[:st.guard] == st.PATTERN).all() and (st.buf[st.guard + st.elems:] == st.PATTERN).all(), f"{label}: guard overwritten"
    rows = st.values()[:res["rows"]]
    assert not (st.bits()[:res["rows"]] == st.PATTERN).any(), f"{label}: reported rows not written"
    M.check_stat_rows(rows, z, label)


def test_statistics_capacity_is_respected(lib):
    """the rows go straight to the caller, so room for the largest grid (1024 rows) is demanded up front: less is
    INVALID_ARG with that count reported, nothing launched, the buffer untouched"""
    gen = torch.Generator().manual_seed(5)
    xh, xl, wt = M.integer_case(1, 18, 28, 64, 64, gen)
    res = run_tconv(lib, wt.cuda(), 0, 0, 628, (1, 18, 28, 64), 64, planes=(xh, xl), stat_cap=1023, expect_rc=ERR_INVALID_ARG)
    assert res["rows"] == 1024
    res["stat"].assert_untouched("capacity")
    res["out"].assert_untouched("capacity")


def test_train_conv3x3_unscaled_fp32(lib):
    """an fp32 operand in the fp16 range, split without a key (split_planes_kernel: the step's path for a unit whose input
    is not kept in planes): inv stays 1, the same bound"""
    n, h, w, cin, cout = 2, 6, 10, 64, 128
    gen = torch.Generator().manual_seed(seed_of("unscaled"))
    wt = (torch.randn(cout, cin, 3, 3, generator=gen) * 0.05).float().contiguous()
    x = torch.randn(n, h, w, cin, generator=gen).float()
    m = M.model_train_conv(*M.split_f16(x), wt, 0, 0, device="cuda")
    for packer in (0, 1):
        res = run_tconv(lib, wt.cuda(), 0, packer, 0, (n, h, w, cin), cout, x32=x.cuda(), scaled=0)
        label = f"unscaled fp32 packer {packer} [{path_str(res['path'])}]"
        assert res["path"][0] == WS and res["path"][2] == 3 and res["inv"] == 1.0, label
        res["out"].assert_written_only(label)
        M.check_f32(res["out"].values(), m["r"], 1.0, m["B"], label)


# ---- transposed convolution, backward ------------------------------------------------------------------------------

UPBWD_SHAPES = [(2, 14, 14, 64), (1, 7, 12, 128), (3, 4, 4, 256), (1, 28, 28, 64)]


@functools.lru_cache(maxsize=2)
def upbwd_case(n, h, w, f, mag):
    gen = torch.Generator().manual_seed(seed_of("upbwd", n, h, w, f, mag))
    g = (torch.randn(n, 2 * h, 2 * w, f, generator=gen) * mag).float()
    xh, xl = M.split_f16(torch.randn(n, h, w, 2 * f, generator=gen).abs())        # a post-ReLU activation
    wt = (torch.randn(2 * f, f, 2, 2, generator=gen) * (1.0 / (2 * f)) ** 0.5).float().contiguous()
    return dict(g=g, xh=xh, xl=xl, w=wt, m=M.model_upconv_bwd(g, xh, xl, wt, device="cuda"))


@pytest.mark.parametrize("structure", [WS, R512])
@pytest.mark.parametrize("mag", [1.0, 3e-8])
@pytest.mark.parametrize("shape", UPBWD_SHAPES, ids=str)
def test_upconv_backward(lib, shape, mag, structure):
    """the gradient slice sits in the upper channel half of a (N, 2h, 2w, 2f) buffer whose skip half is NaN: nothing of it
    may reach the maximum, the sums or the planes.  dW, dIn, db against the model; inv the exact power of two"""
    n, h, w, f = shape
    case = upbwd_case(n, h, w, f, mag)
    m = case["m"]
    dy = torch.full((n, 2 * h, 2 * w, 2 * f), float("nan"))
    dy[..., f:] = case["g"]
    dy = dy.cuda()
    xp, _ = to_dev(case["xh"], case["xl"])
    w_dev = case["w"].cuda()
    db, dw, din = GuardedF32(f), GuardedF32(2 * f, f, 2, 2), GuardedF32(n, h, w, 2 * f)
    inv, st = C.c_float(-1.0), C.c_int(-1)
    prev = lib.unet_set_x3_upconv_r512(1 if structure == R512 else 0)
    try:
        rc = lib.unet_op_upconv_bwd_x3(0, _p(dy), 2 * f, f, _p(xp), _p(w_dev), n, h, w, f, db.ptr, dw.ptr, din.ptr,
                                       C.byref(inv), C.byref(st), None)
    finally:
        lib.unet_set_x3_upconv_r512(prev)
    torch.cuda.synchronize()
    label = f"upconv bwd {shape} g~{mag} structure {st.value}"
    stop_on_hip_error(lib, rc)
    assert rc == 0, (label, rc)
    assert st.value == structure, f"{label}: expected the GEMM on structure {structure}"
    assert inv.value == m["inv"] and inv.value == 2.0 ** -m["k"], (label, inv.value, m["k"])
    for name, t in (("db", db), ("dW", dw), ("dIn", din)):
        t.assert_written_only(f"{label} {name}")
    M.check_f32(dw.values(), m["dW"], m["inv"], m["dW_B"], label + " dW")
    M.check_f32(din.values(), m["dIn"], m["inv"], m["dIn_B"], label + " dIn")
    err = (db.values().cpu().double() - m["db"]).abs()
    print(f"{label} db: max err/bound {(err / m['db_bound']).max().item():.4f}")
    assert (err <= m["db_bound"]).all(), f"{label}: db outside the column sum's bound"


# ---- transposed convolution, forward, device-packed ------------------------------------------------------------------

@pytest.mark.parametrize("structure", [WS, R512])
@pytest.mark.parametrize("shape", [(2, 14, 14, 128, 64), (1, 7, 9, 256, 128)], ids=str)
def test_upconv_forward_device_packed(lib, shape, structure):
    """pack_upconv_x3_kernel (no pre-scale, unit scale, the bias as the shift) into the upper half of a concat buffer"""
    n, h, w, cin, cout = shape
    gen = torch.Generator().manual_seed(seed_of("upfwd", shape))
    xh, xl = M.split_f16(torch.randn(n, h, w, cin, generator=gen).abs())
    wt = (torch.randn(cin, cout, 2, 2, generator=gen) * (1.0 / cin) ** 0.5).float().contiguous()
    bias = (torch.randn(cout, generator=gen) * 0.3).float()
    w_hi, w_lo = M.split_w(wt)
    z, B = M.three_products(xh.double().cuda(), xl.double().cuda(), w_hi.cuda(), w_lo.cuda(), M.upconv2)
    r = M.epilogue(z.cpu(), torch.ones(cout, dtype=torch.float64), bias.double(), False)
    x, xlo = to_dev(xh, xl)
    y = Planes(n, 2 * h, 2 * w, 2 * cout)
    w_dev, b_dev = wt.cuda(), bias.cuda()
    path = (C.c_int * 8)()
    rng = C.c_int(-1)
    prev = lib.unet_set_x3_upconv_r512(1 if structure == R512 else 0)
    try:
        rc = lib.unet_op_upconv_fwd_train_x3(0, _p(x), xlo, n, h, w, cin, _p(w_dev), _p(b_dev), cout, y.ptr, y.lo_off, 2 * cout,
                                             cout, path, C.byref(rng), None)
    finally:
        lib.unet_set_x3_upconv_r512(prev)
    torch.cuda.synchronize()
    label = f"upconv fwd (device-packed) {shape} [{path_str(tuple(path)[:7])}]"
    stop_on_hip_error(lib, rc)
    assert rc == 0, (label, rc)
    assert path[0] == structure and path[2] == 0, f"{label}: expected structure {structure}"
    y.assert_written_only(cout, 2 * cout, label)
    gh, gl = y.halves(cout, 2 * cout)
    M.check(gh, gl, r, torch.ones(cout, dtype=torch.float64), B.cpu(), label)
    assert rng.value == 0, f"{label}: range reported"


# ---- rejections ------------------------------------------------------------------------------------------------------

def test_entry_points_reject_what_they_cannot_run(lib):
    gen = torch.Generator().manual_seed(3)
    wt = torch.randn(64, 64, 3, 3, generator=gen).cuda()
    x32 = torch.randn(1, 6, 10, 64, generator=gen).cuda()
    for tw in REJECTED_WIDTHS:        # the forms without an fp32 epilogue: an explicit list, each INVALID_ARG
        run_tconv(lib, wt, 0, 0, tw, (1, 6, 10, 64), 64, x32=x32, scaled=1, expect_rc=ERR_INVALID_ARG)
    run_tconv(lib, wt, 0, 0, 0, (1, 6, 10, 96), 64, x32=x32, scaled=1, expect_rc=ERR_INVALID_ARG)     # channels % 64
    run_tconv(lib, wt, 1, 0, 0, (1, 6, 10, 64), 32, x32=x32, scaled=1, expect_rc=ERR_INVALID_ARG)
    run_tconv(lib, wt, 0, 0, 332, (1, 6, 10, 64), 64, x32=x32, scaled=1, expect_rc=ERR_INVALID_ARG)   # 7 x 32 tiles: W % 32
    run_tconv(lib, wt, 0, 0, 728, (1, 6, 10, 64), 64, x32=x32, scaled=1, expect_rc=ERR_INVALID_ARG)   # 256 channels per block
    run_tconv(lib, wt, 0, 0, 32, (1, 6, 10, 64), 64, x32=x32, scaled=1, ldo=128, off=128, expect_rc=ERR_INVALID_ARG)
    q = _p(x32)
    for f in (32, 48, 96):            # the 1x1 weight gradient's rows 4 f and columns 2 f must be multiples of 128
        assert lib.unet_op_upconv_bwd_x3(0, q, 2 * f, f, q, q, 1, 2, 2, f, q, q, q, None, None, None) == ERR_INVALID_ARG
    assert lib.unet_op_wgrad3x3_x3(0, q, q, 1, 5, 4, 64, 64, q, 0, None) == ERR_INVALID_ARG            # odd h
    assert lib.unet_op_wgrad3x3_x3(0, q, q, 1, 4, 4, 96, 64, q, 0, None) == ERR_INVALID_ARG
    assert lib.unet_op_wgrad3x3_x3(0, q, q, 1, 4, 4, 64, 32, q, 0, None) == ERR_INVALID_ARG
