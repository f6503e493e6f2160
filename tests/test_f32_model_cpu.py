"""fp32 tier, no GPU: the bound of tests/f32_model.py is wide enough for fp32 arithmetic in the kernels' order and narrow
enough to catch a kernel that is subtly wrong; and the case table of tests/test_f32_ops_gpu.py reaches every instance the
host code can select.

Two numpy emulations (f32_model.emulate_direct, f32_model.emulate_wino) add the terms of an output in the order
csrc/igemm_f32.h and csrc/wino_f32.h add them, each partial sum rounded to fp32.  They stay inside a quarter of the
bound on every case; with one defect planted - a term dropped, two taps swapped, operands of 10 mantissa bits, the
scale / shift of two neighbouring channels exchanged, border taps that read the neighbouring row instead of zero - they
leave it, on every case the defect applies to."""
import ctypes as C

import numpy as np
import pytest

import f32_model as M


def _mutation_sample(c):
    """a small sample for the planted defects: the corner blocks (every border tap) and a few pixels, 8 channels"""
    return M.sample(c, budget=48 * 8 * M.terms(c), max_ch=8, seed=1)


@pytest.mark.parametrize("c", [c for c in M.CASES if c.algo == 2], ids=lambda c: c.name)
def test_winograd_emulation_in_float64_is_the_convolution(c):
    """pins the transform matrices (and the gather of the 4x4 patches): without rounding the emulation is exact"""
    x, w, scale, shift = M.make_inputs(c.name)
    pix, ch = M.sample(c, budget=1_000_000)
    z = M.at(M.reference(c.name)[2], pix, ch)
    got = M.emulate_wino(c, x, w, pix, ch, exact=True)
    assert np.abs(got - z).max() <= 1e-12 * max(1.0, np.abs(z).max())
    d = M.emulate_direct(c, x, w, pix, ch, exact=True)
    assert np.abs(d - z).max() <= 1e-12 * max(1.0, np.abs(z).max())


@pytest.mark.parametrize("c", M.CASES, ids=lambda c: c.name)
def test_emulations_inside_a_quarter_of_the_bound(c):
    """fp32 arithmetic in either kernel's order, with the epilogue rounded once or twice, uses at most a quarter of the
    bound; prints the ratios C_ACC and C_ULP were sized by (f32_model's docstring)"""
    x, w, scale, shift = M.make_inputs(c.name)
    pix, ch = M.sample(c)
    r, bound, z, B = (M.at(a, pix, ch) for a in M.reference(c.name))
    k = M.terms(c)
    unit = M.U24 * np.sqrt(k) * B
    emus = [("direct", M.emulate_direct)]
    if c.kind == "conv" and c.cin % 16 == 0 and c.h % 2 == 0 and c.w % 2 == 0:
        emus.append(("wino", M.emulate_wino))
    sc = np.abs(scale.double().numpy()[ch])
    for name, emu in emus:
        acc = emu(c, x, w, pix, ch)
        pos = unit > 0
        rho_acc = float((np.abs(acc - z)[pos] / unit[pos]).max()) if pos.any() else 0.0
        assert (np.abs(acc - z)[~pos] == 0).all()
        rho_ulp = 0.0
        for fused in ((True,) if name == "wino" else (True, False)):
            out = M.epilogue(acc, scale, shift, ch, c.relu, fused)
            err = np.abs(out - r)
            assert (err <= bound / 4).all(), (c.name, name, fused, float((err / bound).max()))
            # the ulp term is sized where it is the larger one, on the small-K cases
            u = M.ulp32(r)
            dom = u >= unit * sc
            if k <= 144 and dom.any():
                rho_ulp = max(rho_ulp, float((err[dom] / u[dom]).max()))
        print(f"{c.name} [{name} emulation]: |acc - z| / (2^-24 sqrt(K) B) <= {rho_acc:.3f}, |out - r| / ulp32 where the ulp term leads <= {rho_ulp:.3f}")
        # the constants are 4 x the measured worst (rounded up), never fitted per case
        assert 4 * rho_acc <= M.C_ACC and 4 * rho_ulp <= M.C_ULP, (c.name, name, rho_acc, rho_ulp)


def test_bound_is_far_below_one_dropped_term():
    """condition, not measurement: at the largest K of the table the accumulation term of the bound is at least 64 x
    below the average size of one term, |scale| B / sqrt(K)"""
    kmax = max(M.terms(c) for c in M.CASES)
    assert kmax == 9 * 1024
    assert M.C_ACC * M.U24 * kmax <= 1.0 / 64


def _worst(c, x, w, scale, shift, pix, ch, wrap=False):
    r, bound = (M.at(a, pix, ch) for a in M.reference(c.name)[:2])
    out = M.epilogue(M.emulate(c, x, w, pix, ch, wrap=wrap), scale, shift, ch, c.relu, True)
    return float((np.abs(out - r) / bound).max())


def _swap(t, i, j):
    t = t.clone()
    t[i], t[j] = t[j].clone(), t[i].clone()
    return t


@pytest.mark.parametrize("c", M.CASES, ids=lambda c: c.name)
def test_planted_defects_leave_the_bound(c):
    x, w, scale, shift = M.make_inputs(c.name)
    pix, ch = _mutation_sample(c)
    assert ch[0] == 0 and ch[1] == 1
    assert _worst(c, x, w, scale, shift, pix, ch) <= 0.25          # the sample itself is clean
    seen = {}
    # one (channel, tap) term dropped: channel 0 at the centre tap / at (a,b) = (0,0)
    wd = w.clone()
    if c.kind == "conv":
        wd[:, 0, 1, 1] = 0
    elif c.kind == "up":
        wd[0, :, 0, 0] = 0
    else:
        wd[:, 0] = 0
    seen["term dropped"] = _worst(c, x, wd, scale, shift, pix, ch)
    # two taps swapped (the plain 1x1 convolution has one)
    if c.kind == "conv":
        ws = w.clone()
        ws[:, :, 1, 1], ws[:, :, 1, 2] = w[:, :, 1, 2], w[:, :, 1, 1]
        seen["taps swapped"] = _worst(c, x, ws, scale, shift, pix, ch)
    elif c.kind == "up":
        ws = w.clone()
        ws[:, :, 0, 0], ws[:, :, 0, 1] = w[:, :, 0, 1], w[:, :, 0, 0]
        seen["taps swapped"] = _worst(c, x, ws, scale, shift, pix, ch)
    # operands of 10 mantissa bits (fp16 / tf32 class)
    seen["10-bit inputs"] = _worst(c, M.round_mantissa(x, 10), w, scale, shift, pix, ch)
    # scale and shift of channels 0 and 1 exchanged (the plain 1x1 convolution has neither)
    if c.kind != "c1":
        seen["scale/shift exchanged"] = _worst(c, x, w, _swap(scale, 0, 1), _swap(shift, 0, 1), pix, ch)
    # border taps not masked: they read the neighbouring row / image (3x3 only)
    if c.kind == "conv":
        seen["border unmasked"] = _worst(c, x, w, scale, shift, pix, ch, wrap=True)
    print(c.name, {k: round(v, 1) for k, v in seen.items()})
    for what, worst in seen.items():
        assert worst > 1.0, (c.name, what, worst)


# ---- instance coverage through the host plan (no device call) ---------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    return _lib.load()


def host_plan(lib, query):
    q = (C.c_int * 7)(*query)
    out = (C.c_int * 8)()
    rc = lib.unet_host_plan_conv_f32(q, 7, out, 8)
    return rc, list(out)


# Instances and launch shapes the host code cannot select for any shape, by name:
UNREACHABLE = {
    "igemm_f32_kernel<*,*,7,4,*,*>": "run_direct pairs the 224-pixel tile with 64 channels only (224 x 128 accumulators do "
                                     "not fit 256 VGPRs): launch_cfg has no such instance",
    "wino_f32_kernel coGroup 1": "coTiles = nTotal / 32 with nTotal a multiple of 64: always even, so the group is 2, 4 or 8",
    "wino_f32_kernel past wino_fits": "n h w cin >= 2^34 elements fall back to the direct kernel: no device buffer here "
                                      "can hold such an input, the branch is host logic only",
}


def test_case_table_reaches_every_instance(lib):
    direct, wino = set(), []
    for c in M.CASES:
        rc, plan = host_plan(lib, M.plan_query(c))
        assert rc == 0, c.name
        label = M.check_plan(c, plan)          # asserts what the case was written for
        print(f"{c.name}: {label}")
        if plan[0] == 1:
            direct.add((c.kind, 16 if c.cin % 16 == 0 else 4, plan[1], plan[2]))
        else:
            gt, wt = c.n * (c.h // 2), c.w // 2
            wino.append({"tile": (plan[3], plan[4]), "full": gt % plan[3] == 0 and wt % plan[4] == 0, "chunks": c.cin // 16,
                         "grid": plan[5], "cg": plan[6]})
    want = {(kind, ck, ms, ns) for kind in ("conv", "up", "c1") for ck in (4, 16) for ms, ns in ((7, 2), (4, 4), (4, 2))}
    assert direct == want, (want - direct, direct - want)
    assert any(p["tile"] == (16, 8) and p["full"] for p in wino) and any(p["tile"] == (8, 16) and p["full"] for p in wino)
    assert any(not p["full"] for p in wino)
    assert {1, 2, 3, 64} <= {p["chunks"] for p in wino}
    assert {p["cg"] for p in wino} == {2, 4, 8}                       # 1: UNREACHABLE
    assert any(p["grid"] > 8 and p["grid"] % 8 for p in wino)         # the XCD remap's tail
    assert any(c.algo == 1 and host_plan(lib, M.plan_query(c))[1][5] > 8 and host_plan(lib, M.plan_query(c))[1][5] % 8
               for c in M.CASES)                                      # ... and the direct kernel's


def test_winograd_never_groups_one_channel_tile(lib):
    """UNREACHABLE['wino_f32_kernel coGroup 1'], checked: no channel count gives it"""
    for cout in range(4, 1028, 4):
        rc, plan = host_plan(lib, [9, 1, 8, 8, 16, cout, 2])
        assert rc == 0 and plan[0] == 2 and plan[6] in (2, 4, 8), (cout, plan)
    for ms_ns in [(p[1], p[2]) for p in (host_plan(lib, [t, n, h, w, ci, co, 1])[1] for t in (9, 1, 2) for n in (1, 3)
                                         for h in (1, 7, 14, 56) for w in (1, 9, 28, 224) for ci in (4, 16)
                                         for co in (4, 64, 128))]:
        assert ms_ns in ((7, 2), (4, 4), (4, 2)), ms_ns


def test_host_plan_refuses(lib):
    assert host_plan(lib, [9, 1, 4, 4, 4, 4, 2])[0] == 1      # forced Winograd: cin % 16 != 0
    assert host_plan(lib, [9, 1, 3, 4, 16, 4, 2])[0] == 1     # ... odd height
    assert host_plan(lib, [1, 1, 4, 4, 16, 4, 2])[0] == 1     # ... on the transposed convolution
    assert host_plan(lib, [3, 1, 4, 4, 16, 4, 0])[0] == 1 and host_plan(lib, [9, 1, 4, 4, 6, 4, 0])[0] == 1
    q = (C.c_int * 7)(9, 1, 4, 4, 16, 4, 0)
    out = (C.c_int * 8)()
    assert lib.unet_host_plan_conv_f32(q, 6, out, 8) == 1 and lib.unet_host_plan_conv_f32(q, 7, out, 7) == 1
    assert lib.unet_host_plan_conv_f32(None, 7, out, 8) == 1
    # algo 0 follows unet_set_winograd, a forced Winograd does not
    prev = lib.unet_set_winograd(0)
    try:
        assert host_plan(lib, [9, 1, 4, 4, 16, 4, 0])[1][0] == 1 and host_plan(lib, [9, 1, 4, 4, 16, 4, 2])[1][0] == 2
        lib.unet_set_winograd(1)
        assert host_plan(lib, [9, 1, 4, 4, 16, 4, 0])[1][0] == 2 and host_plan(lib, [9, 1, 4, 4, 16, 4, 1])[1][0] == 1
    finally:
        lib.unet_set_winograd(prev)
