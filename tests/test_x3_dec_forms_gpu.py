"""The two block tiles of the f16x3 tier's composed decoder step (csrc/conv_x3_dec.h, unet_set_x3_dec_form): the
64-channel form (one output parity per wave) and the 128-channel form (a row parity and both column parities per wave).
Both add every accumulator's terms in the same order - the skip's chunks tap by tap, then x's - from the same packed
weights, so they must agree bit for bit; the 128-channel form is also held to the CPU oracle at the bound
tests/test_x3_compose_gpu.py uses (2e-5 of the output's range)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from unet_lane_detection_amd import state as S

pytestmark = pytest.mark.gpu

ORACLE_TOL = 2e-5


def _p(t):
    return C.c_void_p(t.data_ptr())


def _h(a):
    a = np.ascontiguousarray(a.numpy(), dtype=np.float32)
    return a, C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    return _lib.load(build_if_missing=False)


class _Form:
    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        self.prev = self.lib.unet_set_x3_dec_form(self.mode)

    def __exit__(self, *exc):
        self.lib.unet_set_x3_dec_form(self.prev)


def _make(n, h, w, f, bias_scale=4.0, amp=1.0):
    g = torch.Generator().manual_seed(n * 1000 + h * 7 + w + f)
    wt = torch.randn(2 * f, f, 2, 2, generator=g) * (1.0 / (2 * f)) ** 0.5
    bt = torch.randn(f, generator=g) * bias_scale           # a non-zero transposed-convolution bias
    w3 = torch.randn(f, 2 * f, 3, 3, generator=g) * (2.0 / (18 * f)) ** 0.5
    scale = torch.rand(f, generator=g) + 0.5
    shift = torch.randn(f, generator=g) * 0.3
    skip = torch.randn(n, f, h, w, generator=g) * amp
    x = torch.randn(n, 2 * f, h // 2, w // 2, generator=g) * amp
    return dict(n=n, h=h, w=w, f=f, wt=wt, bt=bt, w3=w3, scale=scale, shift=shift, skip=skip, x=x)


_CASES = {}


def _case(key, **kw):
    """Inputs, parameters and the oracle's pre-activation output of one shape: made once, shared, never written to."""
    shape, key = key, key + tuple(sorted(kw.items()))
    if key not in _CASES:
        c = _make(*shape, **kw)
        up = O.upconv2x2(c["x"], c["wt"], c["bt"])
        pre = O.conv3x3(torch.cat([c["skip"], up], 1), c["w3"]) * c["scale"][None, :, None, None] + \
            c["shift"][None, :, None, None]
        c["ref"] = {0: pre.permute(0, 2, 3, 1).contiguous(), 1: torch.relu(pre).permute(0, 2, 3, 1).contiguous()}
        c["skip_dev"] = c["skip"].permute(0, 2, 3, 1).contiguous().cuda()
        c["x_dev"] = c["x"].permute(0, 2, 3, 1).contiguous().cuda()
        _CASES[key] = c
    return _CASES[key]


def _run(lib, c, relu, form):
    n, h, w, f = c["n"], c["h"], c["w"], c["f"]
    y = torch.full((n, h, w, f), float("nan"), device="cuda")
    keep = [_h(c[k]) for k in ("wt", "bt", "w3", "scale", "shift")]
    with _Form(lib, form):
        rc = lib.unet_op_upcat_conv3x3_x3(0, _p(c["skip_dev"]), _p(c["x_dev"]), n, h, w, f, *[k[1] for k in keep], relu,
                                          _p(y), None)
    assert rc == 0
    return y


# (n, h, w) at f = 128: one tile touching all four borders; 2 x 2 tiles; a ragged bottom (the second tile holds two
# rows); 12 items of the 128-channel form on a grid of 8 - some blocks run two items, some one (the cross-item prefetch)
SHAPES = [(2, 16, 28), (2, 32, 56), (1, 18, 28), (3, 32, 56)]


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_forms_bit_identical(lib, n, h, w):
    c = _case((n, h, w, 128))
    for relu in (1, 0):
        y1 = _run(lib, c, relu, 1)
        y2 = _run(lib, c, relu, 2)
        assert not torch.isnan(y2).any()
        assert torch.equal(y1, y2), (relu, (y1 - y2).abs().max().item())


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_form2_vs_oracle(lib, n, h, w):
    c = _case((n, h, w, 128))
    for relu in (1, 0):
        ref = c["ref"][relu]
        y = _run(lib, c, relu, 2).cpu()
        rng = ref.abs().max().item()
        err = (y - ref).abs().max().item()
        print(f"form 2 {n}x{h}x{w} relu={relu}: err {err:.3e} range {rng:.3e}")
        assert err <= ORACLE_TOL * rng, (relu, err, rng)


def test_form2_border_classes_matter(lib):
    """A transposed-convolution bias large against the rest: the nine border classes really differ, and the
    128-channel form's epilogue adds the right one to both of a wave's column parities."""
    c = _case((1, 16, 28, 128), bias_scale=50.0, amp=0.01)
    ref = c["ref"][0]
    y = _run(lib, c, 0, 2).cpu()
    assert (y - ref).abs().max().item() <= ORACLE_TOL * ref.abs().max().item()
    assert (ref[0, 0, 0] - ref[0, 5, 5]).abs().max().item() > 1e-2 * ref.abs().max().item()


@pytest.mark.parametrize("n,h,w,relu", [(1, 16, 28, 1), (1, 32, 28, 0)])
def test_two_channel_groups(lib, n, h, w, relu):
    """f = 256 (the operator entry point only): two channel groups of the 128-channel form per pixel tile, four of the
    64-channel form - the channel-group indexing of the weights, the constants and the stores."""
    c = _case((n, h, w, 256))
    ref = c["ref"][relu]
    y2 = _run(lib, c, relu, 2)
    rng = ref.abs().max().item()
    err = (y2.cpu() - ref).abs().max().item()
    print(f"form 2 f=256 {n}x{h}x{w} relu={relu}: err {err:.3e} range {rng:.3e}")
    assert err <= ORACLE_TOL * rng, (err, rng)
    assert torch.equal(_run(lib, c, relu, 1), y2)


def test_switch_returns_previous_and_clamps(lib):
    prev = lib.unet_set_x3_dec_form(2)
    try:
        assert lib.unet_set_x3_dec_form(1) == 2
        assert lib.unet_set_x3_dec_form(7) == 1      # anything but 1 and 2: automatic
        assert lib.unet_set_x3_dec_form(-1) == -1
    finally:
        lib.unet_set_x3_dec_form(prev)


@pytest.fixture(scope="module")
def modelA():
    from unet_lane_detection_amd.model import UNetHIP
    m = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    yield m
    m.release()


def test_path_taken_and_logits_bit_identical(lib, modelA):
    """Model A, batch 2 at 224 x 224 (the work-item rule lifted, as in the graph test of tests/test_x3_compose_gpu.py):
    both covered levels run the composed kernel under its one profiler label whatever the form, and the logits do not
    depend on the form."""
    frames = torch.from_numpy(S.synthetic_frames(2, seed=0)).cuda().contiguous()
    prev = lib.unet_set_x3_compose(1)
    try:
        with _Form(lib, -1):
            modelA.profile(True)
            auto = modelA.run_u8(frames, precision="f16x3").clone()
            recs = modelA.profile_records()
            modelA.profile(False)
            assert modelA.device_error() == 0
        with _Form(lib, 1):
            one = modelA.run_u8(frames, precision="f16x3").clone()
            assert modelA.device_error() == 0
        with _Form(lib, 2):
            two = modelA.run_u8(frames, precision="f16x3").clone()
            assert modelA.device_error() == 0
    finally:
        lib.unet_set_x3_compose(prev)
    names = [r[0] for r in recs]
    assert names.count("upcat_conv3x3_dec_f16x3") == 2, names
    assert torch.equal(auto, one)
    assert torch.equal(two, one)


def test_graph_replay_form2_equals_direct_launches(lib, modelA):
    frames = torch.from_numpy(S.synthetic_frames(4, seed=3)).cuda().contiguous()
    prev = lib.unet_set_x3_compose(1)
    try:
        with _Form(lib, 2):
            direct = modelA.run_u8(frames, precision="f16x3").clone()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                modelA.run_u8(frames, precision="f16x3")                  # warm: workspace at this shape
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = modelA.run_u8(frames, precision="f16x3")
        with _Form(lib, 1):                                               # the graph keeps the form it was captured with
            graph.replay()
            torch.cuda.synchronize()
        assert modelA.device_error() == 0
    finally:
        lib.unet_set_x3_compose(prev)
    assert torch.equal(out, direct)
