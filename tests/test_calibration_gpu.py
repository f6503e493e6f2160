"""Histogram calibration on the GPU: the histogram kernel against its numpy model word for word
(unet_op_histogram_f32 / quant.histogram_model), the histogram pass of the network against the float oracle's
activations, 'mmse' / 'kl_divergence' end to end - their narrower ranges drive the saturating clamps of the int8
kernels, which must stay bit-exact against the integer oracle - and compare_outputs against numpy."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import int8_oracle as Q
from oracle import unet_oracle as O
from unet_lane_detection_amd import quant, state as S

pytestmark = pytest.mark.gpu

FEATS_B = [32, 64, 128]
HIST_MAX_GRID = 1024            # csrc/calib_kernels.h: blocks of one histogram launch at the most
SPANS = {"one-sided": (0.0, 6.0), "two-sided": (-1.7, 4.1)}


@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    return _lib.load()


def device_histogram(lib, x, npix, c, ld, lo, hi, bins, hist=None, offset=0):
    """x: float32 numpy array of npix * ld floats -> the device's words as uint64 (added to `hist` if given)"""
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).reshape(-1)).cuda()
    if hist is None:
        hist = torch.zeros(bins + 1, dtype=torch.int64, device="cuda")
    rc = lib.unet_op_histogram_f32(0, C.c_void_p(xd.data_ptr() + 4 * offset), npix, c, ld, lo, hi, bins,
                                   C.c_void_p(hist.data_ptr()), None)
    assert rc == 0, (rc, lib.unet_op_last_error())
    return hist.cpu().numpy().view(np.uint64), hist


def mixed_data(npix, c, ld, lo, hi, bins, seed):
    """half exact zeros; values inside and beyond the span; lo, hi, the interior bin edges, +-0, NaN and +-inf"""
    rng = np.random.default_rng(seed)
    span = hi - lo
    x = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, (npix, ld)).astype(np.float32)
    x[rng.random((npix, ld)) < 0.5] = 0.0
    edges = (np.float32(lo) + np.arange(bins + 1, dtype=np.float32) * np.float32(span / bins)).astype(np.float32)
    special = np.concatenate([edges, [lo, hi, 0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, lo - 3 * span, hi + 3 * span]])
    flat = x[:, :c].reshape(-1)
    k = min(special.size, flat.size)
    pos = rng.choice(flat.size, k, replace=False)
    flat[pos] = special[rng.permutation(special.size)[:k]].astype(np.float32)
    x[:, :c] = flat.reshape(npix, c)
    return x


# ---- the kernel on its own ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", sorted(SPANS))
@pytest.mark.parametrize("bins", [64, 256, 2048])
@pytest.mark.parametrize("npix,c,ld", [(1, 1, 1), (257, 3, 4), (256 * (HIST_MAX_GRID + 1) + 1, 24, 48)])
def test_histogram_op_matches_the_model(lib, npix, c, ld, bins, span):
    lo, hi = SPANS[span]
    if (npix, c, ld) == (1, 1, 1):
        x = np.array([[0.37 * hi]], dtype=np.float32)
    elif (c, ld) == (3, 4):
        # the pad channel holds hi: counted in error it lands in the last bin, which the data (below hi / 2) leaves empty
        rng = np.random.default_rng(bins)
        x = rng.uniform(lo, hi / 2, (npix, ld)).astype(np.float32)
        x[rng.random((npix, ld)) < 0.5] = 0.0
        x[::7, 1] = np.nan
        x[:, 3] = hi
    else:
        x = mixed_data(npix, c, ld, lo, hi, bins, seed=bins)     # more elements than grid x 256 threads: the loop wraps
        assert npix * c > HIST_MAX_GRID * 256
    want = quant.histogram_model(x, lo, hi, bins, c=c, ld=ld)
    got, hist = device_histogram(lib, x, npix, c, ld, lo, hi, bins)
    assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
    assert int(got.sum()) == npix * c - int(np.isnan(x[:, :c]).sum())
    if (c, ld) == (3, 4):
        assert got[bins - 1] == 0
    # the kernel accumulates: a second call into the same words doubles every one of them
    again, _ = device_histogram(lib, x, npix, c, ld, lo, hi, bins, hist=hist)
    assert np.array_equal(again, 2 * want)


@pytest.mark.parametrize("offset", [0, 1])
def test_histogram_op_dense_paths(lib, offset):
    """c == ld: 16-byte loads with the last total % 4 elements one by one, and single loads when the tensor is not
    aligned for them; more than 1024 blocks' worth, so both loops wrap"""
    lo, hi, bins = -1.7, 4.1, 256
    n = 4 * 1024 * HIST_MAX_GRID + 3
    x = mixed_data(n + offset, 1, 1, lo, hi, bins, seed=11 + offset).reshape(-1)
    want = quant.histogram_model(x[offset:], lo, hi, bins)
    got, _ = device_histogram(lib, x, n, 1, 1, lo, hi, bins, offset=offset)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


def test_histogram_op_zeros_stay_out_of_the_bins(lib):
    """2^16 + 4463 exact zeros and a single other element: one word each"""
    x = np.zeros(70000, dtype=np.float32)
    x[1::2] = -0.0
    x[12345] = 2.5
    for lo, hi in SPANS.values():
        got, _ = device_histogram(lib, x, x.size, 1, 1, lo, hi, 256)
        assert got[256] == 69999 and int(got[:256].sum()) == 1
        assert np.array_equal(got, quant.histogram_model(x, lo, hi, 256))


def test_histogram_op_refuses_bad_arguments_and_launches_nothing(lib):
    x = torch.ones(64, device="cuda")
    hist = torch.zeros(4097, dtype=torch.int64, device="cuda")
    xp, hp = C.c_void_p(x.data_ptr()), C.c_void_p(hist.data_ptr())
    inf, nan = float("inf"), float("nan")

    def op(x=xp, npix=16, c=3, ld=4, lo=0.0, hi=2.0, bins=64, hist=hp):
        return lib.unet_op_histogram_f32(0, x, npix, c, ld, lo, hi, bins, hist, None)
    for bad in (dict(hi=0.0), dict(lo=2.0, hi=1.0), dict(hi=inf), dict(lo=-inf), dict(hi=nan), dict(lo=-3e38, hi=3e38),
                dict(hi=1e-44), dict(bins=32), dict(bins=8192), dict(bins=96), dict(c=5), dict(x=None), dict(hist=None)):
        assert op(**bad) == 1, bad
    torch.cuda.synchronize()
    assert int(hist.abs().sum()) == 0
    assert op() == 0 and int(hist.sum()) == 48


# ---- the histogram pass of the network --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_b():
    """float model B on the data of the int8 suite (ragged last batch), calibrated by every algorithm at 256 bins"""
    from unet_lane_detection_amd.int8 import calibrate
    from unet_lane_detection_amd.model import UNetHIP
    sdn = S.seeded_state_dict(FEATS_B, seed=0)
    fm = UNetHIP(sdn, device=0)
    calib = S.synthetic_frames(6, 64, 64, seed=1)
    frames = torch.from_numpy(calib)
    out = {"sd": sdn, "fm": fm, "calib": calib, "default": calibrate(fm, frames, batch=4),
           "normal": calibrate(fm, frames, batch=4, algorithm="normal")}
    out["mmse"], out["hists"] = calibrate(fm, frames, batch=4, algorithm="mmse", bins=256, return_histograms=True)
    out["kl_divergence"] = calibrate(fm, frames, batch=4, algorithm="kl_divergence", bins=256)
    yield out
    fm.release()


@pytest.fixture(scope="module")
def oracle_activations(model_b):
    """the float oracle's tensors on the calibration frames, named as quant.tensor_names (the ones the oracle taps)"""
    sd = O.to_torch_state(model_b["sd"])
    d = len(FEATS_B)
    taps = {}
    x = O.normalize_u8_nhwc(model_b["calib"])
    with torch.no_grad():
        O.forward(sd, x, taps=taps)
    acts = {"input": x.numpy(), "bott.b": taps["bottleneck"].numpy()}
    for l in range(d):
        acts[f"cat{l}"] = np.concatenate([taps[f"enc{l}"].numpy(), taps[f"up{d - 1 - l}"].numpy()], axis=1)
    for j in range(d):
        acts[f"dec{j}.b"] = taps[f"dec{j}"].numpy()
    return acts


def test_network_histograms_count_every_element(model_b):
    names = quant.tensor_names(len(FEATS_B))
    hists = model_b["hists"]
    assert list(hists) == names
    n, h, w = model_b["calib"].shape[:3]
    for name, (c, level) in zip(names, quant.tensor_shapes(FEATS_B)):
        hist, lo, hi = hists[name]
        assert hist.shape == (257,) and hist.dtype == np.uint64
        assert int(hist.sum()) == n * (h >> level) * (w >> level) * c, name
        assert hist[255] > 0, f"{name}: the maximum of the range pass must land in the last bin"
        assert (lo, hi) == (min(model_b["normal"][name][0], 0.0), max(model_b["normal"][name][1], 0.0))


def test_network_histograms_match_the_float_oracle(model_b, oracle_activations):
    """|CDF_device - CDF_oracle| at every interior bin edge is at most the number of oracle elements within
    1e-4 span + 1e-5 of that edge, the agreement test_device_calibration_matches_float_oracle holds the two tiers to;
    few enough elements are that near an edge (<= 6 % per tensor) for the bound to say something"""
    bins = 256
    assert set(oracle_activations) == {"input", "bott.b", "cat0", "cat1", "cat2", "dec0.b", "dec1.b", "dec2.b"}
    for name, act in oracle_activations.items():
        dev, lo, hi = model_b["hists"][name]
        ref = quant.histogram_model(act, lo, hi, bins)
        assert int(ref.sum()) == int(dev.sum()) == act.size, name
        zb = quant.zero_bin(lo, hi, bins)
        fold = lambda h: np.cumsum(h[:bins].astype(np.int64) + np.eye(1, bins, zb, dtype=np.int64)[0] * int(h[bins]))
        cdf_dev, cdf_ref = fold(dev), fold(ref)
        tol = 1e-4 * (hi - lo) + 1e-5
        edges = lo + np.arange(1, bins) * (hi - lo) / bins
        v = np.sort(act.reshape(-1).astype(np.float64))
        near = np.searchsorted(v, edges + tol, side="right") - np.searchsorted(v, edges - tol, side="left")
        share = near.sum() / act.size
        diff = np.abs(cdf_dev[:bins - 1] - cdf_ref[:bins - 1])
        print(f"{name}: near-edge share {share:.4f}, max |dCDF| {diff.max()}, max allowed there {near[diff.argmax()]}")
        assert share <= 0.06, (name, share)
        worst = int(np.argmax(diff - near))
        assert np.all(diff <= near), (name, worst + 1, int(diff[worst]), int(near[worst]))


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_normal_is_the_default(model_b):
    assert model_b["normal"] == model_b["default"]


@pytest.mark.parametrize("algorithm", ["mmse", "kl_divergence"])
def test_chosen_ranges_lie_inside_minmax(model_b, algorithm):
    ranges, normal = model_b[algorithm], model_b["normal"]
    assert list(ranges) == list(normal)
    for k in normal:
        assert normal[k][0] <= ranges[k][0] <= 0.0 <= ranges[k][1] <= normal[k][1], (k, ranges[k], normal[k])
    print(algorithm, {k: (round(ranges[k][0] / normal[k][0], 3) if normal[k][0] else 1.0,
                          round(ranges[k][1] / normal[k][1], 3)) for k in normal})


@pytest.mark.parametrize("algorithm", ["mmse", "kl_divergence"])
def test_int8_forward_stays_bit_exact_under_clipping_ranges(model_b, algorithm):
    from unet_lane_detection_amd.int8 import UNetInt8
    qm = quant.quantize_model(model_b["sd"], model_b[algorithm])
    n, h, w = 2, 64, 64
    frames = S.synthetic_frames(n, h, w, seed=3)
    taps = {}
    ref = Q.forward(qm, frames, taps=taps)
    net = UNetInt8(qm, device=0)
    logits = net.run_u8(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    d = len(FEATS_B)
    checks = []
    for l in range(d):
        checks += [(f"enc{l}.a", taps[f"encoder_blocks.{l}.0"], l),
                   (f"cat{l}.pool", Q.maxpool2x2(taps[f"encoder_blocks.{l}.3"]), l + 1)]
    checks += [("bott.a", taps["bottleneck.0"], d), ("bott.b", taps["bottleneck.3"], d)]
    for j in range(d):
        l = d - 1 - j
        cat = np.concatenate([taps[f"encoder_blocks.{l}.3"], taps[f"decoder_blocks.{2 * j}"]], axis=1)
        checks += [(f"cat{l}", cat, l), (f"dec{j}.a", taps[f"decoder_blocks.{2 * j + 1}.0"], l),
                   (f"dec{j}.b", taps[f"decoder_blocks.{2 * j + 1}.3"], l)]
    saturated = 0
    for name, want, level in checks:
        got = net.read_tensor(name, n, h >> level, w >> level)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {want.size} int8 values differ"
        saturated += int((want == 127).sum())
    assert np.array_equal(logits.cpu().numpy(), ref)
    print(f"{algorithm}: {saturated} activations at the upper clamp")
    net.release()


def test_calibrate_names_the_tensor_that_holds_nan(model_b):
    from unet_lane_detection_amd.int8 import calibrate
    from unet_lane_detection_amd.model import UNetHIP
    sd = dict(model_b["sd"])
    bias = np.array(sd["decoder_blocks.4.bias"], dtype=np.float32)      # the last transposed conv: no ReLU behind it,
    bias[3] = np.nan                                                    # so one channel of cat0's upper half is NaN
    sd["decoder_blocks.4.bias"] = bias
    fm = UNetHIP(sd, device=0)
    try:
        with pytest.raises(ValueError, match="cat0"):
            calibrate(fm, torch.from_numpy(model_b["calib"][:2]), algorithm="mmse", bins=256)
        with pytest.raises(ValueError):
            calibrate(fm, torch.from_numpy(model_b["calib"][:2]), algorithm="percentile")
    finally:
        fm.release()


# ---- compare_outputs -------------------------------------------------------------------------------------------------
def test_compare_outputs_against_numpy(model_b):
    from unet_lane_detection_amd.int8 import UNetInt8, compare_outputs
    net = UNetInt8(quant.quantize_model(model_b["sd"], model_b["mmse"]), device=0)
    frames = torch.from_numpy(S.synthetic_frames(3, 32, 32, seed=21))
    r = compare_outputs(model_b["fm"], net, frames, batch=2)              # ragged last batch
    _, pf = model_b["fm"].run_u8(frames.cuda(), return_probs=True)
    _, pq = net.run_u8(frames.cuda(), return_probs=True)
    want = np.abs(pf.cpu().numpy() - pq.cpu().numpy()).astype(np.float64).reshape(3, -1).mean(axis=1)
    assert r.per_frame.shape == (3,) and np.all(want > 0)
    np.testing.assert_allclose(r.per_frame, want, rtol=1e-10, atol=0)
    assert r.mean == pytest.approx(want.mean(), rel=1e-10) and r.max == pytest.approx(want.max(), rel=1e-10)
    assert r.grade == ("GOOD" if want.mean() < 0.05 else "ACCEPTABLE" if want.mean() < 0.10 else "POOR")
    print(r)
    net.release()


def test_prob_mae_on_constructed_inputs():
    """the sums on the device, frame by frame, and the verdict's boundaries (reference README.md:3557-3562)"""
    from unet_lane_detection_amd.int8 import OutputComparison, prob_mae
    rng = np.random.default_rng(5)
    a = rng.random((4, 1, 24, 40)).astype(np.float32)
    b = a.copy()
    b[0] += np.float32(0.03)
    b[1] -= np.float32(0.07)
    b[2, 0, :12] += np.float32(0.5)
    got = prob_mae(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
    want = np.abs(a - b).astype(np.float64).reshape(4, -1).mean(axis=1)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
    assert got[3] == 0.0
    assert [OutputComparison(got[i:i + 1]).grade for i in range(3)] == ["GOOD", "ACCEPTABLE", "POOR"]
    with pytest.raises(ValueError):
        prob_mae(torch.from_numpy(a).cuda(), torch.from_numpy(b[:2]).cuda())
