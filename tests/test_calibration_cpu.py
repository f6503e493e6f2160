"""Host side of the 'mmse' / 'kl_divergence' calibration (unet_lane_detection_amd/quant.py): the numpy model of the
device histogram's binning rule on elements whose bins can be given by hand, and range_from_histogram against an
independent plain-loop implementation, against 'normal', and on the degenerate histograms.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from unet_lane_detection_amd import quant, state as S

INF, NAN = float("inf"), float("nan")


# ---- histogram_model: the binning rule ----------------------------------------------------------------------------
def test_histogram_model_bins_given_by_hand():
    """span (-1, 3), 64 bins: the bin width 1/16 and every edge are exact in float32, so each bin follows by hand"""
    lo, hi, bins = -1.0, 3.0, 64
    cases = [(-1.0, 0),                 # at lo
             (3.0, 63),                 # at hi: the last bin
             (-5.0, 0), (-1.0000001, 0),        # below the span
             (10.0, 63), (3.0000002, 63),       # above it
             (-1.0 + 1 / 16, 1), (-1.0 + 17 / 16, 17), (-1.0 + 63 / 16, 63),     # on interior edges: the bin that starts there
             # one ulp below an edge: v - lo is exact in [2, 4) and the element stays below; near 1/16 the
             # subtraction's own rounding absorbs the ulp (v + 1 rounds to 17/16) and the element is in the edge's bin
             (np.nextafter(np.float32(-1.0 + 63 / 16), np.float32(0)), 62),
             (np.nextafter(np.float32(-1.0 + 17 / 16), np.float32(0)), 17),
             (0.03, 16), (2.99, 63),
             (INF, 63), (-INF, 0)]
    want = np.zeros(bins + 1, dtype=np.uint64)
    for _, b in cases:
        want[b] += 1
    want[bins] = 3                      # +0.0, -0.0, +0.0: the zero word only (0 sits on the edge of bin 16)
    values = [v for v, _ in cases] + [0.0, -0.0, 0.0, NAN, NAN]
    got = quant.histogram_model(np.array(values, dtype=np.float32), lo, hi, bins)
    assert got.dtype == np.uint64 and got.shape == (bins + 1,)
    assert np.array_equal(got, want), np.nonzero(got != want)
    assert int(got.sum()) == len(values) - 2          # NaN is counted nowhere
    assert quant.zero_bin(lo, hi, bins) == 16


def test_histogram_model_two_roundings():
    """t = (v - lo) * inv, each operation rounded to float32 on its own: an element for which the float64 value of the
    same expression lands in the neighbouring bin"""
    lo, hi, bins = np.float32(0.1), np.float32(0.7), 64
    inv = np.float32(bins) / (hi - lo)
    edges = (float(lo) + np.arange(1, bins) * (float(hi) - float(lo)) / bins).astype(np.float32)
    v = np.concatenate([edges] + [np.nextafter(v, np.float32(s)) for s in (-1, 1) for v in [edges]])
    for _ in range(2):                                     # a few ulps to either side of every interior edge
        v = np.unique(np.concatenate([v, np.nextafter(v, np.float32(-1)), np.nextafter(v, np.float32(1))]))
    t32 = ((v - lo) * inv).astype(np.float32)
    t64 = (v.astype(np.float64) - float(lo)) * (bins / (float(hi) - float(lo)))
    differ = np.nonzero(t32.astype(np.int64) != t64.astype(np.int64))[0]
    assert differ.size, "no element separates float32 from float64 binning: the test shows nothing"
    for i in differ:
        got = quant.histogram_model(v[i:i + 1], lo, hi, bins)
        assert got[int(t32[i])] == 1 and int(got.sum()) == 1, (v[i], t32[i], t64[i])
    want = np.append(np.bincount(t32.astype(np.int64), minlength=bins), 0)
    assert np.array_equal(quant.histogram_model(v, lo, hi, bins), want)


def test_histogram_model_strided_form_skips_pad_channels():
    rng = np.random.default_rng(1)
    x = rng.normal(size=(37, 4)).astype(np.float32)
    x[:, 3] = 8.0                                            # pad channel: would land in the last bin
    got = quant.histogram_model(x, -4.0, 8.0, 64, c=3, ld=4)
    assert np.array_equal(got, quant.histogram_model(x[:, :3].copy(), -4.0, 8.0, 64))
    assert int(got.sum()) == 37 * 3 and got[63] == 0
    assert quant.histogram_model(x, -4.0, 8.0, 64, c=4, ld=4)[63] == 37
    with pytest.raises(ValueError):
        quant.histogram_model(x, -4.0, 8.0, 64, c=5, ld=4)


@pytest.mark.parametrize("lo,hi", [(1.0, 1.0), (2.0, 1.0), (0.0, INF), (NAN, 1.0), (0.0, 1e-44)])
def test_histogram_model_rejects_spans_that_cannot_be_binned(lo, hi):
    with pytest.raises(ValueError):
        quant.histogram_model(np.ones(4, dtype=np.float32), lo, hi, 64)


# ---- range_from_histogram ------------------------------------------------------------------------------------------
def plain_mmse(hist, lo, hi, steps):
    """'mmse' in plain loops, written from the issue's text alone: README quantiser (scale = (max - min) / 255 with 0
    inside, zero point round(-128 - min / scale)), every bin at its centre, the zero word at 0, ties to the wider
    candidate"""
    bins = len(hist) - 1
    lo_w, hi_w = min(lo, 0.0), max(hi, 0.0)
    best = None
    for b in range(1, steps + 1) if hi_w > 0 else [steps]:
        for a in range(1, steps + 1) if lo_w < 0 else [steps]:
            r_min, r_max = a / steps * lo_w, b / steps * hi_w
            scale = (r_max - r_min) / 255.0
            zp = min(max(round(-128 - r_min / scale), -128), 127)
            err = 0.0
            for k in range(bins + 1):
                v = 0.0 if k == bins else lo + (k + 0.5) * (hi - lo) / bins
                q = min(max(round(v / scale) + zp, -128), 127)
                err += int(hist[k]) * ((q - zp) * scale - v) ** 2
            key = (err, -b, -a)
            if best is None or key < best[0]:
                best = (key, (r_min, r_max))
    return best[1], best[0][0]


def skewed_histogram(bins, seed, two_sided):
    """a bulk near 0 with a thin far tail: where clipping pays"""
    rng = np.random.default_rng(seed)
    k = np.arange(bins)
    centre = bins // 3 if two_sided else 0
    h = (4e6 * np.exp(-np.abs(k - centre) / (bins / 16.0))).astype(np.int64) + rng.integers(0, 3, bins)
    return np.append(h, 5000).astype(np.uint64)


@pytest.mark.parametrize("lo,hi,two_sided", [(0.0, 6.0, False), (-2.0, 5.0, True)])
def test_mmse_equals_an_independent_plain_loop(lo, hi, two_sided):
    rng = np.random.default_rng(3)
    hist = np.zeros(65, dtype=np.uint64)                   # a heavy bulk of 16 bins, one far count at either end
    first = 14 if two_sided else 0
    hist[first:first + 16] = rng.integers(500000, 1000000, 16)
    hist[63] = 1
    hist[0] += 1 if two_sided else 0
    hist[64] = 123456
    got = quant.range_from_histogram(hist, lo, hi, "mmse", steps=8)
    want, want_err = plain_mmse(hist, lo, hi, 8)
    assert got == pytest.approx(want, rel=1e-12, abs=0)
    assert quant.mmse_objective(hist, lo, hi, *got) == pytest.approx(want_err, rel=1e-9)
    assert got != (lo, hi), "the histogram was built so that clipping pays"


@pytest.mark.parametrize("seed", range(6))
def test_mmse_is_never_worse_than_normal(seed):
    """the full span is a candidate, so the chosen range cannot lose to it"""
    rng = np.random.default_rng(seed)
    bins = 256
    hist = np.append(rng.integers(0, 1000, bins) * (rng.random(bins) < 0.6), rng.integers(0, 50000)).astype(np.uint64)
    lo, hi = ((0.0, 3.0), (-1.5, 4.0), (-2.0, 0.0))[seed % 3]
    r = quant.range_from_histogram(hist, lo, hi, "mmse", steps=16)
    assert lo <= r[0] <= 0.0 <= r[1] <= hi
    assert quant.mmse_objective(hist, lo, hi, *r) <= quant.mmse_objective(hist, lo, hi, lo, hi)


def test_mmse_clips_one_outlier():
    """a bulk in [0, 1] plus one count at 50: min/max spends 98 % of the codes on one element"""
    bins, lo, hi = 2048, 0.0, 50.0
    hist = np.zeros(bins + 1, dtype=np.uint64)
    hist[:bins // 50] = 1000
    hist[bins - 1] = 1
    hist[bins] = 30000
    r = quant.range_from_histogram(hist, lo, hi, "mmse")
    assert r[0] == 0.0 and r[1] < hi
    assert quant.mmse_objective(hist, lo, hi, *r) < quant.mmse_objective(hist, lo, hi, lo, hi)


@pytest.mark.parametrize("algorithm", ["mmse", "kl_divergence"])
@pytest.mark.parametrize("lo,hi", [(0.0, 4.0), (-1.0, 3.0)])
def test_uniform_histogram_keeps_the_full_span(algorithm, lo, hi):
    hist = np.append(np.full(256, 100), 0).astype(np.uint64)
    assert quant.range_from_histogram(hist, lo, hi, algorithm, steps=16) == (lo, hi)


@pytest.mark.parametrize("algorithm", ["normal", "mmse", "kl_divergence"])
@pytest.mark.parametrize("lo,hi", [(0.0, 2.0), (-3.0, 2.0), (-3.0, 0.0), (0.5, 2.0)])
def test_only_the_zero_word(algorithm, lo, hi):
    """every element an exact zero: any range represents them, the widest is returned and the quantiser accepts it"""
    hist = np.append(np.zeros(256), 12345).astype(np.uint64)
    r = quant.range_from_histogram(hist, lo, hi, algorithm, steps=8)
    if algorithm == "normal":
        assert r == (lo, hi)
    else:
        assert r == (min(lo, 0.0), max(hi, 0.0))
    scale, zp = quant.affine_params(*r)
    assert math.isfinite(scale) and scale > 0 and -128 <= zp <= 127
    assert quant.dequantize(quant.quantize(0.0, scale, zp), scale, zp) == 0.0


def test_ties_go_to_the_wider_candidate():
    """an empty histogram scores every candidate alike; so does 'kl_divergence' when no candidate keeps 128 bins"""
    empty = np.zeros(257, dtype=np.uint64)
    for algorithm in ("mmse", "kl_divergence"):
        assert quant.range_from_histogram(empty, -1.0, 2.0, algorithm, steps=8) == (-1.0, 2.0)
    assert quant.range_from_histogram(skewed_histogram(64, 0, True), -1.0, 2.0, "kl_divergence", steps=8) == (-1.0, 2.0)
    # larger b before larger a: all the mass in one bin next to 0 of a symmetric span.  No candidate clips it, so its
    # error depends on the scale alone, that is on a + b (quarters: exact), and every pair with the best sum ties
    hist = np.zeros(257, dtype=np.uint64)
    hist[130] = 10
    got = quant.range_from_histogram(hist, -1.0, 1.0, "mmse", steps=4)
    want, err = plain_mmse(hist, -1.0, 1.0, 4)
    assert got == want
    a, b = round(-got[0] * 4), round(got[1] * 4)
    tied = [(i, j) for i in range(1, 5) for j in range(1, 5) if i + j == a + b]
    assert len(tied) > 1, "no tie among the candidates: the test shows nothing"
    for i, j in tied:
        assert quant.mmse_objective(hist, -1.0, 1.0, -i / 4, j / 4) == err
    assert (b, a) == max((j, i) for i, j in tied)


def test_kl_divergence_clips_a_thin_tail_and_stays_inside():
    hist = skewed_histogram(2048, 5, False)
    hist[1500:2048] = 0
    hist[2047] = 1
    r = quant.range_from_histogram(hist, 0.0, 8.0, "kl_divergence")
    assert r[0] == 0.0 and 0.5 <= r[1] < 8.0            # at least 128 of 2048 bins kept: r_max >= 0.5
    two = quant.range_from_histogram(skewed_histogram(512, 6, True), -2.0, 4.0, "kl_divergence", steps=16)
    assert -2.0 <= two[0] <= 0.0 <= two[1] <= 4.0


def test_kl_divergence_charges_for_clipping():
    """2048 bins, a smooth bulk that fills the whole span: the candidate that keeps 256 bins has one bin per int8 code,
    so a Q built from P itself would equal P there (KL = 0) and an eighth of the span would win.  Q is built from the
    kept counts: cutting 7/8 of a span that holds mass everywhere must lose to the full span"""
    k = np.arange(2048)
    hist = np.append((1e6 * np.exp(-k / 700.0)).astype(np.int64), 10 ** 6).astype(np.uint64)
    r = quant.range_from_histogram(hist, 0.0, 16.0, "kl_divergence")
    assert r[0] == 0.0 and r[1] > 8.0, r
    two = quant.range_from_histogram(np.append(hist[1023::-1], hist[:1025]).astype(np.uint64), -8.0, 8.0, "kl_divergence", steps=16)
    assert two[1] - two[0] > 8.0, two


def test_unknown_algorithm():
    with pytest.raises(ValueError):
        quant.range_from_histogram(np.zeros(65, dtype=np.uint64), 0.0, 1.0, "percentile")


def test_quantize_model_accepts_the_chosen_ranges():
    feats = [8, 16]
    sd = S.seeded_state_dict(feats, seed=0)
    names = quant.tensor_names(len(feats))
    assert len(quant.tensor_shapes(feats)) == len(names)
    assert quant.tensor_shapes(feats) == [(3, 0), (8, 0), (16, 0), (16, 1), (32, 1), (32, 2), (32, 2), (16, 1), (16, 1),
                                          (8, 0), (8, 0)]
    for algorithm in ("mmse", "kl_divergence"):
        ranges = {}
        for i, name in enumerate(names):
            two_sided = name == "input" or name.startswith("cat")
            lo, hi = (-2.0, 2.5) if two_sided else (0.0, 3.0 + i)
            ranges[name] = quant.range_from_histogram(skewed_histogram(256, i, two_sided), lo, hi, algorithm, steps=8)
        qm = quant.quantize_model(sd, ranges)
        assert np.isfinite(qm["input.scale"]) and qm["input.lut"].shape == (3, 256)
        for k, v in qm.items():
            if k.endswith(".mult"):
                assert np.all(np.isfinite(v)) and np.all(v > 0), k


# ---- compare_outputs: the verdict ------------------------------------------------------------------------------------
def test_output_comparison_grades():
    """reference README.md:3557-3562: mean < 0.05 GOOD, < 0.10 ACCEPTABLE, else POOR"""
    from unet_lane_detection_amd.int8 import OutputComparison
    for per_frame, grade in (([0.0], "GOOD"), ([0.01, 0.0899], "GOOD"), ([0.05], "ACCEPTABLE"), ([0.0, 0.1999], "ACCEPTABLE"),
                             ([0.10], "POOR"), ([0.9, 0.0], "POOR")):
        r = OutputComparison(per_frame)
        assert r.grade == grade, (per_frame, r)
        assert r.mean == pytest.approx(np.mean(per_frame)) and r.max == max(per_frame)
    with pytest.raises(ValueError):
        OutputComparison([])


# ---- the entry points' own checks (no device is touched) --------------------------------------------------------------
def test_histogram_entry_points_refuse_bad_arguments():
    from unet_lane_detection_amd import _lib
    lib = _lib.load()
    f = (C.c_float * 64)()
    w = (C.c_uint64 * 4097)()
    x, hist = C.cast(f, C.c_void_p), C.cast(w, C.c_void_p)

    def op(x=x, npix=4, c=3, ld=4, lo=0.0, hi=1.0, bins=64, hist=hist):
        return lib.unet_op_histogram_f32(0, x, npix, c, ld, lo, hi, bins, hist, None)
    assert op(hi=0.0) == 1 and op(lo=1.0, hi=0.5) == 1                       # hi <= lo
    assert op(hi=INF) == 1 and op(lo=-INF) == 1 and op(hi=NAN) == 1 and op(lo=-3e38, hi=3e38) == 1   # span not finite
    assert op(hi=1e-44) == 1                                                 # bins / span overflows
    assert op(bins=32) == 1 and op(bins=8192) == 1 and op(bins=100) == 1 and op(bins=0) == 1
    assert op(c=5, ld=4) == 1 and op(c=0) == 1
    assert op(x=None) == 1 and op(hist=None) == 1
    assert lib.unet_op_last_error().startswith(b"invalid argument")
    assert lib.unet_prob_mae_accumulate(0, None, x, 1, 4, hist, None) == 1
    assert lib.unet_prob_mae_accumulate(0, x, x, 0, 4, hist, None) == 1
    assert lib.unet_forward_u8_histograms(None, x, 1, 8, 8, x, 64, hist, None) == 1
