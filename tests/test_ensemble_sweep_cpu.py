"""Host side of the checkpoint ensemble and the threshold sweep: the numpy models (metrics.sweep_model,
ensemble.combine_model), metrics.ThresholdSweep, and the argument checks of the two entry points, which refuse before a
device is touched.  No kernel runs here; tests/test_ensemble_sweep_gpu.py holds the kernels to these models."""
import ctypes as C

import numpy as np
import pytest

from unet_lane_detection_amd import _lib, ensemble as E, metrics as M

INF, NAN = np.float32(np.inf), np.float32(np.nan)


def brute(scores, targets, t):
    with np.errstate(invalid="ignore"):
        pred = np.asarray(scores, dtype=np.float32) > np.float32(t)
    truth = np.asarray(targets) != 0
    return (int((pred & truth).sum()), int((pred & ~truth).sum()), int((~pred & truth).sum()),
            int((~pred & ~truth).sum()))


def edge_scores(rng, n, thresholds):
    """random scores with every finite threshold, NaN and both infinities planted"""
    s = rng.random(n).astype(np.float32)
    plant = [t for t in thresholds if np.isfinite(t)] + [NAN, INF, -INF, np.float32(0.0), np.float32(1.0)]
    pos = rng.choice(n, size=2 * len(plant), replace=False)
    s[pos] = np.array(plant + plant, dtype=np.float32)
    return s


@pytest.mark.parametrize("thresholds", [
    np.array(M.DEFAULT_THRESHOLDS, dtype=np.float32),
    np.array([0.5], dtype=np.float32),
    np.array([-np.inf, 0.25, 0.5, np.inf], dtype=np.float32),
    np.array([-np.inf, np.inf], dtype=np.float32),
])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_sweep_counts_against_brute_force(thresholds, dtype):
    rng = np.random.default_rng(len(thresholds))
    s = edge_scores(rng, 997, thresholds)
    truth = rng.random(s.size) < 0.3
    t = truth.astype(np.float32) if dtype == np.float32 else np.where(truth, rng.choice([1, 255], s.size), 0).astype(np.uint8)
    counts = M.sweep_model(s, t, thresholds)
    assert counts.shape == (2, len(thresholds) + 1) and counts.dtype == np.int64 and counts.sum() == s.size
    assert counts[1].sum() == truth.sum()
    sw = M.ThresholdSweep(thresholds, counts, "probability")
    for j, tj in enumerate(thresholds):
        assert (sw.tp[j], sw.fp[j], sw.fn[j], sw.tn[j]) == brute(s, t, tj), (j, tj)
    assert sw.tp.dtype == np.int64 and sw.pixels == s.size
    # -inf is below everything but NaN and -inf itself; nothing is above +inf
    if thresholds[0] == -np.inf:
        assert sw.fn[0] + sw.tn[0] == 4                       # the planted NaN and -inf, two of each
    if thresholds[-1] == np.inf:
        assert sw.tp[-1] + sw.fp[-1] == 0


def test_sweep_metrics_follow_segmetrics():
    rng = np.random.default_rng(3)
    s = rng.random(4096).astype(np.float32)
    t = (rng.random(4096) < 0.2).astype(np.float32)
    th = np.array(M.DEFAULT_THRESHOLDS, dtype=np.float32)
    sw = M.ThresholdSweep(th, M.sweep_model(s, t, th))
    for j in range(len(th)):
        acc = np.zeros(M.NUM_ACCUMULATORS)
        acc[M.TP:M.TN + 1] = sw.tp[j], sw.fp[j], sw.fn[j], sw.tn[j]
        one = M.SegMetrics(acc)
        for k in ("iou", "precision", "recall", "f1", "pixel_accuracy"):
            assert getattr(sw, k)[j] == getattr(one, k), (k, j)
        at = sw.at(M.DEFAULT_THRESHOLDS[j])
        assert at["tp"] == one.tp and at["tn"] == one.tn and at["f1"] == one.f1 and at["iou"] == one.iou
    assert np.array_equal(sw.dice, sw.f1)
    with pytest.raises(KeyError):
        sw.at(0.123)


def test_sweep_empty_denominators_give_one():
    th = np.array([0.25, 0.5, 0.75], dtype=np.float32)
    # no positive target and nothing predicted at any threshold
    sw = M.ThresholdSweep(th, M.sweep_model(np.zeros(10, np.float32), np.zeros(10, np.float32), th))
    for k in ("iou", "precision", "recall", "f1", "pixel_accuracy"):
        assert np.array_equal(getattr(sw, k), np.ones(3)), k
    # no element at all: every ratio is empty
    sw = M.ThresholdSweep(th, np.zeros((2, 4), dtype=np.int64))
    assert np.array_equal(sw.pixel_accuracy, np.ones(3)) and np.array_equal(sw.iou, np.ones(3))
    # positives that are never predicted: recall 0, precision empty = 1
    sw = M.ThresholdSweep(th, M.sweep_model(np.zeros(4, np.float32), np.ones(4, np.float32), th))
    assert np.array_equal(sw.recall, np.zeros(3)) and np.array_equal(sw.precision, np.ones(3))


def test_best_and_its_ties():
    th = np.array([0.2, 0.4, 0.6, 0.8], dtype=np.float32)
    # every positive scores 0.9 and every negative 0.1: all four thresholds separate them perfectly - a four-way tie;
    # 0.4 and 0.6 are equally near 0.5 (0.5 - 0.4 == 0.6 - 0.5 in float64), the lower one wins
    s = np.array([0.9] * 5 + [0.1] * 20, dtype=np.float32)
    t = np.array([1] * 5 + [0] * 20, dtype=np.float32)
    sw = M.ThresholdSweep(th, M.sweep_model(s, t, th), probabilities=[0.2, 0.4, 0.6, 0.8])
    assert np.array_equal(sw.f1, np.ones(4))
    p, v, j = sw.best("f1")
    assert (p, v, j) == (0.4, 1.0, 1)
    # nearest 0.5 beats lower: 0.45 against 0.2
    sw = M.ThresholdSweep(np.array([0.2, 0.45, 0.8], np.float32), M.sweep_model(s, t, [0.2, 0.45, 0.8]),
                          probabilities=[0.2, 0.45, 0.8])
    assert sw.best()[2] == 1 and sw.best("iou")[2] == 1
    # no tie: the maximum wins wherever it is
    s2 = np.array([0.9] * 5 + [0.1] * 10 + [0.7] * 10, dtype=np.float32)
    sw = M.ThresholdSweep(th, M.sweep_model(s2, t, th))
    assert sw.best("f1")[2] == 3 and sw.best("f1")[1] == 1.0
    # the logit domain reports the threshold as a probability
    lt = M.sweep_thresholds([0.25, 0.5, 0.75], "logit")
    assert lt.dtype == np.float32 and lt[1] == 0.0 and lt[0] == np.float32(np.log(0.25 / 0.75))
    sw = M.ThresholdSweep(lt, M.sweep_model(np.array([-5, 5], np.float32), np.array([0, 1], np.float32), lt), "logit")
    assert sw.best()[0] == 0.5 and abs(sw.probabilities[0] - 0.25) < 1e-7
    with pytest.raises(ValueError):
        sw.best("loss")
    with pytest.raises(ValueError):
        M.ThresholdSweep([0.5, 0.5], np.zeros((2, 3)))
    with pytest.raises(ValueError):
        M.ThresholdSweep([0.5], np.zeros((2, 3)))
    with pytest.raises(ValueError):
        M.ThresholdSweep([0.5], np.zeros((2, 2)), "percent")


def test_default_thresholds():
    assert len(M.DEFAULT_THRESHOLDS) == 19
    assert np.allclose(M.DEFAULT_THRESHOLDS, np.arange(1, 20) * 0.05, rtol=0, atol=1e-12)
    assert M.DEFAULT_THRESHOLDS[9] == 0.5


# ---- combine_model -----------------------------------------------------------------------------------------------

def test_combine_model_of_one_is_its_input():
    rng = np.random.default_rng(0)
    p = rng.random(1000).astype(np.float32)
    p[:6] = [0.0, 1.0, 1e-45, 1e-39, 0.5, np.nan]
    for w in (None, [1.0]):
        got, mask = E.combine_model([p], w, 0.5)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), p.view(np.uint32))
        assert np.array_equal(mask, np.where(np.nan_to_num(p, nan=0.0) > 0.5, 255, 0)) and mask.dtype == np.uint8
    assert mask[4] == 0 and mask[5] == 0                     # equal to the threshold, and NaN


def test_combine_model_is_the_sequential_float32_sum():
    rng = np.random.default_rng(1)
    p = rng.random(5000).astype(np.float32)
    w = np.float32(1.0 / 3)
    want = np.empty_like(p)
    for i, v in enumerate(p):                                # one rounding per operation, written out
        a = np.float32(w * v)
        a = np.float32(a + np.float32(w * v))
        a = np.float32(a + np.float32(w * v))
        want[i] = a
    got, _ = E.combine_model([p, p, p], None, 0.5)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got != p).any()                                  # three equal members do not always average to themselves
    # unequal members and weights, against float64 rounding of each step
    q, r = rng.random(5000).astype(np.float32), rng.random(5000).astype(np.float32)
    ws = E.normalise_weights([1, 2, 5], 3)
    assert ws.dtype == np.float32 and np.array_equal(ws, (np.array([1, 2, 5]) / 8.0).astype(np.float32))
    acc = (ws[0].astype(np.float64) * p).astype(np.float32)
    for wk, x in ((ws[1], q), (ws[2], r)):
        acc = (acc.astype(np.float64) + (wk.astype(np.float64) * x).astype(np.float32)).astype(np.float32)
    got, mask = E.combine_model([p, q, r], ws, 0.4)
    assert np.array_equal(got, acc) and np.array_equal(mask, np.where(acc > np.float32(0.4), 255, 0))


def test_normalise_weights():
    assert np.array_equal(E.normalise_weights(None, 3), np.full(3, np.float32(1.0 / 3)))
    assert np.array_equal(E.normalise_weights([2.0], 1), [np.float32(1.0)])
    for bad in ([1, -1], [0, 0], [1, np.nan], [1, np.inf], [1, 2, 3]):
        with pytest.raises(ValueError):
            E.normalise_weights(bad, 2)


# ---- the entry points refuse before a device is touched ----------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def refused(lib, rc):
    return rc == 1 and lib.unet_op_last_error().startswith(b"invalid argument")


def test_combine_refuses_bad_arguments(lib):
    f = (C.c_float * 64)()
    q = C.cast(f, C.c_void_p)
    m8 = C.cast((C.c_uint8 * 64)(), C.c_void_p)

    def ptrs(k, null_at=None):
        return (C.c_void_p * max(k, 1))(*[None if i == null_at else q.value for i in range(max(k, 1))])

    def w(*v):
        return (C.c_float * len(v))(*v)
    call = lib.unet_ensemble_combine
    assert refused(lib, call(0, None, 2, None, 64, 0.5, q, m8, None))                    # no pointer array
    assert refused(lib, call(0, ptrs(3, null_at=1), 3, None, 64, 0.5, q, m8, None))      # a null member
    assert refused(lib, call(0, ptrs(1), 0, None, 64, 0.5, q, m8, None))                 # k outside 1 .. 8
    assert refused(lib, call(0, ptrs(9), 9, None, 64, 0.5, q, m8, None))
    assert refused(lib, call(0, ptrs(1), -1, None, 64, 0.5, q, m8, None))
    assert refused(lib, call(0, ptrs(2), 2, None, 64, 0.5, None, None, None))            # both outputs null
    assert b"outputs" in lib.unet_op_last_error()
    assert refused(lib, call(0, ptrs(2), 2, w(0.5, -0.5), 64, 0.5, q, m8, None))         # weights
    assert b"weight" in lib.unet_op_last_error()
    assert refused(lib, call(0, ptrs(2), 2, w(0.5, float("nan")), 64, 0.5, q, m8, None))
    assert refused(lib, call(0, ptrs(2), 2, w(float("inf"), 0.5), 64, 0.5, q, m8, None))
    assert refused(lib, call(0, ptrs(2), 2, None, 0, 0.5, q, m8, None))                  # numel == 0
    # what passes the checks goes on to the device: an ordinal the runtime refuses shows it got that far
    assert call(1 << 20, ptrs(2), 2, w(0.5, 0.5), 64, 0.5, q, None, None) == _lib.UNET_ERR_HIP
    assert b"hipSetDevice" in lib.unet_op_last_error()
    assert call(1 << 20, ptrs(8), 8, None, 64, 0.5, None, m8, None) == _lib.UNET_ERR_HIP
    assert call(1 << 20, ptrs(2), 2, w(0.0, 1.0), 64, 0.5, q, m8, None) == _lib.UNET_ERR_HIP   # a zero weight is allowed


def test_sweep_refuses_bad_arguments(lib):
    f = (C.c_float * 64)()
    q = C.cast(f, C.c_void_p)
    cnt = C.cast((C.c_uint64 * 200)(), C.c_void_p)

    def th(*v):
        return (C.c_float * len(v))(*v)
    ok = th(0.25, 0.5, 0.75)
    call = lib.unet_score_sweep_accumulate
    for u8 in (0, 1):
        assert refused(lib, call(0, None, q, u8, 64, ok, 3, cnt, None))                  # null inputs
        assert refused(lib, call(0, q, None, u8, 64, ok, 3, cnt, None))
        assert refused(lib, call(0, q, q, u8, 64, None, 3, cnt, None))
        assert refused(lib, call(0, q, q, u8, 64, ok, 3, None, None))
        assert refused(lib, call(0, q, q, u8, 0, ok, 3, cnt, None))                      # numel == 0
    assert refused(lib, call(0, q, q, 0, 64, ok, 0, cnt, None))                          # T outside 1 .. 64
    assert refused(lib, call(0, q, q, 0, 64, th(*np.linspace(0, 1, 65)), 65, cnt, None))
    assert refused(lib, call(0, q, q, 0, 64, ok, -3, cnt, None))
    assert refused(lib, call(0, q, q, 0, 64, th(0.5, 0.5), 2, cnt, None))                # not strictly ascending
    assert b"ascending" in lib.unet_op_last_error()
    assert refused(lib, call(0, q, q, 0, 64, th(0.5, 0.25), 2, cnt, None))
    assert refused(lib, call(0, q, q, 0, 64, th(float("nan")), 1, cnt, None))            # NaN, alone and inside
    assert refused(lib, call(0, q, q, 0, 64, th(0.1, float("nan"), 0.9), 3, cnt, None))
    assert refused(lib, call(0, q, q, 0, 64, th(float("-inf"), float("-inf")), 2, cnt, None))
    assert not any(cnt_word for cnt_word in C.cast(cnt, C.POINTER(C.c_uint64))[:200])
    # more elements than the grid rule covers with 32-bit counters per block
    assert call(0, q, q, 0, 1 << 41, ok, 3, cnt, None) == 2
    assert b"2^41" in lib.unet_op_last_error()
    # accepted: -inf first, +inf last, 64 thresholds - refused only by the device ordinal
    bad = 1 << 20
    assert call(bad, q, q, 0, 64, th(float("-inf"), 0.5, float("inf")), 3, cnt, None) == _lib.UNET_ERR_HIP
    assert b"hipSetDevice" in lib.unet_op_last_error()
    assert call(bad, q, q, 1, 64, th(*np.linspace(0, 1, 64)), 64, cnt, None) == _lib.UNET_ERR_HIP
    assert call(bad, q, q, 1, (1 << 41) - 1, th(0.5), 1, cnt, None) == _lib.UNET_ERR_HIP
    assert lib.unet_set_sweep_combine(0) == 1 and lib.unet_set_sweep_combine(1) == 0     # returns the previous setting


def test_grid_rule_keeps_block_counters_below_2_32():
    """csrc/ensemble_kernels.h, sweep_grid restated: one block per 4096 elements, 1024 at the most; what a block of
    256 threads can see on either path stays below 2^32 for every numel the entry point accepts."""
    def grid(n):
        return max(1, min(1024, -(-n // 4096)))
    for n in (1, 4095, 4096, 4097, 3 * 64 * 64 + 1, 1 << 30, (1 << 41) - 1):
        g = grid(n)
        vec_rounds = -(-(n // 4) // (256 * g))
        scalar_rounds = -(-n // (256 * g))
        assert vec_rounds * 1024 + 256 < 1 << 32 and scalar_rounds * 256 < 1 << 32, n
