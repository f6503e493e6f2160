"""K-class models on the int8 tier, the part that needs no device: the K-row head arrays of quant.quantize_model, the
float64 unit models with K rows, the sliced-oracle reference the GPU tests compare with, the file round trip, the
device-free refusals of the new entry points and the argument checks of run_u8 / FramePipeline / LanePipelineGPU."""
import ctypes as C

import numpy as np
import pytest

from int8_classes_model import sliced_reference
from oracle import int8_oracle as Q
from unet_lane_detection_amd import _lib, quant, state as S

FEATS = [16, 32]
INVALID, STATE = 1, 3
NO_DEVICE = 1 << 20          # an ordinal the runtime refuses, with or without GPUs: no device is touched


@pytest.fixture(scope="module")
def model3():
    sd = S.seeded_state_dict(FEATS, seed=0, out_channels=3)
    frames = S.synthetic_frames(2, 16, 16, seed=1)
    ranges = Q.float_ranges(sd, frames)
    return sd, frames, ranges, quant.quantize_model(sd, ranges)


def test_k_class_head_arrays(model3):
    sd, _, ranges, qm = model3
    c = FEATS[0]
    assert qm["output.w_q"].shape == (3, c, 1, 1) and qm["output.w_q"].dtype == np.int8
    for f, dt in (("w_zp", np.int32), ("bias_q", np.int32), ("mult", np.float32)):
        a = np.asarray(qm["output." + f])
        assert a.shape == (3,) and a.dtype == dt, f
    assert quant.out_channels(qm) == 3
    for k in range(3):                     # row k is what quantising row k alone gives
        one = dict(sd)
        one["output.weight"] = np.asarray(sd["output.weight"])[k:k + 1]
        one["output.bias"] = np.asarray(sd["output.bias"])[k:k + 1]
        q1 = quant.quantize_model(one, ranges)
        assert quant.out_channels(q1) == 1
        for f in ("w_q", "w_zp", "bias_q", "mult", "w_scale"):
            assert np.array_equal(np.asarray(qm["output." + f])[k:k + 1], np.asarray(q1["output." + f])), (k, f)
    body = [k for k in qm if not k.startswith("output.")]
    single = quant.quantize_model(S.seeded_state_dict(FEATS, seed=0), ranges)
    assert all(np.array_equal(qm[k], single[k]) for k in body)          # the body does not know the class count


def test_sliced_oracle_reference(model3):
    _, frames, _, qm = model3
    with pytest.raises(Exception):          # the oracle's head has one row
        Q.forward(qm, frames)
    ref = sliced_reference(qm, frames)
    assert ref.shape == (2, 3, 16, 16) and ref.dtype == np.float32 and np.isfinite(ref).all()
    labels = ref.argmax(1)
    assert set(np.unique(labels)) == {0, 1, 2}
    top = np.sort(ref, axis=1)
    assert (top[:, -1] > top[:, -2]).all()  # no exact tie on this model: argmax needs no tie rule here
    # the same logits from the product's own integer rule on the K rows at once
    lg, info = quant.hybrid_forward_model(qm, frames)
    assert info == {} and np.array_equal(lg, ref)


def _direct_head(qm, x):
    """float64 evaluation of a hybrid head's arithmetic, written out: v[k] = (sum_c w16[k,c] x[c]) m[k] + b[k]"""
    w = np.asarray(qm["output.w_h"]).view(np.float16).astype(np.float64).reshape(-1, x.shape[1])
    if x.dtype == np.int8:
        xv = x.astype(np.float64) - float(qm["output.x_zp"])
        m = np.asarray(qm["output.gain"], np.float32).astype(np.float64) * float(np.float32(qm["output.x_scale"]))
    else:
        xv = x.astype(np.float64)
        m = np.asarray(qm["output.gain"], np.float32).astype(np.float64)
    b = np.asarray(qm["output.bias_f"], np.float32).astype(np.float64)
    return np.einsum("nchw,kc->nkhw", xv, w) * m[None, :, None, None] + b[None, :, None, None]


def test_unit_model_with_k_rows(model3):
    sd, frames, ranges, _ = model3
    qh = quant.quantize_model(sd, ranges, hybrid=("output",))
    assert qh["output.w_h"].shape == (3, FEATS[0], 1, 1) and qh["output.gain"].shape == (3,) and qh["output.bias_f"].shape == (3,)
    rng = np.random.default_rng(0)
    x8 = rng.integers(-128, 128, size=(2, FEATS[0], 4, 6)).astype(np.int8)
    out = quant.unit_model(qh, "output", x8)
    assert out["dtype"] == "fp32" and out["K"] == FEATS[0] and out["v"].shape == (2, 3, 4, 6)
    assert np.abs(out["v"] - _direct_head(qh, x8)).max() <= 1e-12 * np.abs(out["S"]).max()
    assert (np.abs(out["v"]) <= out["S"] * (1 + 1e-12)).all()
    qa = quant.quantize_model(sd, ranges, hybrid=quant.unit_names(FEATS))
    x16 = rng.normal(0, 2, size=(1, FEATS[0], 4, 4)).astype(np.float16).astype(np.float32)
    out = quant.unit_model(qa, "output", x16)
    assert np.abs(out["v"] - _direct_head(qa, x16)).max() <= 1e-12 * np.abs(out["S"]).max()
    lg, info = quant.hybrid_forward_model(qa, frames)
    assert lg.shape == (2, 3, 16, 16) and info["output"]["v"].shape == (2, 3, 16, 16)
    # a unit that is not hybrid: the integer rule on K rows equals the rule on each row alone
    qp = quant.quantize_model(sd, ranges)
    y = quant.unit_model(qp, "output", x8)["y"]
    for k in range(3):
        q1 = dict(qp)
        for f in ("w_q", "w_zp", "bias_q", "mult"):
            q1["output." + f] = np.asarray(qp["output." + f])[k:k + 1]
        assert np.array_equal(y[:, k:k + 1], quant.unit_model(q1, "output", x8)["y"])


def test_single_row_results_are_what_they_were():
    """K = 1 through unit_model / hybrid_forward_model: the float32 bit patterns the parent commit's quant.py gives for
    the same inputs (computed there, pinned here)."""
    sd = S.seeded_state_dict(FEATS, 0)
    frames = S.synthetic_frames(1, 8, 8, seed=3)
    ranges = {n: (-4.0 + 0.1 * i, 5.0 + 0.2 * i) for i, n in enumerate(quant.tensor_names(2))}
    qh = quant.quantize_model(sd, ranges, hybrid=("output", "decoder_blocks.3.3"))
    qp = quant.quantize_model(sd, ranges)
    lg, _ = quant.hybrid_forward_model(qh, frames)
    assert lg.shape == (1, 1, 8, 8)
    assert lg[0, 0, 2].view(np.uint32).tolist() == [1066366131, 1057927798, 1063473277, 1080731396, 3202515568, 1052084972,
                                                    1065846398, 1066533149]
    lg, _ = quant.hybrid_forward_model(qp, frames)
    assert lg[0, 0, 2].view(np.uint32).tolist() == [1066606577, 1057720306, 1064144320, 1080885847, 3201676976, 1051742686,
                                                    1065985986, 1066622439]
    x = np.arange(-64, 64, dtype=np.int8).reshape(1, 16, 2, 4)
    assert quant.unit_model(qh, "output", x)["y"].reshape(-1).view(np.uint32).tolist() == [
        1090921892, 1091045097, 1091168302, 1091291507, 1091414712, 1091537917, 1091661122, 1091784327]
    assert quant.unit_model(qp, "output", x)["y"].reshape(-1).view(np.uint32).tolist() == [
        1090936189, 1091059613, 1091183037, 1091306462, 1091429886, 1091553310, 1091676735, 1091800159]


def test_file_round_trip(model3, tmp_path):
    sd, _, ranges, _ = model3
    qm = quant.quantize_model(sd, ranges, hybrid=("output",))
    p = tmp_path / "classes.npz"
    quant.save_quantized(p, qm)
    back = quant.load_quantized(p)
    assert set(back) == set(qm) and quant.out_channels(back) == 3 and quant.hybrid_units(back) == ["output"]
    for k in qm:
        a, b = np.asarray(qm[k]), np.asarray(back[k])
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), k


# ---- the C entry points, as far as they go without a device ---------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _handle(lib, qm, device=NO_DEVICE):
    feats = (C.c_int * len(FEATS))(*FEATS)
    h = C.c_void_p()
    assert lib.unet_i8_create(len(FEATS), feats, device, C.byref(h)) == 0
    for k, v in qm.items():
        if k == "features":
            continue
        a = np.ascontiguousarray(np.asarray(v))
        if a.dtype == np.float64:
            a = a.astype(np.float32)
        if a.dtype == np.int64:
            a = a.astype(np.int32)
        assert lib.unet_i8_load(h, k.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
    return h


def _refused(lib, h, rc, *words):
    msg = lib.unet_i8_last_error(h) or b""
    return rc == INVALID and len(msg) > 10 and all(w in msg for w in words)


def test_finalize_derives_the_class_count_before_any_device(lib, model3):
    sd, _, ranges, qm = model3
    h = _handle(lib, qm)
    assert lib.unet_i8_out_channels(h) == 0 and lib.unet_i8_out_channels(None) == 0
    assert lib.unet_i8_finalize(h) == _lib.UNET_ERR_HIP          # the head is settled, then the device is refused
    assert lib.unet_i8_out_channels(h) == 3
    assert lib.unet_i8_destroy(h) == 0
    single = quant.quantize_model(S.seeded_state_dict(FEATS, seed=0), ranges)
    h = _handle(lib, single)
    assert lib.unet_i8_finalize(h) == _lib.UNET_ERR_HIP and lib.unet_i8_out_channels(h) == 1
    assert lib.unet_i8_destroy(h) == 0


@pytest.mark.parametrize("field,rows", [("w_zp", 2), ("mult", 4), ("w_q", 2), ("bias_q", 9), ("bias_q", 0), ("w_h", 1),
                                        ("gain", 2), ("bias_f", 1)])
def test_finalize_refuses_head_arrays_that_disagree(lib, model3, field, rows):
    sd, _, ranges, _ = model3
    qm = dict(quant.quantize_model(sd, ranges, hybrid=("output",)))
    a = np.asarray(qm["output." + field])
    qm["output." + field] = np.ascontiguousarray(np.resize(a, (rows,) + a.shape[1:]))
    h = _handle(lib, qm)
    assert lib.unet_i8_finalize(h) == STATE
    msg = lib.unet_i8_last_error(h)
    assert b"output." in msg and len(msg) > 20, msg
    assert lib.unet_i8_destroy(h) == 0


def test_forward_entry_points_refuse_the_other_kind_and_bad_outputs(lib, model3):
    sd, _, ranges, qm = model3
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.unet_i8_forward_classes_u8(None, p, 1, 8, 8, p, None, None, 0, None, None) == INVALID
    assert lib.unet_i8_run_head(None, p, None, None, 0, None, 0.0, None) == INVALID
    h = _handle(lib, qm)
    lib.unet_i8_finalize(h)
    assert lib.unet_i8_forward_classes_u8(h, None, 1, 8, 8, p, None, None, 0, None, None) == INVALID
    assert _refused(lib, h, lib.unet_i8_forward_u8(h, p, 1, 8, 8, p, None, None, 0.0, None), b"unet_i8_forward_u8", b"3 classes")
    assert _refused(lib, h, lib.unet_i8_forward_classes_u8(h, p, 1, 8, 8, None, None, None, 0, None, None), b"no output")
    for bad in (-1, 3, 8):
        assert _refused(lib, h, lib.unet_i8_forward_classes_u8(h, p, 1, 8, 8, None, None, None, bad, p, None), b"mask_class")
    odd = C.c_void_p(p.value + 4)
    assert _refused(lib, h, lib.unet_i8_forward_classes_u8(h, p, 1, 8, 8, odd, None, None, 0, None, None), b"aligned")
    assert lib.unet_i8_forward_classes_u8(h, p, 1, 8, 8, p, None, None, 0, None, None) == STATE      # no device was there
    assert lib.unet_i8_run_head(h, p, None, None, 0, None, 0.0, None) == STATE
    assert lib.unet_i8_destroy(h) == 0
    single = quant.quantize_model(S.seeded_state_dict(FEATS, seed=0), ranges)
    h = _handle(lib, single)
    lib.unet_i8_finalize(h)
    assert _refused(lib, h, lib.unet_i8_forward_classes_u8(h, p, 1, 8, 8, p, None, None, 0, None, None), b"single-class")
    assert lib.unet_i8_forward_u8(h, p, 1, 8, 8, p, None, None, 0.0, None) == STATE
    assert lib.unet_i8_destroy(h) == 0


def _float_handle(lib, k):
    cfg = _lib.UnetConfig()
    cfg.in_channels, cfg.out_channels, cfg.depth = 3, k, 2
    cfg.features[0], cfg.features[1] = 8, 16
    h = C.c_void_p()
    assert lib.unet_create(C.byref(cfg), C.byref(h)) == 0
    return h


def test_class_calibration_entry_points_refuse_a_single_class_handle(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    h = _float_handle(lib, 1)
    for rc in (lib.unet_forward_classes_u8_ranges(h, p, 1, 8, 8, p, None),
               lib.unet_forward_classes_u8_histograms(h, p, 1, 8, 8, p, 64, p, None)):
        assert rc == INVALID and b"single-class" in lib.unet_last_error(h)
    assert lib.unet_destroy(h) == 0
    h = _float_handle(lib, 3)
    assert lib.unet_forward_u8_histograms(h, p, 1, 8, 8, p, 64, p, None) == INVALID      # and the other way round, as before
    assert lib.unet_forward_classes_u8_ranges(h, None, 1, 8, 8, p, None) == INVALID
    assert lib.unet_destroy(h) == 0
    assert lib.unet_forward_classes_u8_ranges(None, p, 1, 8, 8, p, None) == INVALID


# ---- Python argument checks that precede any device call -----------------------------------------------------------
class _Net:
    """run_u8's argument checks need the handle's class count and nothing else"""

    def __init__(self, k):
        import torch
        self.out_channels, self._h, self.device = k, object(), torch.device("cpu")

    def _require_live(self):
        pass


def test_run_u8_argument_checks():
    import torch
    from unet_lane_detection_amd.int8 import UNetInt8
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    k3, k1 = _Net(3), _Net(1)
    with pytest.raises(ValueError, match="return_mask"):
        UNetInt8.run_u8(k3, frames, return_mask=True)
    with pytest.raises(ValueError, match="threshold"):
        UNetInt8.run_u8(k3, frames, threshold=0.3)
    with pytest.raises(ValueError, match="mask_class"):
        UNetInt8.run_u8(k3, frames, mask_class=3)
    with pytest.raises(ValueError, match="K-class"):
        UNetInt8.run_u8(k1, frames, return_labels=True)
    with pytest.raises(ValueError, match="K-class"):
        UNetInt8.run_u8(k1, frames, mask_class=0)
    with pytest.raises(ValueError, match="K-class"):
        UNetInt8.predict_labels(k1, frames)
    with pytest.raises(ValueError, match="K-class"):
        UNetInt8.evaluate_classes(k1, frames, torch.zeros((1, 8, 8), dtype=torch.uint8))


def test_pipelines_check_mask_class_at_construction():
    from unet_lane_detection_amd.ros_bridge import LanePipelineGPU
    from unet_lane_detection_amd.video import FramePipeline, check_mask_class
    k3, k1 = _Net(3), _Net(1)
    assert check_mask_class(k3, 2) == 2 and check_mask_class(k1, None) is None
    for cls in (FramePipeline, LanePipelineGPU):
        with pytest.raises(ValueError, match="mask_class"):
            cls(k3)
        with pytest.raises(ValueError, match="mask_class"):
            cls(k3, mask_class=3)
        with pytest.raises(ValueError, match="mask_class"):
            cls(k1, mask_class=0)
