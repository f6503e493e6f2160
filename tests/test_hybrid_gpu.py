"""Hybrid quantisation of the int8 tier on the GPU (csrc/conv_h16.h): every hybrid unit against the float64 model of its
arithmetic (quant.unit_model) on the device's own input tensor, within the derived bound quant.hybrid_bound - no element
excluded; every other unit bit-exact against the integer oracle on the device's own input; tensor types, the pure-int8
run of a hybrid file, the file and the container, accuracy against the fp32 tier, and the sensitivity search."""
import numpy as np
import pytest
import torch

from oracle import int8_oracle as Q
from unet_lane_detection_amd import quant, state as S

pytestmark = pytest.mark.gpu

NETS = {"small": [16, 32], "b": [32, 64, 128]}
# (network, N, H, W): the second network gives ragged tile grids and 256-channel inputs
SHAPES = [("small", 2, 32, 32), ("small", 3, 24, 40), ("small", 1, 8, 8), ("b", 2, 16, 24), ("b", 1, 40, 72)]


def _sets(feats):
    """The hybrid sets of more than one unit, by name."""
    d = len(feats)
    return {
        "all": tuple(quant.unit_names(feats)),
        "encoder_block": ("encoder_blocks.1.0", "encoder_blocks.1.3"),
        # cat0: both writers and both readers
        "cat0_fp16": ("encoder_blocks.0.3", f"decoder_blocks.{2 * d - 2}", f"decoder_blocks.{2 * d - 1}.0", "encoder_blocks.1.0"),
        "decoder_block_and_head": (f"decoder_blocks.{2 * d - 2}", f"decoder_blocks.{2 * d - 1}.0", f"decoder_blocks.{2 * d - 1}.3",
                                   "output"),
    }


CASES = [(s, u) for s in range(len(SHAPES)) for u in quant.unit_names(NETS[SHAPES[s][0]])]
CASES += [(s, name) for s in range(len(SHAPES)) for name in ("all", "encoder_block", "cat0_fp16", "decoder_block_and_head")]


@pytest.fixture(scope="module")
def nets():
    """Per network: seeded float weights, the fp32 HIP handle and the ranges of a device calibration."""
    from unet_lane_detection_amd.int8 import calibrate
    from unet_lane_detection_amd.model import UNetHIP
    out = {}
    calib = torch.from_numpy(S.synthetic_frames(6, 64, 64, seed=1))
    for name, feats in NETS.items():
        sd = S.seeded_state_dict(feats, seed=0)
        fm = UNetHIP(sd, device=0)
        out[name] = (sd, fm, calibrate(fm, calib, batch=6))
    yield out
    for _, fm, _ in out.values():
        fm.release()


_frames = {}


def frames_of(s):
    if s not in _frames:
        _, n, h, w = SHAPES[s]
        _frames[s] = S.synthetic_frames(n, h, w, seed=20 + s)
    return _frames[s]


def _level(name, d):
    if name.startswith("enc"):
        return int(name[3:-2])
    if name.startswith("cat"):
        return int(name.split(".")[0][3:]) + (1 if name.endswith(".pool") else 0)
    if name.startswith("bott"):
        return d
    return d - 1 - int(name[3:-2])          # dec<j>.a / .b


def _oracle_unit(qm, key, kind, x):
    """The integer oracle's arithmetic of one unit on int8 input x: int8 output, or float32 logits for the head."""
    if kind == "head":
        xz = x.astype(np.int64) - int(qm["output.x_zp"])
        wz = qm["output.w_q"].astype(np.int64).reshape(1, -1) - np.asarray(qm["output.w_zp"], dtype=np.int64).reshape(1, 1)
        acc = np.einsum("nchw,oc->nohw", xz, wz) + np.asarray(qm["output.bias_q"], dtype=np.int64)[None, :, None, None]
        return (acc.astype(np.float32) * np.asarray(qm["output.mult"], dtype=np.float32)[None, :, None, None]).astype(np.float32)
    fn = Q.upconv2x2_acc if kind == "up" else Q.conv3x3_acc
    acc = fn(x, int(qm[key + ".x_zp"]), qm[key + ".w_q"], qm[key + ".w_zp"])
    return Q.requantize(acc, qm[key + ".bias_q"], qm[key + ".mult"], int(qm[key + ".y_zp"]), bool(int(qm[key + ".relu"])))


def check_forward(qm, net, frames):
    """One device forward; every unit checked on the device's own input.  Returns the logits."""
    feats = [int(f) for f in qm["features"]]
    d = len(feats)
    n, h, w, _ = frames.shape
    hybrid = quant.hybrid_units(qm)
    logits = net.run_u8(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    logits = logits.cpu().numpy()
    dtypes = quant.tensor_dtypes(feats, hybrid)
    for name, dt in dtypes.items():
        assert net.tensor_dtype(name) == dt, (name, dt)
    assert net.tensor_dtype("im2col") == "int8"

    def read(name):
        if name == "input":              # the centre tap of the im2col rows is the quantised input itself
            return np.ascontiguousarray(net.read_tensor("im2col", n, h, w)[:, 12:15])
        lv = _level(name, d)
        t = net.read_tensor(name, n, h >> lv, w >> lv)
        assert t.dtype == (np.float32 if dtypes[name] == "fp16" else np.int8), name
        return t

    assert np.array_equal(read("input"), Q.quantize_input(frames, qm["input.lut"]))
    for key, kind, xname, yname, relu in quant.unit_table(feats):
        x = read(xname)
        if yname is None:
            got = logits
        else:
            got = read(yname)
            if yname.startswith("cat"):
                f = feats[int(yname[3:])]
                got = got[:, :f] if kind == "conv" else got[:, f:]
        if key not in hybrid:
            want = _oracle_unit(qm, key, kind, x)
            assert got.shape == want.shape and np.array_equal(got, want), \
                f"{key}: {(got != want).sum()} of {want.size} values differ from the integer oracle"
            continue
        out = quant.unit_model(qm, key, x)
        assert got.shape == out["v"].shape, (key, got.shape)
        if out["dtype"] == "int8":
            zy, sy = int(qm[key + ".y_zp"]), float(qm[key + ".y_scale"])
            want = np.clip(out["v"] / sy + zy, zy if relu else -128, 127)
            bound = quant.hybrid_bound(out, sy)
        else:
            want = np.minimum(out["v"], 65504.0)
            bound = quant.hybrid_bound(out)
        excess = np.abs(got.astype(np.float64) - want) - bound
        bad = int((excess > 0).sum())
        assert bad == 0, (f"{key} ({out['dtype']} output, K = {out['K']}): {bad} of {want.size} elements outside the bound, "
                          f"worst by {excess.max():.3g} where the bound is {np.ravel(bound)[np.argmax(excess)]:.3g}")
    for l in range(d):                  # pooled tensors are exact, whichever the type
        assert np.array_equal(read(f"cat{l}.pool"), Q.maxpool2x2(read(f"cat{l}")[:, :feats[l]])), f"cat{l}.pool"
    return logits


@pytest.mark.parametrize("s,which", CASES, ids=[f"{SHAPES[s][0]}-{SHAPES[s][1]}x{SHAPES[s][2]}x{SHAPES[s][3]}-{u}" for s, u in CASES])
def test_hybrid_units_match_the_model(nets, s, which):
    from unet_lane_detection_amd.int8 import UNetInt8
    name = SHAPES[s][0]
    sd, _, ranges = nets[name]
    hybrid = _sets(NETS[name]).get(which, (which,))
    qm = quant.quantize_model(sd, ranges, hybrid=hybrid)
    net = UNetInt8(qm, device=0)
    try:
        logits = check_forward(qm, net, frames_of(s))
        assert np.isfinite(logits).all()
    finally:
        net.release()


def test_pure_int8_from_a_hybrid_file_is_bit_identical(nets):
    from unet_lane_detection_amd.int8 import UNetInt8
    sd, _, ranges = nets["b"]
    frames = torch.from_numpy(S.synthetic_frames(2, 32, 32, seed=31)).cuda()
    plain = UNetInt8(quant.quantize_model(sd, ranges), device=0)
    ref = plain.run_u8(frames).cpu().numpy()
    plain.release()
    qm = quant.quantize_model(sd, ranges, hybrid=quant.unit_names(NETS["b"]))
    pure = UNetInt8(qm, device=0, hybrid=False)
    got = pure.run_u8(frames).cpu().numpy()
    assert all(pure.tensor_dtype(t) == "int8" for t in quant.tensor_names(3))
    pure.release()
    assert np.array_equal(got, ref)
    assert np.array_equal(ref, Q.forward(qm, frames.cpu().numpy()))
    hyb = UNetInt8(qm, device=0)
    other = hyb.run_u8(frames).cpu().numpy()
    hyb.release()
    assert not np.array_equal(other, ref)           # the marks are honoured by default


def test_hybrid_file_container_range_and_device_error(nets, tmp_path):
    from unet_lane_detection_amd import _lib
    from unet_lane_detection_amd.int8 import UNetInt8
    from unet_lane_detection_amd.py_utils.rknn_executor import RKNN_model_container
    sd, fm, ranges = nets["b"]
    hybrid = ("encoder_blocks.0.0", "encoder_blocks.0.3", "decoder_blocks.5.3", "output")
    qm = quant.quantize_model(sd, ranges, hybrid=hybrid)
    p = tmp_path / "lane_unet_hybrid.npz"
    quant.save_quantized(p, qm)
    assert quant.hybrid_units(quant.load_quantized(p)) == list(hybrid)
    frame = S.synthetic_frames(1, 224, 224, seed=11)
    direct = UNetInt8(qm, device=0)
    net = UNetInt8.from_file(p, device=0)
    assert net.tensor_dtype("enc0.a") == "fp16" and net.tensor_dtype("dec2.b") == "fp16" and net.tensor_dtype("cat0") == "int8"
    fd = torch.from_numpy(frame).cuda()
    la, pa = direct.run_u8(fd, return_probs=True)
    lb = net.run_u8(fd)
    assert torch.equal(la, lb)
    with pytest.raises(_lib.UnetError):              # the int8 reader refuses an fp16 tensor, and the other way round
        net._check(net._lib.unet_i8_read_tensor(net._h, b"enc0.a", np.empty(1 << 22, np.int8).ctypes.data, 1 << 22, None), "read")
    with pytest.raises(_lib.UnetError):
        net._check(net._lib.unet_i8_read_tensor_f16(net._h, b"cat0", np.empty(1 << 22, np.int8).ctypes.data, 1 << 22, None), "read")
    c = RKNN_model_container(str(p), "rk3588", "0")
    assert c.precision == "int8"
    out = c.run(inputs=[frame])
    assert isinstance(out, list) and out[0].shape == (1, 1, 224, 224) and out[0].dtype == np.float32
    assert np.abs(out[0] - pa.cpu().numpy()).max() < 1e-6
    pure = UNetInt8(qm, device=0, hybrid=False)
    assert not torch.equal(pure.run_u8(fd), la)
    c.release()
    for m in (direct, net, pure):
        m.release()
    broken = dict(qm)
    del broken["output.w_h"]
    with pytest.raises(_lib.UnetError):
        UNetInt8(broken, device=0)
    wide = dict(ranges)
    wide["enc0.a"] = (0.0, 60001.0)
    with pytest.raises(ValueError):
        quant.quantize_model(sd, wide, hybrid=hybrid)
    torch.cuda.synchronize()
    assert fm.device_error() == 0


def test_all_hybrid_is_no_further_from_fp32_than_int8(nets):
    """tests/test_hybrid_cpu.py establishes the same with the float64 model alone (0.0013 against 0.0166)."""
    from unet_lane_detection_amd.int8 import UNetInt8, compare_outputs
    sd, fm, ranges = nets["b"]
    frames = torch.from_numpy(S.synthetic_frames(4, 64, 64, seed=9))
    maes = []
    for hybrid in ((), quant.unit_names(NETS["b"])):
        net = UNetInt8(quant.quantize_model(sd, ranges, hybrid=hybrid), device=0)
        maes.append(compare_outputs(fm, net, frames).mean)
        net.release()
    print("MAE against the fp32 tier: pure int8 %.6f, all units hybrid %.6f" % tuple(maes))
    assert maes[1] <= maes[0]


def test_sensitivity_and_choose_hybrid(nets):
    from unet_lane_detection_amd.int8 import UNetInt8, choose_hybrid, compare_outputs, sensitivity
    sd, fm, ranges = nets["small"]
    frames = torch.from_numpy(S.synthetic_frames(2, 32, 32, seed=41))
    rows = sensitivity(fm, sd, ranges, frames)
    units = quant.unit_names(NETS["small"])
    assert sorted(r[0] for r in rows) == sorted(units) and len(rows) == len(units)
    net = UNetInt8(quant.quantize_model(sd, ranges), device=0)
    base = compare_outputs(fm, net, frames).mean
    net.release()
    assert all(r[2] == base for r in rows)
    assert [r[1] for r in rows] == sorted(r[1] for r in rows)            # the largest gain first
    assert all(np.isfinite(r[1]) and r[1] >= 0 for r in rows)
    picked = choose_hybrid(fm, sd, ranges, frames, k=2)
    assert len(picked) == 2 and picked[0] != picked[1] and set(picked) <= set(units)
    assert picked[0] == rows[0][0]                   # the first greedy pick is the most sensitive unit
