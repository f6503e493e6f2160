"""Post-training quantisation of the float U-Net to the int8 tier.

What the reference does (README.md:3039-3272, `convert_rknn.py`): the float model goes through
`rknn.config(mean_values, std_values, quantized_dtype='asymmetric_quantized-8', quantized_algorithm='normal',
quantized_method='channel')` (README.md:3106-3116) and `rknn.build(do_quantization=True, dataset=...)` with ~100
calibration frames (README.md:3046-3078); the quantisation rule it documents is (README.md:3370-3383)

    q = round(r / scale) + zero_point,   scale = (r_max - r_min) / 255,   r ~= (q - zero_point) * scale

with q in [-128, 127].  The conversion itself happens inside Rockchip's closed toolkit, so its exact choices
(rounding, range handling, operator fusion) are not in the reference: this module restates the documented scheme.
Parity against the shipped .rknn blobs is **unpinned** (they cannot be executed and hold no float weights).

Scheme implemented here (the integer-exact contract of the int8 tier; oracle/int8_oracle.py restates the forward):
  * activations: per-tensor asymmetric int8; (r_min, r_max) from calibration ("normal" = min/max; "mmse" and
    "kl_divergence" choose a range inside min/max from a device histogram: range_from_histogram below), widened to
    contain 0 so that zero is exactly representable (padding, ReLU);
  * weights: per-output-channel ('channel') asymmetric int8 of the BatchNorm-folded weights (the blob's 14 ConvRelu
    nodes carry folded weight/bias pairs);
  * bias: int32 in units of x_scale * w_scale[co];
  * the two halves of a concat share one (scale, zero_point): both producers requantise into the concat tensor;
  * input: (u8 - mean) / std quantised per tensor through a 256-entry table per channel (the normalisation lives in
    the blob, README.md:3110-3111);
  * requantisation: q_out = clamp(rint(float32(acc + bias_q) * float32(x_scale * w_scale[co] / y_scale)) + y_zp),
    float32 multiply and round-half-even, ReLU as the lower clamp y_zp;
  * head (ConvSigmoid in the blob): logits = float32(acc + bias_q) * float32(x_scale * w_scale), then sigmoid.  A head
    of K = 2..8 rows (multi-class segmentation) is K such rows - row k quantised as it would be alone, with its own
    w_scale, w_zp, bias_q and mult - followed by softmax / argmax over the K logits.
"""
from __future__ import annotations

import numpy as np

from .state import BN_EPS, INPUT_MEAN, INPUT_STD

QMIN, QMAX = -128, 127


def affine_params(r_min, r_max):
    """(scale, zero_point) of an asymmetric int8 tensor whose real range is [r_min, r_max] widened to contain 0
    (README.md:3376-3379).  Returns (float64 scale, int zero_point)."""
    r_min = min(float(r_min), 0.0)
    r_max = max(float(r_max), 0.0)
    if r_max - r_min < 1e-30:
        return 1.0, 0
    scale = (r_max - r_min) / 255.0
    zp = int(np.clip(np.rint(QMIN - r_min / scale), QMIN, QMAX))
    return scale, zp


def quantize(r, scale, zp):
    """q = clamp(round(r / scale) + zp) (README.md:3370)."""
    return np.clip(np.rint(np.asarray(r, dtype=np.float64) / scale) + zp, QMIN, QMAX).astype(np.int8)


def dequantize(q, scale, zp):
    return (np.asarray(q, dtype=np.float64) - zp) * scale


def quantize_weight_per_channel(w, axis=0):
    """Per-output-channel asymmetric int8 ('channel', README.md:3116): returns (w_q int8, scale float64[O], zp int32[O])."""
    w = np.asarray(w, dtype=np.float64)
    wm = np.moveaxis(w, axis, 0).reshape(w.shape[axis], -1)
    scales = np.empty(wm.shape[0], dtype=np.float64)
    zps = np.empty(wm.shape[0], dtype=np.int32)
    q = np.empty_like(wm, dtype=np.int8)
    for o in range(wm.shape[0]):
        scales[o], zps[o] = affine_params(wm[o].min(), wm[o].max())
        q[o] = quantize(wm[o], scales[o], zps[o])
    wq = np.moveaxis(q.reshape((w.shape[axis],) + tuple(np.delete(w.shape, axis))), 0, axis)
    return np.ascontiguousarray(wq), scales, zps


def fold_bn(sd, prefix, conv_i, bn_i):
    """Conv + eval BatchNorm -> (w_fold, b_fold), float64 (what 'ConvRelu' nodes of the blob carry)."""
    w = np.asarray(sd[f"{prefix}.{conv_i}.weight"], dtype=np.float64)
    g = np.asarray(sd[f"{prefix}.{bn_i}.weight"], dtype=np.float64)
    b = np.asarray(sd[f"{prefix}.{bn_i}.bias"], dtype=np.float64)
    m = np.asarray(sd[f"{prefix}.{bn_i}.running_mean"], dtype=np.float64)
    v = np.asarray(sd[f"{prefix}.{bn_i}.running_var"], dtype=np.float64)
    s = g / np.sqrt(v + BN_EPS)
    return w * s[:, None, None, None], b - m * s


def tensor_names(depth):
    """Activation tensors that carry quantisation parameters, in the order the calibration pass reports them
    (unet_forward_u8_ranges): input, per level the first encoder conv and the concat tensor (skip half = second encoder
    conv, upper half = the decoder's transposed conv), the two bottleneck convs, per decoder step its two convs."""
    names = ["input"]
    for l in range(depth):
        names += [f"enc{l}.a", f"cat{l}"]
    names += ["bott.a", "bott.b"]
    for j in range(depth):
        names += [f"dec{j}.a", f"dec{j}.b"]
    return names


def tensor_shapes(features):
    """(channels, pooling level) of every tensor of tensor_names(len(features)), in that order: the tensor holds
    N * (H >> level) * (W >> level) * channels elements (the input counts its 3 real channels)."""
    d = len(features)
    shapes = [(3, 0)]
    for l in range(d):
        shapes += [(features[l], l), (2 * features[l], l)]
    shapes += [(2 * features[-1], d)] * 2
    for j in range(d):
        shapes += [(features[d - 1 - j], d - 1 - j)] * 2
    return shapes


# ---- calibration algorithms beyond min/max (README.md:3407-3412: 'normal', 'mmse', 'kl_divergence') ----------------
ALGORITHMS = ("normal", "mmse", "kl_divergence")
HIST_BINS = 2048            # default resolution of a calibration histogram
KL_MIN_BINS = 128           # 'kl_divergence' skips candidates that keep fewer bins than this


def _f32_span(lo, hi, bins):
    """(lo, inv) of the binning rule in float32: inv = float32(bins) / (hi - lo)."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        inv = np.float32(bins) / (hi32 - lo32)
    if not (hi32 > lo32) or not np.isfinite(inv) or not inv > 0:
        raise ValueError(f"histogram span ({lo}, {hi}) is empty or not finite")
    return lo32, inv


def _bin_index(v, lo32, inv, bins):
    """Bin of every element of the float32 array v (NaN: undefined, callers mask it):
    t = (v - lo) * inv in float32, two roundings; 0 below the span, bins - 1 at or above its end, else trunc(t)."""
    with np.errstate(all="ignore"):
        t = (v - lo32) * inv
    idx = np.zeros(t.shape, dtype=np.int64)
    inside = (t >= 0) & (t < bins)
    idx[inside] = t[inside].astype(np.int64)
    idx[t >= bins] = bins - 1
    return idx


def histogram_model(values, lo, hi, bins, c=None, ld=None):
    """numpy restatement, bit for bit, of the device histogram (csrc/calib_kernels.cpp, include/unet_hip.h): uint64
    [bins + 1].  Words 0 .. bins - 1: the elements binned over [lo, hi) in float32 arithmetic, elements outside the
    span in the first / last bin; word `bins`: the elements equal to 0 (either sign), which are in no bin.  NaN is not
    counted.  c, ld: `values` is pixels of ld floats of which the first c are counted."""
    v = np.ascontiguousarray(np.asarray(values, dtype=np.float32)).reshape(-1)
    if c is not None or ld is not None:
        if c is None or ld is None or not 1 <= c <= ld:
            raise ValueError("c and ld go together, 1 <= c <= ld")
        v = v.reshape(-1, ld)[:, :c].reshape(-1)
    lo32, inv = _f32_span(lo, hi, bins)
    zero = v == 0
    counted = ~zero & ~np.isnan(v)
    out = np.zeros(bins + 1, dtype=np.uint64)
    out[:bins] = np.bincount(_bin_index(v[counted], lo32, inv, bins), minlength=bins).astype(np.uint64)
    out[bins] = np.uint64(int(zero.sum()))
    return out


def zero_bin(lo, hi, bins):
    """The bin the binning rule gives the value 0 (where the exact-zero word belongs when a histogram is folded)."""
    lo32, inv = _f32_span(lo, hi, bins)
    return int(_bin_index(np.zeros(1, dtype=np.float32), lo32, inv, bins)[0])


def bin_centres(lo, hi, bins):
    """float64 value a non-zero bin stands for: lo + (k + 0.5) (hi - lo) / bins."""
    return float(lo) + (np.arange(bins, dtype=np.float64) + 0.5) * (float(hi) - float(lo)) / bins


def _mmse_error(v, w, r_min, r_max):
    scale, zp = affine_params(r_min, r_max)
    e = dequantize(quantize(v, scale, zp), scale, zp) - v
    return float(np.dot(w, e * e))


def mmse_objective(hist, lo, hi, r_min, r_max):
    """sum count * (dequantize(quantize(v)) - v)^2 of a histogram under affine_params(r_min, r_max); the zero word stands
    for the value 0."""
    hist = np.asarray(hist)
    v = np.append(bin_centres(lo, hi, hist.size - 1), 0.0)
    return _mmse_error(v, hist.astype(np.float64), r_min, r_max)


def _kl_objective(h, centres, r_min, r_max):
    """KL(P || Q) of the folded histogram h clipped to [r_min, r_max]; None when fewer than KL_MIN_BINS bins are kept."""
    keep = np.nonzero((centres >= r_min) & (centres <= r_max))[0]
    if keep.size < KL_MIN_BINS:
        return None
    first, last = int(keep[0]), int(keep[-1])
    own = h[first:last + 1]
    p = own.copy()
    p[0] += h[:first].sum()
    p[-1] += h[last + 1:].sum()
    total = p.sum()
    if total <= 0:
        return 0.0
    scale, zp = affine_params(r_min, r_max)
    code = quantize(centres[first:last + 1], scale, zp).astype(np.int64)
    code -= code.min()
    live = p > 0
    mass = np.bincount(code, weights=own)
    members = np.bincount(code, weights=live.astype(np.float64))
    q = (mass[code] / np.maximum(members[code], 1.0))[live]
    if np.any(q <= 0):          # mass beyond an end whose code holds none of the kept mass: nothing to model it with
        return float("inf")
    pn = p[live] / total
    return float(np.sum(pn * np.log(pn / (q / q.sum()))))


def range_from_histogram(hist, lo, hi, algorithm, steps=64):
    """(r_min, r_max) for affine_params from a histogram (histogram_model layout) taken over [lo, hi).

    'normal': (lo, hi).  Otherwise the candidates (a / steps * lo', b / steps * hi'), a, b = 1 .. steps, of the span
    widened to contain 0 (an end that is 0 keeps its factor at 1) are scored and the best is returned, ties going to the
    wider candidate (larger b, then larger a):
      'mmse'           sum count * (dequantize(quantize(v)) - v)^2, every non-zero bin standing for its centre and
                       the zero word for 0;
      'kl_divergence'  sum_{P>0} p log(p / q): the zero word is added to the bin that contains 0; P is the histogram over
                       the bins whose centres lie inside the candidate, mass outside added to the first / last kept
                       bin; Q groups the kept bins by their int8 code and spreads each group's own mass - the kept
                       bins' counts, before the outside mass went to P's edges - evenly over its bins with P > 0; both
                       normalised; candidates that keep fewer than KL_MIN_BINS bins are skipped, and one whose edge
                       code holds none of the kept mass while mass lies beyond it scores +inf.  (Q is built from the
                       kept counts, as in the published entropy calibration, so that clipping costs something: built
                       from P, every candidate of at most 256 kept bins has one bin per code, Q = P and KL = 0, and
                       at 2048 bins the search then returns an eighth of the span.)
    The result lies within [min(lo, 0), max(hi, 0)] and contains 0."""
    if algorithm not in ALGORITHMS:
        raise ValueError(f"algorithm={algorithm!r}: one of {ALGORITHMS}")
    if algorithm == "normal":
        return float(lo), float(hi)
    hist = np.asarray(hist)
    bins = hist.size - 1
    _f32_span(lo, hi, bins)
    lo_w, hi_w = min(float(lo), 0.0), max(float(hi), 0.0)
    centres = bin_centres(lo, hi, bins)
    if algorithm == "mmse":
        used = np.nonzero(hist[:bins])[0]               # the zero word's own error is 0 under every candidate
        v, w = centres[used], hist[used].astype(np.float64)

        def objective(r_min, r_max):
            return _mmse_error(v, w, r_min, r_max)
    else:
        h = hist[:bins].astype(np.float64)
        h[zero_bin(lo, hi, bins)] += float(hist[bins])

        def objective(r_min, r_max):
            return _kl_objective(h, centres, r_min, r_max)
    best, best_range = None, (lo_w, hi_w)
    for b in (range(steps, 0, -1) if hi_w > 0 else (steps,)):          # widest first: a tie keeps what it has
        for a in (range(steps, 0, -1) if lo_w < 0 else (steps,)):
            cand = (a / steps * lo_w, b / steps * hi_w)
            score = objective(*cand)
            if score is not None and (best is None or score < best):
                best, best_range = score, cand
    return best_range


def conv_units(features):
    """(state_dict prefix, conv index, bn index, input tensor, output tensor) of the 3x3 conv units in forward order."""
    d = len(features)
    units = []
    for l in range(d):
        src = "input" if l == 0 else f"cat{l - 1}.pool"
        units.append((f"encoder_blocks.{l}", 0, 1, src, f"enc{l}.a"))
        units.append((f"encoder_blocks.{l}", 3, 4, f"enc{l}.a", f"cat{l}"))
    units.append(("bottleneck", 0, 1, f"cat{d - 1}.pool", "bott.a"))
    units.append(("bottleneck", 3, 4, "bott.a", "bott.b"))
    for j in range(d):
        l = d - 1 - j
        units.append((f"decoder_blocks.{2 * j + 1}", 0, 1, f"cat{l}", f"dec{j}.a"))
        units.append((f"decoder_blocks.{2 * j + 1}", 3, 4, f"dec{j}.a", f"dec{j}.b"))
    return units


def quantize_model(state_dict, ranges, input_mean=INPUT_MEAN, input_std=INPUT_STD, hybrid=()):
    """Float state_dict + calibrated activation ranges {tensor name: (r_min, r_max)} -> quantised model: a flat dict
    of numpy arrays (int8 weights, int32 zero points / biases, float32 multipliers) keyed '<unit>.<field>', the unit
    names being the reference's state_dict prefixes ('encoder_blocks.0.0', 'decoder_blocks.0', 'output', ...).

    hybrid: unit keys (a subset of unit_names) that run in fp16 (hybrid quantisation, see the section below).  Each
    adds '<key>.hybrid', '.w_h', '.gain', '.bias_f', '.x_scale' (and keeps '.y_scale'); its int8 arrays stay, so the
    same dict runs as pure int8.  ValueError for an unknown key or a tensor that would be stored as fp16 with a
    calibrated range beyond +-HYBRID_RANGE_LIMIT.  With hybrid=() the dict is what it was before hybrid units existed."""
    feats = []
    while f"encoder_blocks.{len(feats)}.0.weight" in state_dict:
        feats.append(int(np.asarray(state_dict[f"encoder_blocks.{len(feats)}.0.weight"]).shape[0]))
    d = len(feats)
    q = {"features": np.asarray(feats, dtype=np.int32)}
    tq = {}
    for name in tensor_names(d):
        lo, hi = ranges[name]
        tq[name] = affine_params(lo, hi)
    for l in range(d):                      # a max-pooled tensor keeps its source's parameters
        tq[f"cat{l}.pool"] = tq[f"cat{l}"]

    # input: (u8 - mean) / std -> int8 through a table per channel
    s_in, z_in = tq["input"]
    lut = np.empty((3, 256), dtype=np.int8)
    for c in range(3):
        lut[c] = quantize((np.arange(256, dtype=np.float64) - input_mean[c]) / input_std[c], s_in, z_in)
    q["input.lut"] = lut
    q["input.zp"] = np.int32(z_in)
    q["input.scale"] = np.float32(s_in)

    def put_unit(key, w_q, w_s, w_z, b_fold, xname, yname, relu):
        s_x, z_x = tq[xname]
        q[key + ".w_q"] = w_q
        q[key + ".w_zp"] = w_z.astype(np.int32)
        q[key + ".w_scale"] = w_s.astype(np.float32)
        q[key + ".bias_q"] = np.rint(np.asarray(b_fold, dtype=np.float64) / (s_x * w_s)).astype(np.int64).clip(
            -2**31, 2**31 - 1).astype(np.int32)
        q[key + ".x_zp"] = np.int32(z_x)
        if yname is not None:
            s_y, z_y = tq[yname]
            q[key + ".mult"] = (s_x * w_s / s_y).astype(np.float32)
            q[key + ".y_zp"] = np.int32(z_y)
            q[key + ".y_scale"] = np.float32(s_y)
        else:
            q[key + ".mult"] = (s_x * w_s).astype(np.float32)      # head: real-valued logits
        q[key + ".relu"] = np.int32(1 if relu else 0)

    for prefix, ci, bi, xname, yname in conv_units(feats):
        w_fold, b_fold = fold_bn(state_dict, prefix, ci, bi)
        w_q, w_s, w_z = quantize_weight_per_channel(w_fold, axis=0)
        put_unit(f"{prefix}.{ci}", w_q, w_s, w_z, b_fold, xname, yname, True)
    for j in range(d):
        l = d - 1 - j
        w = np.asarray(state_dict[f"decoder_blocks.{2 * j}.weight"], dtype=np.float64)      # (I, O, 2, 2)
        b = np.asarray(state_dict[f"decoder_blocks.{2 * j}.bias"], dtype=np.float64)
        w_q, w_s, w_z = quantize_weight_per_channel(w, axis=1)
        src = "bott.b" if j == 0 else f"dec{j - 1}.b"
        put_unit(f"decoder_blocks.{2 * j}", w_q, w_s, w_z, b, src, f"cat{l}", False)
    w = np.asarray(state_dict["output.weight"], dtype=np.float64)
    w_q, w_s, w_z = quantize_weight_per_channel(w, axis=0)
    put_unit("output", w_q, w_s, w_z, np.asarray(state_dict["output.bias"], dtype=np.float64), f"dec{d - 1}.b", None,
             False)
    if len(hybrid):
        _put_hybrid(q, state_dict, ranges, feats, tq, hybrid)
    return q


# ---- hybrid quantisation: chosen units run in fp16 (README.md:3466-3474 "mixed precision"; with every unit named it
# is the table's "NPU FP16" row, README.md:3386-3393) --------------------------------------------------------------
# Semantics, stated once (csrc/conv_h16.h computes it in fp32, hybrid_forward_model / unit_model in float64):
#   * weights of a hybrid unit: the BatchNorm-folded float64 weights (plain weights for the transposed convolutions
#     and the head) divided per output channel by the power-of-two gain g[co] = 2^ceil(log2 max|w[co]|) (1 for an
#     all-zero channel) and rounded to IEEE fp16: '.w_h';
#   * operand: from an int8 tensor x = q - x_zp (an integer of magnitude <= 255, exact in fp16), from an fp16 tensor the
#     stored value; positions outside the image contribute exactly 0;
#   * a = sum w16 x in fp32 (every product is exact); v = a m[co] + b[co] in fp32 with m = g x_scale for an int8
#     input and m = g for an fp16 input, b the folded bias as float32; ReLU where the int8 unit has it;
#   * into an int8 tensor: clamp(rint(v / y_scale) + y_zp, lo, 127) with the int8 unit's lo; into an fp16 tensor:
#     fp16(min(v, 65504)), round to nearest even; the head writes v as float32 logits;
#   * a tensor is fp16 iff every unit that writes it and every unit that reads it is hybrid (tensor_dtypes); 'input'
#     is always int8, and every int8 tensor keeps its calibrated (scale, zero_point).
HYBRID_RANGE_LIMIT = 60000.0        # an fp16 tensor's calibrated range must stay inside +-this (fp16 max: 65504)
FP16_MAX = 65504.0


def unit_table(features):
    """(key, kind, input tensor, output tensor or None, relu) of every unit in forward order; kind is 'conv', 'up' or
    'head'."""
    d = len(features)
    conv = [(f"{p}.{ci}", "conv", x, y, True) for p, ci, _, x, y in conv_units(features)]
    units = conv[:2 * d + 2]
    for j in range(d):
        src = "bott.b" if j == 0 else f"dec{j - 1}.b"
        units.append((f"decoder_blocks.{2 * j}", "up", src, f"cat{d - 1 - j}", False))
        units += conv[2 * d + 2 + 2 * j:2 * d + 4 + 2 * j]
    units.append(("output", "head", f"dec{d - 1}.b", None, False))
    return units


def unit_names(features):
    """Keys of the units of quantize_model in forward order: what `hybrid=` takes."""
    return [u[0] for u in unit_table(features)]


def _check_hybrid(features, hybrid):
    names = unit_names(features)
    hybrid = set(hybrid)
    unknown = sorted(hybrid - set(names))
    if unknown:
        raise ValueError(f"hybrid: unknown unit(s) {unknown}; the units are {names}")
    return hybrid


def tensor_dtypes(features, hybrid):
    """{activation tensor: 'int8' | 'fp16'} for tensor_names plus the pooled tensors 'cat<l>.pool'.  A tensor is fp16
    iff every unit that writes it and every unit that reads it is in `hybrid`; cat<l> and cat<l>.pool are one tensor for
    this rule (max-pooling is type agnostic; cat<l> has two writers and, through the pool, two readers); 'input' is
    always int8 (it comes from the 256-entry table)."""
    hybrid = _check_hybrid(features, hybrid)
    d = len(features)
    users = {}
    for key, _, x, y, _ in unit_table(features):
        for t in (x, y):
            if t is not None:
                users.setdefault(t.replace(".pool", ""), []).append(key)
    out = {}
    for name in tensor_names(d) + [f"cat{l}.pool" for l in range(d)]:
        base = name.replace(".pool", "")
        out[name] = "fp16" if base != "input" and all(u in hybrid for u in users[base]) else "int8"
    return out


def hybrid_units(qmodel):
    """The hybrid units a quantised model carries, in forward order."""
    feats = [int(f) for f in qmodel["features"]]
    return [k for k in unit_names(feats) if k + ".hybrid" in qmodel and int(qmodel[k + ".hybrid"])]


def hybrid_weights(w, axis=0):
    """float64 weights -> (w / g rounded to fp16, g): per-output-channel power-of-two gain (output channels on `axis`)."""
    w = np.asarray(w, dtype=np.float64)
    amax = np.abs(np.moveaxis(w, axis, 0).reshape(w.shape[axis], -1)).max(axis=1)
    g = np.ones_like(amax)
    g[amax > 0] = 2.0 ** np.ceil(np.log2(amax[amax > 0]))
    shape = [1] * w.ndim
    shape[axis] = -1
    return (w / g.reshape(shape)).astype(np.float16), g


def _put_hybrid(q, state_dict, ranges, feats, tq, hybrid):
    hybrid = _check_hybrid(feats, hybrid)
    for name, dt in tensor_dtypes(feats, hybrid).items():
        lo, hi = ranges[name.replace(".pool", "")]
        if dt == "fp16" and max(abs(float(lo)), abs(float(hi))) > HYBRID_RANGE_LIMIT:
            raise ValueError(f"hybrid: tensor {name!r} would be stored as fp16 but its calibrated range ({lo}, {hi}) "
                             f"is beyond +-{HYBRID_RANGE_LIMIT:g}")
    folded = {f"{p}.{ci}": fold_bn(state_dict, p, ci, bi) for p, ci, bi, _, _ in conv_units(feats)}
    for key, kind, xname, yname, _ in unit_table(feats):
        if key not in hybrid:
            continue
        if kind == "conv":
            w, b = folded[key]
        else:
            w = np.asarray(state_dict[key + ".weight"], dtype=np.float64)
            b = np.asarray(state_dict[key + ".bias"], dtype=np.float64)
        w16, g = hybrid_weights(w, axis=1 if kind == "up" else 0)
        q[key + ".hybrid"] = np.int32(1)
        q[key + ".w_h"] = np.ascontiguousarray(w16).view(np.uint16)
        q[key + ".gain"] = g.astype(np.float32)
        q[key + ".bias_f"] = np.asarray(b, dtype=np.float64).astype(np.float32)
        q[key + ".x_scale"] = np.float32(tq[xname][0])
        if yname is not None:
            q[key + ".y_scale"] = np.float32(tq[yname][0])


def _conv_f64(kind, x, w):
    """float64 convolution of a unit: x (N,C,H,W); w (O,C,3,3) for 'conv', (I,O,2,2) for 'up', (K,C,1,1) for 'head'.
    Zero padding: positions outside the image contribute exactly 0."""
    import torch
    import torch.nn.functional as F
    xt, wt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)), torch.from_numpy(
        np.ascontiguousarray(w, dtype=np.float64))
    if kind == "up":
        return F.conv_transpose2d(xt, wt, stride=2).numpy()
    return F.conv2d(xt, wt, padding=1 if kind == "conv" else 0).numpy()


def unit_model(qmodel, key, x):
    """One unit of a quantised model on a given input tensor, in float64 (the GPU tests feed it the device's own input).

    x: (N,C,H,W); an int8 array is an int8 tensor (codes), any float array an fp16 tensor (its stored values); for a
    decoder's first convolution it is the whole concat tensor.  Returns a dict:
      'dtype'   'int8' | 'fp16' | 'fp32' (the head): how the unit's output is stored (tensor_dtypes of the model's set)
      'y'       the stored output by this model: int8 codes, fp16 values (as float32) or float32 logits ((N,K,H,W) for
                a head of K rows)
    and for a hybrid unit also
      'v'       a m + b in float64 with the fp16-rounded weights, after the ReLU where the unit has one: unrounded
      'S'       m sum |w16| |x| + |b| per output element: what the rounding errors of the fp32 evaluation scale with
      'K'       the real GEMM depth (taps x input channels)
    A unit that is not hybrid is evaluated by the integer rule of the module header (int8 in, int8 out / logits)."""
    feats = [int(f) for f in qmodel["features"]]
    unit = {u[0]: u for u in unit_table(feats)}
    if key not in unit:
        raise ValueError(f"unknown unit {key!r}")
    _, kind, _, yname, relu = unit[key]
    x = np.asarray(x)
    x_int8 = x.dtype == np.int8
    ydt = "fp32" if yname is None else tensor_dtypes(feats, hybrid_units(qmodel))[yname]
    bshape = (1, -1, 1, 1)
    if not (key + ".hybrid" in qmodel and int(qmodel[key + ".hybrid"])):
        if not x_int8 or ydt == "fp16":
            raise ValueError(f"{key} is not hybrid: its tensors are int8")
        ax = 1 if kind == "up" else 0
        wsh = [1, 1, 1, 1]
        wsh[ax] = -1
        wz = qmodel[key + ".w_q"].astype(np.float64) - np.asarray(qmodel[key + ".w_zp"], dtype=np.float64).reshape(wsh)
        acc = np.rint(_conv_f64(kind, x.astype(np.float64) - float(qmodel[key + ".x_zp"]), wz)).astype(np.int64)
        t = (acc + np.asarray(qmodel[key + ".bias_q"], dtype=np.int64).reshape(bshape)).astype(np.float32)
        t = t * np.asarray(qmodel[key + ".mult"], dtype=np.float32).reshape(bshape)
        if yname is None:
            return {"dtype": "fp32", "y": t.astype(np.float32)}
        zy = int(qmodel[key + ".y_zp"])
        y = np.clip(np.rint(t).astype(np.int64) + zy, zy if relu else QMIN, QMAX).astype(np.int8)
        return {"dtype": "int8", "y": y}
    w16 = np.asarray(qmodel[key + ".w_h"]).view(np.float16).astype(np.float64)
    m = np.asarray(qmodel[key + ".gain"], dtype=np.float32).astype(np.float64)
    if x_int8:
        xv = x.astype(np.float64) - float(qmodel[key + ".x_zp"])
        m = m * float(np.float32(qmodel[key + ".x_scale"]))
    else:
        xv = x.astype(np.float64)
    b = np.asarray(qmodel[key + ".bias_f"], dtype=np.float32).astype(np.float64)
    v = _conv_f64(kind, xv, w16) * m.reshape(bshape) + b.reshape(bshape)
    big = _conv_f64(kind, np.abs(xv), np.abs(w16)) * m.reshape(bshape) + np.abs(b).reshape(bshape)
    if relu:
        v = np.maximum(v, 0.0)
    k = int(xv.shape[1]) * (9 if kind == "conv" else 1)
    out = {"dtype": ydt, "v": v, "S": big, "K": k}
    if ydt == "int8":
        zy, sy = int(qmodel[key + ".y_zp"]), float(np.float32(qmodel[key + ".y_scale"]))
        out["y"] = np.clip(np.rint(v / sy) + zy, zy if relu else QMIN, QMAX).astype(np.int8)
    elif ydt == "fp16":
        out["y"] = np.minimum(v, FP16_MAX).astype(np.float16).astype(np.float32)
    else:
        out["y"] = v.astype(np.float32)
    return out


def hybrid_bound(out, y_scale=None):
    """Per-element bound of |device - model| for a hybrid unit's unit_model result `out`: gamma = (K + 3) 2^-24 S is the
    first-order worst case of an fp32 sum of K exact products plus the epilogue's roundings.  int8 output (codes, against
    clip(v / y_scale + y_zp, lo, 127)): 0.5 + gamma / y_scale; fp16 output: gamma + 2^-11 |v| + 2^-25 (the storage
    rounding and half the smallest subnormal); float32 logits: gamma."""
    gamma = (out["K"] + 3) * 2.0 ** -24 * out["S"]
    if out["dtype"] == "int8":
        return 0.5 + gamma / float(y_scale)
    if out["dtype"] == "fp16":
        return gamma + 2.0 ** -11 * np.abs(out["v"]) + 2.0 ** -25
    return gamma


def hybrid_forward_model(qmodel, frames, taps=None):
    """The forward of a quantised model with its hybrid units, in float64 with the fp16-rounded weights (unit_model on
    every unit; max-pooling and the concat on stored values).  frames: (N,H,W,3) uint8.  Returns (logits float32
    (N,K,H,W) - K = 1 for the reference's head -, {unit key: {'v', 'S', 'K'}} for the hybrid units).  taps, if a dict, receives every stored tensor by
    name."""
    feats = [int(f) for f in qmodel["features"]]
    d = len(feats)
    f = np.asarray(frames)
    lut = np.asarray(qmodel["input.lut"])
    t = {"input": np.stack([lut[c][f[..., c]] for c in range(3)], axis=1).astype(np.int8)}
    info = {}
    logits = None
    for key, kind, xname, yname, _ in unit_table(feats):
        if xname.endswith(".pool") and xname not in t:
            src = t[xname[:-5]][:, :feats[int(xname[3:-5])]]
            n, c, h, w = src.shape
            t[xname] = src.reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5))
        out = unit_model(qmodel, key, t[xname])
        if "v" in out:
            info[key] = {k: out[k] for k in ("v", "S", "K")}
        if yname is None:
            logits = out["y"]
        elif yname.startswith("cat"):                       # skip half first, the transposed convolution's behind it
            t[yname] = out["y"] if kind == "conv" else np.concatenate([t[yname], out["y"]], axis=1)
        else:
            t[yname] = out["y"]
    if taps is not None:
        taps.update(t)
    return logits, info


def out_channels(qmodel):
    """1 for the reference's lane head, K for a K-class quantised model: the entries of output.bias_q"""
    return int(np.asarray(qmodel["output.bias_q"]).size)


def save_quantized(path, qmodel):
    """One .npz of the model's arrays; a K-class model's head arrays keep their K rows."""
    np.savez_compressed(path, **qmodel)


def load_quantized(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
