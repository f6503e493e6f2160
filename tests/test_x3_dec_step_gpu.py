"""The f16x3 decoder step's plan against a real forward: model A, batch 1, 224 x 224.  The profiler labels of the decoder's
launches must be the ones x3_plan_dec_step gives for the four levels (through unet_host_plan_dec_step_x3) - deep, deep,
composed, composed in the forward's order with unet_set_x3_compose(1), the two kernels everywhere with (0) - and the
two modes' logits must agree to the 1e-4 of tests/test_x3_compose_gpu.py."""
import os

import pytest
import torch

from unet_lane_detection_amd import state as S
from x3_dispatch_queries import (COMPOSED, DEEP, FINISH_PASS, TWO_KERNEL, VALID, ask, conv_query, dec_step_query,
                                 switches_from_env)

pytestmark = pytest.mark.gpu

FEATURES = (64, 128, 256, 512)


@pytest.fixture(scope="module")
def lib():
    from unet_lane_detection_amd import _lib
    return _lib.load(build_if_missing=False)


@pytest.fixture(scope="module")
def modelA():
    from unet_lane_detection_amd.model import UNetHIP
    m = UNetHIP(S.seeded_state_dict(seed=0), device=0)
    yield m
    m.release()


def _decoder_labels(lib, n, size, compose):
    """-> (forms, labels) of the decoder's launches in the forward's order: per level the step, then its second convolution"""
    sw = switches_from_env()
    forms, labels = [], []
    for lv in reversed(range(len(FEATURES))):
        f, low = FEATURES[lv], size >> (lv + 1)
        step, names = ask(lib, "dec", dec_step_query(
            n, low, low, f, compose=compose, switches=sw, deep=0 if os.environ.get("UNET_X3_COMPOSE_DEEP", "")[:1] == "0" else 1,
            dec_form=int(os.environ.get("UNET_X3_DEC_FORM", "-1")), upconv_mode=0 if os.environ.get("UNET_X3_UPCONV_R512", "")[:1] == "0" else -1))
        forms.append(step[0])
        labels += names.split(",")
        head = lv == 0
        plan, name = ask(lib, "conv", conv_query(n, 2 * low, 2 * low, f, f, 2, switches=sw) if head else
                         conv_query(n, 2 * low, 2 * low, f, f, 0, split=1, switches=sw))
        assert plan[VALID] == 1
        labels += [name] + (["splitk_finish_f16x3"] if plan[FINISH_PASS] else [])
    return forms, labels


def test_forward_launches_what_the_step_plan_names(lib, modelA):
    n, size = 1, 224
    frames = torch.from_numpy(S.synthetic_frames(n, seed=5)).cuda().contiguous()
    logits = {}
    prev = lib.unet_set_x3_compose(-1)
    try:
        for mode, want_forms in ((1, [DEEP, DEEP, COMPOSED, COMPOSED]), (0, [TWO_KERNEL] * 4)):
            lib.unet_set_x3_compose(mode)
            forms, want = _decoder_labels(lib, n, size, mode)
            assert forms == want_forms, mode
            modelA.profile(True)
            logits[mode] = modelA.run_u8(frames, precision="f16x3").clone()
            names = [r[0] for r in modelA.profile_records()]
            modelA.profile(False)
            assert modelA.device_error() == 0
            assert names[-len(want):] == want, (mode, names)
            # nothing of the decoder in front of that tail: its kernels appear nowhere else in the forward
            assert not any(nm.startswith(("upconv2x2", "upcat_conv3x3", "conv3x3_t448add")) for nm in names[:-len(want)]), names
    finally:
        modelA.profile(False)
        lib.unet_set_x3_compose(prev)
    assert (logits[1] - logits[0]).abs().max().item() < 1e-4
