"""The launch sequence of the training handle, per branch of its forward walk and backward pass (csrc/unet_train.inc):
the ordered profiler labels of one forward_backward and one eval_logits per case equal the recorded lists of
tests/golden/train_sequence.json (tests/golden/make_golden_train_sequence.py: the cases, and how to regenerate the file
when the sequence is changed on purpose).  The profiler forces the weight gradients in line; the side-stream modes are
tied to that order bit for bit by test_train_gpu.py::test_side_stream_weight_gradients_are_bit_identical."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_train_sequence as G  # noqa: E402


@pytest.fixture(scope="module")
def table():
    with open(G.TABLE) as f:
        return json.load(f)["cases"]


def _same(got, want, name):
    for key in ("train", "eval"):
        g, w = got[key], want[key]
        first = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
        assert g == w, f"case {name}, {key}: {len(g)} launches against {len(w)} recorded; first difference at {first}: " \
                       f"{g[first:first + 3]} against {w[first:first + 3]}"


def test_golden_file_is_well_formed(table):
    assert set(table) == set(G.CASES) | set(G.ENV_CASES)
    for name, rec in table.items():
        assert set(rec) == {"train", "eval"}, name
        for key in ("train", "eval"):
            assert rec[key] and all(isinstance(x, str) and x for x in rec[key]), (name, key)
    # both passes walk the same network: 2 units per level, 2 in the bottleneck, 2 per decoder step
    a = table["a"]
    n_train = sum(x.startswith("conv3x3") for x in a["train"])
    n_eval = sum(x.startswith("eval_conv3x3") for x in a["eval"])
    assert n_train == n_eval == 2 * (2 * len(G.CASES["a"]["feats"]) + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(G.CASES))
def test_launch_sequence_is_the_recorded_one(table, case):
    _same(G.record(case), table[case], case)


@pytest.mark.gpu
def test_launch_sequence_with_the_fusions_switched_off(table):
    """UNET_TRAIN_POOL_FUSED=0 and UNET_TRAIN_FUSED_STATS=0 are read once per process: case a in one fresh child process
    each, one after the other; the first failure ends the test."""
    for name in sorted(G.ENV_CASES):
        _same(G.record_in_child(name, timeout=300), table[name], name)
