"""The f16x3 tier's dispatch on the CPU: x3_plan_conv / x3_plan_upconv / x3_plan_dec_step (csrc/unet_x3.inc; DESIGN.md,
"f16x3 dispatch") through the host hooks unet_host_plan_conv3x3_x3 / unet_host_plan_upconv2x2_x3 /
unet_host_plan_dec_step_x3.  No device is touched.

What the plan is held to was not produced by the plan: the path tuples the GPU operator tests assert against real
launches, the per-layer labels of two recorded batch-256 runs, and two tables generated from the decision code as it was
before it became a plan (tests/golden/x3_dispatch.json, x3_dec_step.json; tests/golden/make_golden_x3_*.py regenerate
them)."""
import ctypes as C
import json
import os
import sys

import pytest

import test_train_x3_ops_gpu as TT
import test_x3_ops_gpu as TX
from unet_lane_detection_amd import _lib
from x3_dispatch_queries import (COMPOSED, DEEP, GRID, PATH, STAT_ROWS, TWO_KERNEL, VALID, ask, conv_query, dec_step_query,
                                 upconv_query)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_x3_dispatch as G  # noqa: E402
import make_golden_x3_dec_step as GD  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def plan_path(lib, query):
    plan, _ = ask(lib, "conv", query)
    assert plan[VALID] == 1, query
    return tuple(plan[PATH])


# ---- the paths the GPU tests assert against real launches ---------------------------------------------------------------

CONV_TABLES = [("ws", TX.WS_CASES, 0), ("r512", TX.R512_CASES, 0), ("t448", TX.T448_CASES, 0), ("splitk", TX.SPLITK_CASES, 1),
               ("auto", TX.AUTO_CASES, 1)]


@pytest.mark.parametrize("table", CONV_TABLES, ids=[t[0] for t in CONV_TABLES])
def test_plan_gives_the_paths_of_the_gpu_case_tables(lib, table):
    _, rows, split = table
    for name, n, h, w, cin, cout, tw, pool, modes, want in rows:
        for mode in modes:              # ldo modes of conv_and_check: 2 = at channel offset cout
            q = conv_query(n, h, w, cin, cout, 1 if pool else 0, tile_width=tw, co_off=cout if mode == 2 else 0, split=split)
            assert plan_path(lib, q) == tuple(want), (name, mode)


def test_plan_gives_the_paths_of_the_fused_head_cases(lib):
    for name, n, h, w, cin, tw, want in TX.HEAD_CASES:
        assert plan_path(lib, conv_query(n, h, w, cin, 64, 2, tile_width=tw)) == tuple(want), name


def test_plan_without_scratch_does_not_split(lib):
    name, n, h, w, cin, cout, tw, pool, modes, want = TX.SPLITK_CASES[0]
    assert plan_path(lib, conv_query(n, h, w, cin, cout, 0)) == (TX.WS, 16, 0, 0, 1, 0, 0)


def test_plan_gives_the_paths_of_the_training_case_table(lib):
    for name, n, h, w, cin, cout, mode, tw, want in TT.TCONV_CASES:
        cin_op, cout_op = (cout, cin) if mode else (cin, cout)
        for off in (cout_op, 0):
            q = conv_query(n, h, w, cin_op, cout_op, 3, tile_width=tw, co_off=off)
            assert plan_path(lib, q) == (want[0], want[1], 3, want[2], 1, want[3], 0), name


def test_plan_gives_the_fused_statistics_rows_of_the_training_cases(lib):
    for name, n, h, w, cout, tw, want, want_rows in TT.STAT_CASES:
        plan, _ = ask(lib, "conv", conv_query(n, h, w, 64, cout, 3, tile_width=tw, stats=1))
        assert tuple(plan[PATH]) == (want[0], want[1], 3, want[2], 1, want[3], 0), name
        if want[0] == TX.WS:
            assert plan[STAT_ROWS] == 0, name
        else:
            assert 0 < plan[STAT_ROWS] <= 1024 and (want_rows is None or plan[STAT_ROWS] == want_rows), name
        without, _ = ask(lib, "conv", conv_query(n, h, w, 64, cout, 3, tile_width=tw))
        assert without[STAT_ROWS] == 0 and without[PATH] == plan[PATH], name


def test_plan_gives_the_structures_of_the_upconv_cases(lib):
    for name, n, h, w, cin, cout, mode, want_st, want_ab in TX.UPCONV_CASES:
        plan, _ = ask(lib, "upconv", upconv_query(n, h, w, cin, cout, co_off=cout, mode=mode))
        assert plan[VALID] == 1 and plan[0] == want_st and plan[5] == want_ab, name


# ---- the labels of two recorded batch-256 runs ----------------------------------------------------------------------------

def recorded_layer_labels(path):
    """the per-launch labels of a `bench.py --layers` record, in launch order"""
    labels = []
    with open(path) as f:
        for line in f:
            t = line.split()
            if len(t) >= 3 and t[2] == "ms":
                labels.append(t[0])
    return labels


@pytest.mark.parametrize("compose", ["on", "off"])
def test_plan_labels_equal_the_recorded_batch_256_run(lib, compose):
    """model A, batch 256, 224 x 224, fp8 tier off.  With the composed decoder on, a recorded upcat row stands for the
    transposed convolution and the decoder's first convolution of that step: the step's plan says which (the deep
    switch off: the recordings predate the deep form)."""
    want = recorded_layer_labels(os.path.join(HERE, "..", "profiles", "r05", f"layers_batch256_compose_{compose}.txt"))
    assert want[0] == "conv3x3_first_f16x3" and len(want) == (22 if compose == "off" else 20)
    n, size = 256, 224
    got, k = [], 1

    def conv_label(hh, ww, cin, cout, epi):
        q = conv_query(n, hh, ww, cin, cout, epi) if epi == 2 else conv_query(n, hh, ww, cin, cout, epi, split=1)
        plan, label = ask(lib, "conv", q)
        assert plan[VALID] == 1
        return label

    for name, hh, ww, cin, cout, epi in G.network_layers(size, size):
        if name.startswith("dec") and name.endswith("conv1"):
            step, labels = ask(lib, "dec", dec_step_query(n, hh // 2, ww // 2, cout, compose=-1 if compose == "on" else 0, deep=0))
            if step[0] == COMPOSED:
                assert compose == "on" and cout <= 128, name
                got += labels.split(",")
                k += 1
                continue
            assert step[0] == TWO_KERNEL
            plan, label = ask(lib, "upconv", upconv_query(n, hh // 2, ww // 2, cin, cout, co_off=cout))
            assert plan[VALID] == 1
            got.append(label)
            k += 1
            assert labels.split(",") == [label, conv_label(hh, ww, cin, cout, epi)], name
        got.append(conv_label(hh, ww, cin, cout, epi))
        k += 1
    assert got == want[1:]
    assert sum(lb == "upcat_conv3x3_dec_f16x3" for lb in want) == (2 if compose == "on" else 0)


# ---- the table from the decision code before it became a plan ---------------------------------------------------------------

def test_plan_reproduces_the_dispatch_table(lib):
    with open(G.TABLE) as f:
        table = json.load(f)
    queries = G.sweep()
    assert (len(queries), G.queries_digest(queries)) == (table["queries"], table["queries_sha256"]) and \
        len(table["rows"]) == len(queries), "the table's queries are not the sweep's: regenerate it on purpose"
    structures = set()
    for (kind, q), k in zip(queries, table["rows"]):
        want = table["plans"][k]
        plan, label = ask(lib, kind, q)
        assert [kind, *plan[:G.STORED[kind]], label] == want, (kind, q)
        structures.add((kind, plan[0], plan[4] > 1))
        if kind == "conv" and plan[VALID]:      # the geometry the kernel gets is consistent with the grid
            n_, h_, img_h, tx, ty, pix, co_t, co_g, chunks, ks = plan[14:24]
            items = pix * co_t * ks
            assert pix == n_ * ty * tx and n_ * h_ == q[0] * q[1] and img_h == q[1] and chunks * ks == q[3] // 32 and co_t % co_g == 0
            assert plan[GRID] == max(8, min(256, items // 8 * 8)) or (q[16] and plan[0] == TX.T448 and plan[GRID] % co_t == 0)
    # the sweep reaches every family of both dispatches, split-K and the refusals
    assert structures >= {("conv", 1, False), ("conv", 1, True), ("conv", 2, False), ("conv", 3, False), ("conv", 4, False),
                          ("conv", 0, False), ("upconv", 1, False), ("upconv", 2, False), ("upconv", 0, False)}


def test_plan_reproduces_the_decoder_step_table(lib):
    with open(GD.TABLE) as f:
        table = json.load(f)
    queries = GD.sweep()
    assert (len(queries), G.queries_digest(queries)) == (table["queries"], table["queries_sha256"]) and \
        len(table["rows"]) == len(queries), "the table's queries are not the sweep's: regenerate it on purpose"
    forms = set()
    for q, k in zip(queries, table["rows"]):
        plan, labels = ask(lib, "dec", q)
        assert [*plan, labels] == table["plans"][k], q
        forms.add((plan[0], q[8]))
        n_labels = len(labels.split(","))
        assert n_labels == plan[7] if plan[0] != TWO_KERNEL else n_labels >= 2, q
        if plan[0] == COMPOSED:             # the geometry the kernel gets is consistent with the grid
            wco, tx, ty, pix, co_t, grid = plan[1:7]
            assert pix == q[0] * ty * tx and co_t * 64 * wco == q[3] and grid == max(8, min(256, pix * co_t // 8 * 8)), q
    # the sweep reaches every form from both askers (an entry point is never handed the two kernels' launches, only told)
    assert forms == {(form, who) for form in (TWO_KERNEL, COMPOSED, DEEP) for who in (0, 1)}


# ---- the forced form ----------------------------------------------------------------------------------------------------------

# tile_width -> (structure, tile width, waves) the form must run with, on a shape that fits every form of its family
FORCED = {16: (1, 16, 0), 32: (1, 32, 0), 28: (2, 28, 1), 14: (2, 14, 1), 228: (2, 28, 2), 214: (2, 14, 2), 332: (2, 32, 1),
          316: (2, 16, 1), 308: (2, 8, 1), 532: (2, 32, 2), 428: (4, 28, 1), 414: (4, 14, 1), 628: (3, 28, 2), 632: (3, 32, 1),
          728: (3, 28, 4)}


def test_every_legal_tile_width_decodes_to_its_form(lib):
    assert sorted(FORCED) == [14, 16, 28, 32, 214, 228, 308, 316, 332, 414, 428, 532, 628, 632, 728]
    for tw, (st, tile, waves) in FORCED.items():
        w = 14 if tile == 14 else 224          # 224 = 8 * 28 = 7 * 32: every other tile width divides it
        plan, label = ask(lib, "conv", conv_query(1, 16, w, 64, 256, 0, tile_width=tw, q8=1 if st == 4 else 0))
        assert plan[VALID] == 1 and (plan[0], plan[1], plan[5]) == (st, tile, waves), (tw, plan)
        assert label.startswith({1: "conv3x3_ws_f16x3_tw", 2: "conv3x3_r512_f16x3_t", 3: "conv3x3_t448_f16x3_t",
                                 4: "conv3x3_q8_f16q8_t"}[st] + str(tile)), (tw, label)
    plan, _ = ask(lib, "conv", conv_query(1, 16, 224, 64, 256, 0))
    assert plan[VALID] == 1


def test_every_other_tile_width_is_refused(lib):
    plan = (C.c_int * 24)()
    for tw in range(1000):
        if tw == 0 or tw in FORCED:
            continue
        q = conv_query(1, 16, 224, 64, 256, 0, tile_width=tw)
        rc = lib.unet_host_plan_conv3x3_x3((C.c_int * 22)(*q), 22, plan, 24, None, 0)
        assert rc == 1, tw                 # UNET_ERR_INVALID_ARG


def test_a_forced_form_that_does_not_fit_is_invalid_and_never_the_first_structure(lib):
    for tw, (st, tile, waves) in FORCED.items():
        if st == 1:
            continue
        plan, label = ask(lib, "conv", conv_query(1, 10, 33, 64, 256, 0, tile_width=tw, split=1, q8=1))   # W = 33: no tile divides it
        assert plan == [0] * 24 and label == "", tw
