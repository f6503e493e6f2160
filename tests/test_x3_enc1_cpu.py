"""The plan of the f16x3 tier's fused first encoder block (csrc/conv_x3_enc1.h) on the CPU: x3_plan_enc1
(csrc/unet_x3.inc) through the host hook unet_host_plan_enc1_x3.  No device is touched.

The fused kernel stands for exactly one pair of launches - uint8 frames into conv_first_x3.h, then the 64-channel form of
conv_x3_t448.h with the pooled epilogue on 16 x 28 tiles - so the plan takes the block exactly where the dispatch's own
answer for the second convolution (unet_host_plan_conv3x3_x3) is that form, and nowhere else."""
import ctypes as C

import pytest

from unet_lane_detection_amd import _lib
from x3_dispatch_queries import GRID, PATH, SPLIT_FLOATS, SWITCHES_ON, VALID, ask, conv_query

T448 = 3
THE_FORM = (T448, 28, 1, 0, 1, 1, 0)     # structure 3, 28-wide tiles, pooled epilogue, per image, no split-K, one wave along the channels


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def enc1_query(n, h, w, *, u8=1, cout=64, tile_width=0, q8=0, on=1, switches=SWITCHES_ON):
    return [u8, n, h, w, cout, tile_width, q8, on, *switches, q8]


def ask_enc1(lib, query):
    q = (C.c_int * len(query))(*query)
    plan = (C.c_int * 8)()
    assert lib.unet_host_plan_enc1_x3(q, len(query), plan, 8) == 0, query
    return list(plan)


def conv2_plan(lib, n, h, w, *, tile_width=0, q8=0, switches=SWITCHES_ON):
    """the dispatch's own answer for the block's second convolution as the forward asks it"""
    q = conv_query(n, h, w, 64, 64, 1, tile_width=tile_width, split=1, q8=q8, switches=switches)
    assert q[9] == SPLIT_FLOATS
    return ask(lib, "conv", q)[0]


def test_plan_takes_the_headline_batch(lib):
    plan = ask_enc1(lib, enc1_query(256, 224, 224))
    c2 = conv2_plan(lib, 256, 224, 224)
    assert c2[VALID] == 1 and tuple(c2[PATH]) == THE_FORM
    # the fused launch runs on the second convolution's tiles and grid: 256 images x 14 x 8 tiles of 16 x 28 pixels
    assert plan == [1, c2[GRID], 8, 14, 256 * 14 * 8, 0, 0, 0]
    assert plan[1] == 256


def test_plan_declines_fp32_input(lib):
    assert ask_enc1(lib, enc1_query(256, 224, 224, u8=0)) == [0] * 8


def test_plan_declines_32_wide_tiles(lib):
    c2 = conv2_plan(lib, 64, 640, 640)
    assert c2[VALID] == 1 and c2[PATH][0] == T448 and c2[PATH][1] == 32     # the third structure, but on 16 x 32 tiles
    assert ask_enc1(lib, enc1_query(64, 640, 640)) == [0] * 8


def test_plan_declines_where_the_second_convolution_lands_elsewhere(lib):
    # a single frame: 112 work items, fewer than half of the CUs - the dispatch keeps the layer off the third structure
    c2 = conv2_plan(lib, 1, 224, 224)
    assert c2[VALID] == 1 and c2[PATH][0] != T448
    assert ask_enc1(lib, enc1_query(1, 224, 224)) == [0] * 8
    # ... and batch 2 is the smallest that lands on it
    assert tuple(conv2_plan(lib, 2, 224, 224)[PATH]) == THE_FORM
    assert ask_enc1(lib, enc1_query(2, 224, 224))[0] == 1
    # the third structure switched off (UNET_X3_T448=0)
    assert ask_enc1(lib, enc1_query(256, 224, 224, switches=(1, 1, 0, 1))) == [0] * 8
    # forced onto the first structure
    assert ask_enc1(lib, enc1_query(256, 224, 224, tile_width=32)) == [0] * 8


def test_plan_declines_with_the_switch_off(lib):
    assert ask_enc1(lib, enc1_query(256, 224, 224, on=0)) == [0] * 8


def test_plan_declines_with_the_q8_scratch(lib):
    assert ask_enc1(lib, enc1_query(256, 224, 224, q8=1)) == [0] * 8


def test_plan_declines_other_widths_of_the_block(lib):
    assert ask_enc1(lib, enc1_query(256, 224, 224, cout=128)) == [0] * 8


def test_forced_form_takes_a_single_tile(lib):
    """what the operator entry point asks: the third structure forced (tile_width 628), however few the work items"""
    assert ask_enc1(lib, enc1_query(1, 16, 28, tile_width=628)) == [1, 8, 1, 1, 1, 0, 0, 0]
    assert ask_enc1(lib, enc1_query(3, 40, 56, tile_width=628)) == [1, 16, 2, 3, 18, 0, 0, 0]
    assert ask_enc1(lib, enc1_query(1, 16, 30, tile_width=628)) == [0] * 8     # no whole 28-wide tiles


def test_hook_refuses_malformed_queries(lib):
    plan = (C.c_int * 8)()
    q = enc1_query(256, 224, 224)
    assert lib.unet_host_plan_enc1_x3((C.c_int * 12)(*q[:12]), 12, plan, 8) != 0
    assert lib.unet_host_plan_enc1_x3((C.c_int * 13)(*q), 13, plan, 7) != 0
    bad = list(q)
    bad[5] = 5     # a tile_width outside the table
    assert lib.unet_host_plan_enc1_x3((C.c_int * 13)(*bad), 13, plan, 8) != 0
    assert lib.unet_set_x3_fuse_first(lib.unet_set_x3_fuse_first(0)) == 0     # the setter returns the previous setting
