"""Queries for the f16x3 dispatch's host hooks (unet_host_plan_conv3x3_x3, unet_host_plan_upconv2x2_x3,
unet_host_plan_dec_step_x3; the layouts are in include/unet_hip.h), shared by tests/test_x3_dispatch_cpu.py, the GPU operator tests, which hold every launch's
path_out against the plan, and tests/golden/make_golden_x3_dispatch.py.  No torch, no device."""
import ctypes as C
import os

SPLIT_FLOATS = 256 * 256 * 64          # kSplitFloats: the forward's split-K scratch
SWITCHES_ON = (1, 1, 1, 1)             # UNET_X3_FLAT, UNET_X3_R512, UNET_X3_T448, UNET_X3_T448_C4
N_CONV_PLAN, N_UPCONV_PLAN, N_DEC_PLAN = 24, 16, 16
TWO_KERNEL, COMPOSED, DEEP = 0, 1, 2   # plan[0] of a decoder step; as bits 1 / 2: the operators an asker holds
PATH, GRID, STAT_ROWS, TO_Q8_PASS, POOL_PASS, FINISH_PASS, OUT_Q, VALID = slice(0, 7), 7, 8, 9, 10, 11, 12, 13


def switches_from_env():
    """the A/B switches as the library reads them from the environment of this process"""
    return tuple(0 if os.environ.get(name, "")[:1] == "0" else 1
                 for name in ("UNET_X3_FLAT", "UNET_X3_R512", "UNET_X3_T448", "UNET_X3_T448_C4"))


def conv_query(n, h, w, cin, cout, epi, *, tile_width=0, co_off=0, split=0, q8=0, in_q=0, out_q=0, pool_src_q=0, pool_dst_q=0,
               stats=0, switches=SWITCHES_ON):
    return [n, h, w, cin, cout, epi, tile_width, co_off, split, SPLIT_FLOATS if split else 0, q8, q8, in_q, out_q, pool_src_q,
            pool_dst_q, stats, *switches, q8]


def upconv_query(n, h, w, cin, cout, *, co_off=0, out_q=0, mode=-1, gemm=0):
    return [n, h, w, cin, cout, co_off, out_q, mode, gemm]


def dec_step_query(n, h, w, f, *, compose=-1, deep=1, dec_form=-1, q8=0, entry=0, have=COMPOSED | DEEP, window_only=0,
                   upconv_mode=-1, switches=SWITCHES_ON):
    """h, w: the low-resolution map of x"""
    return [n, h, w, f, compose, deep, dec_form, q8, entry, have, window_only, upconv_mode, *switches, q8]


def ask(lib, kind, query):
    """-> (plan ints, label) from the host hook ("dec": the step's labels, comma-separated); raises on a refused query"""
    n_plan = {"conv": N_CONV_PLAN, "upconv": N_UPCONV_PLAN, "dec": N_DEC_PLAN}[kind]
    fn = {"conv": lib.unet_host_plan_conv3x3_x3, "upconv": lib.unet_host_plan_upconv2x2_x3,
          "dec": lib.unet_host_plan_dec_step_x3}[kind]
    q = (C.c_int * len(query))(*query)
    plan = (C.c_int * n_plan)()
    label = C.create_string_buffer(128)
    rc = fn(q, len(query), plan, n_plan, label, 128)
    if rc != 0:
        raise ValueError((kind, query, rc))
    return list(plan), label.value.decode()
