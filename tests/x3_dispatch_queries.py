"""Queries for the f16x3 dispatch's host hooks (unet_host_plan_conv3x3_x3, unet_host_plan_upconv2x2_x3; the layouts are
in include/unet_hip.h), shared by tests/test_x3_dispatch_cpu.py, the GPU operator tests, which hold every launch's
path_out against the plan, and tests/golden/make_golden_x3_dispatch.py.  No torch, no device."""
import ctypes as C
import os

SPLIT_FLOATS = 256 * 256 * 64          # kSplitFloats: the forward's split-K scratch
SWITCHES_ON = (1, 1, 1, 1)             # UNET_X3_FLAT, UNET_X3_R512, UNET_X3_T448, UNET_X3_T448_C4
N_CONV_PLAN, N_UPCONV_PLAN = 24, 16
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


def ask(lib, kind, query):
    """-> (plan ints, label) from the host hook; raises on a refused query"""
    n_plan = N_CONV_PLAN if kind == "conv" else N_UPCONV_PLAN
    fn = lib.unet_host_plan_conv3x3_x3 if kind == "conv" else lib.unet_host_plan_upconv2x2_x3
    q = (C.c_int * len(query))(*query)
    plan = (C.c_int * n_plan)()
    label = C.create_string_buffer(64)
    rc = fn(q, len(query), plan, n_plan, label, 64)
    if rc != 0:
        raise ValueError((kind, query, rc))
    return list(plan), label.value.decode()


