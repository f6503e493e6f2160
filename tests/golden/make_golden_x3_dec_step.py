"""Regenerates tests/golden/x3_dec_step.json from the library's host hook unet_host_plan_dec_step_x3: run it when the
decoder step's dispatch (x3_plan_dec_step, csrc/unet_x3.inc) is changed ON PURPOSE, and review the diff of the table.

    python tests/golden/make_golden_x3_dec_step.py [out.json [library.so]]

The table holds, for every query of sweep(), the plan and the step's profiler labels (distinct answers once, one index
per query; the queries are sweep()'s, pinned by their count and digest).  tests/test_x3_dispatch_cpu.py asserts that the
hook reproduces it row by row.  The sweep: model A's four decoder levels at batches 1, 2, 4, 8, 16, 64 and 256, at
224 x 224, 640 x 640 and 176 x 224; compose modes -1, 0, 1; the deep switch on and off; dec-form modes -1, 1, 2; f16q8
scratch absent and present; asked by the forward and by an operator entry point (the latter holding both operators, the
composed one alone, the deep one alone).

The committed table was not produced by x3_plan_dec_step.  It comes from the decision code as it was before it became a
plan: on a copy of that commit, the composed and the deep form's launch functions (each held its own rules between
argument filling and the launch) returned their geometry in front of their launches, a
temporary hook with this hook's layouts called them in the order forward_x3 did (the composed operator where no f16q8
scratch is held, then the deep form, with the operators x3_build or the entry points built) and took the two-kernel
labels from the queries run_upconv_x3 / run_conv_x3 make; `library.so` pointed this script at that build."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden_x3_dispatch import BATCHES, FEATURES, SIZES, dump, queries_digest  # noqa: E402
from x3_dispatch_queries import COMPOSED, DEEP, N_DEC_PLAN, ask, dec_step_query  # noqa: E402

TABLE = os.path.join(HERE, "x3_dec_step.json")


def decoder_levels(h, w):
    """(f, low-resolution height, width of x) of model A's decoder steps, in the forward's order"""
    return [(f, h >> (lv + 1), w >> (lv + 1)) for lv, f in reversed(list(enumerate(FEATURES)))]


def sweep():
    """-> list of query ints, in a fixed order"""
    rows = []
    for h, w in SIZES:
        for n in BATCHES:
            for f, lh, lw in decoder_levels(h, w):
                for compose in (-1, 0, 1):
                    for deep in (1, 0):
                        for dec_form in (-1, 1, 2):
                            for q8 in (0, 1):
                                for entry, have in ((0, COMPOSED | DEEP), (1, COMPOSED | DEEP), (1, COMPOSED), (1, DEEP)):
                                    rows.append(dec_step_query(n, lh, lw, f, compose=compose, deep=deep, dec_form=dec_form,
                                                               q8=q8, entry=entry, have=have))
    return rows


def encode(answers):
    """answers: [(plan ints, labels)] in sweep() order -> the table: distinct answers once, one index per query"""
    plans, index, rows = [], {}, []
    for plan, label in answers:
        key = (*plan, label)
        if key not in index:
            index[key] = len(plans)
            plans.append(list(key))
        rows.append(index[key])
    return plans, rows


def main(out, library=None):
    if library:
        lib = C.CDLL(library)       # another build that exports a hook of this name and these layouts
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
        from unet_lane_detection_amd import _lib
        lib = _lib.load(build_if_missing=False)
    queries = sweep()
    plans, rows = encode([ask(lib, "dec", q) for q in queries])
    assert all(len(p) == N_DEC_PLAN + 1 for p in plans)
    dump(dict(queries=len(queries), queries_sha256=queries_digest(queries), plans=plans, rows=rows), out)
    print("wrote", out, len(queries), "queries,", len(plans), "distinct answers")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else TABLE, *sys.argv[2:3])
