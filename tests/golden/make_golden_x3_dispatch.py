"""Regenerates tests/golden/x3_dispatch.json from the library's host hooks (unet_host_plan_conv3x3_x3,
unet_host_plan_upconv2x2_x3): run it when the f16x3 dispatch is changed ON PURPOSE, and review the diff of the table.

    python tests/golden/make_golden_x3_dispatch.py [out.json]

The table holds, for every query of sweep(), the plan and the profiler label (distinct answers once, one index per query;
the queries themselves are sweep()'s, pinned by their count and digest).  tests/test_x3_dispatch_cpu.py asserts that the
hooks reproduce it row by row.  The sweep: model A (features 64 / 128 / 256 / 512, bottleneck 1024) at batches 1, 2, 4,
8, 16, 64 and 256, at 224 x 224, 640 x 640 and 176 x 224 (level heights 44, 22, 11: no multiples of 8); every layer of the
network as the forward calls it, with the f16q8 tier off (split-K scratch present and absent) and on with its scratch and
every way the q planes can be linked; the training forms (fp32 epilogue with and without statistics, the input gradient
with cin and cout swapped); the transposed convolutions and the backward pass's plain GEMMs; no forced width."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from x3_dispatch_queries import ask, conv_query, upconv_query  # noqa: E402

TABLE = os.path.join(HERE, "x3_dispatch.json")
FEATURES = (64, 128, 256, 512)
BATCHES = (1, 2, 4, 8, 16, 64, 256)
SIZES = ((224, 224), (640, 640), (176, 224))


def network_layers(h, w):
    """(name, level height, level width, cin, cout, epilogue asked for) of model A's 3x3 convolutions behind the first one"""
    layers = []
    for lv, f in enumerate(FEATURES):
        hh, ww = h >> lv, w >> lv
        if lv > 0:
            layers.append((f"enc{lv + 1}.conv1", hh, ww, f // 2, f, 0))
        layers.append((f"enc{lv + 1}.conv2", hh, ww, f, f, 1))
    d = len(FEATURES)
    fb = 2 * FEATURES[-1]
    layers.append(("bott.conv1", h >> d, w >> d, fb // 2, fb, 0))
    layers.append(("bott.conv2", h >> d, w >> d, fb, fb, 0))
    for lv in reversed(range(d)):
        f = FEATURES[lv]
        hh, ww = h >> lv, w >> lv
        layers.append((f"dec{d - lv}.conv1", hh, ww, 2 * f, f, 0))
        layers.append((f"dec{d - lv}.conv2", hh, ww, f, f, 2 if lv == 0 else 0))
    return layers


def sweep():
    """-> list of ("conv" | "upconv", query ints), without duplicates, in a fixed order"""
    rows, seen = [], set()

    def add(kind, q):
        key = (kind, tuple(q))
        if key not in seen:
            seen.add(key)
            rows.append((kind, q))

    for h, w in SIZES:
        for n in BATCHES:
            for _, hh, ww, cin, cout, epi in network_layers(h, w):
                if epi == 2:                       # the fused head is handed neither scratch
                    add("conv", conv_query(n, hh, ww, cin, cout, 2))
                    continue
                for split in (0, 1):
                    add("conv", conv_query(n, hh, ww, cin, cout, epi, split=split))
                links = ([dict(), dict(pool_src_q=1, pool_dst_q=1), dict(pool_dst_q=1), dict(in_q=1, pool_dst_q=1)] if epi == 1 else
                         [dict(), dict(out_q=1), dict(in_q=1), dict(in_q=1, out_q=1)])
                for link in links:
                    add("conv", conv_query(n, hh, ww, cin, cout, epi, split=1, q8=1, **link))
                # training: forward with and without fused statistics, input gradient (cout -> cin)
                add("conv", conv_query(n, hh, ww, cin, cout, 3, stats=1))
                add("conv", conv_query(n, hh, ww, cin, cout, 3))
                add("conv", conv_query(n, hh, ww, cout, cin, 3))
            for lv, f in enumerate(FEATURES):
                lh, lw = h >> (lv + 1), w >> (lv + 1)
                for out_q in (0, 1):
                    add("upconv", upconv_query(n, lh, lw, 2 * f, f, co_off=f, out_q=out_q))
                add("upconv", upconv_query(n, lh, lw, 4 * f, 2 * f, gemm=1))
    return rows


STORED = {"conv": 14, "upconv": 16}    # plan ints kept per row: path (7), grid, statistics rows, the three passes, outQ, valid
                                       # (+ pixTiles, coTiles of the transposed convolution); then the label


def queries_digest(rows):
    return hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()


def encode(answers):
    """answers: [(kind, plan ints, label)] in sweep() order -> the table: distinct answers once, one index per query"""
    plans, index, rows = [], {}, []
    for kind, plan, label in answers:
        key = (kind, *plan[:STORED[kind]], label)
        if key not in index:
            index[key] = len(plans)
            plans.append(list(key))
        rows.append(index[key])
    return plans, rows


def dump(table, path):
    """compact, a few long lines per key: the file is data for a test, not reading matter"""
    def wrapped(items):
        lines, cur = [], ""
        for it in items:
            t = json.dumps(it, separators=(",", ":"))
            if cur and len(cur) + len(t) > 150:
                lines.append(cur)
                cur = ""
            cur += ("," if cur else "") + t
        return "[\n" + ",\n".join(lines + [cur]) + "\n]"
    with open(path, "w") as f:
        f.write('{"queries":%d,"queries_sha256":"%s",\n"plans":%s,\n"rows":%s}\n'
                % (table["queries"], table["queries_sha256"], wrapped(table["plans"]), wrapped(table["rows"])))


def main(out):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from unet_lane_detection_amd import _lib
    lib = _lib.load(build_if_missing=False)
    queries = sweep()
    plans, rows = encode([(kind, *ask(lib, kind, q)) for kind, q in queries])
    dump(dict(queries=len(queries), queries_sha256=queries_digest(queries), plans=plans, rows=rows), out)
    print("wrote", out, len(queries), "queries,", len(plans), "distinct answers")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else TABLE)
