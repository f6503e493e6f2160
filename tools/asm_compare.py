#!/usr/bin/env python3
"""Compare two sets of device-only assembly listings of the library, kernel by kernel.

    hipcc <build.py's FLAGS without -shared> --cuda-device-only -S -o parent/NAME.s NAME.cpp
        (at each commit, for each NAME.cpp of build.py's SOURCES: one listing per source)
    python tools/asm_compare.py parent this [--only SUBSTRING] [--all]
    python tools/asm_compare.py parent/unet_hip.cpp.s this/unet_hip.cpp.s,this/launch_conv_x3_ws.cpp.s

A side is a comma-separated list of listings and of directories of listings (*.s), all taken together; a kernel symbol
that occurs in more than one listing of a side is an error (the library would carry it in two code objects).

Per kernel symbol: whether the text is identical, the register / spill / scratch figures of both builds from the
metadata, and, where the text differs, the instruction totals and the mnemonics whose counts differ.  Text and counts
only; the __hip_cuid_* symbol (a per-build id) is ignored.  Exit status 1 if a kernel exists in one listing only or a
figure of the second listing is above the first's (ABOVE) or the count of a mnemonic of one of CLASSES differs (CLASS)."""
import argparse
import collections
import glob
import os
import re
import sys

FIGURES = (".vgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size")
# instruction classes whose counts a refactor of the device code must leave alone: matrix, LDS, memory, lane exchange,
# accumulator-file moves, barriers
CLASSES = ("v_mfma", "ds_", "buffer_", "global_", "scratch_", "v_permlane", "v_accvgpr", "s_barrier")


def parse(path):
    """{kernel symbol: [instruction lines]}, {kernel symbol: {figure: value}}"""
    text = open(path).read()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    bodies, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_$.][\w$.]*):", line)
        if m and not m.group(1).startswith((".L", "__hip_cuid")):
            cur = m.group(1) if m.group(1) in kernels else None
            if cur:
                bodies[cur] = []
            continue
        # block labels carry the function's ordinal in the module (.LBB<function>_<block>): a kernel added ahead of this one
        # renumbers them without touching the text
        s = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip())
        if cur and s.startswith(".Lfunc_end"):
            cur = None
        elif cur and s and not s.startswith(".") or cur and s.startswith(".L"):
            bodies[cur].append(s)
    figures = {}
    # amdhsa.kernels metadata as this compiler writes it: one YAML entry per kernel, keys in alphabetical order, so that
    # "- .agpr_count:" opens every entry.  An entry without one of FIGURES is an error here, not a zero.  (.sgpr_count and
    # the LDS size are not compared: the first is not what limits these kernels, the second is set by the shape structs.)
    for blk in re.split(r"^\s*- \.agpr_count:", text, flags=re.M)[1:]:
        blk = ".agpr_count:" + blk
        sym = re.search(r"^\s*\.symbol:\s+(\S+)\.kd", blk, re.M)
        vals = {k: re.search(r"^\s*" + re.escape(k) + r":\s+(\d+)", blk, re.M) for k in FIGURES}
        if sym is None or None in vals.values():
            missing = [k for k, v in vals.items() if v is None] or [".symbol"]
            raise SystemExit(f"{path}: a kernel's metadata entry lacks {missing}: not the layout this script knows")
        figures[sym.group(1)] = {k: int(v.group(1)) for k, v in vals.items()}
    if set(figures) != set(bodies):
        raise SystemExit(f"{path}: {len(bodies)} kernel bodies but {len(figures)} metadata entries")
    return bodies, figures


def parse_side(side):
    """parse() over the listings of one side, merged; a kernel in two of them ends the run"""
    bodies, figures, where = {}, {}, {}
    paths = []
    for item in side.split(","):
        paths += sorted(glob.glob(os.path.join(item, "*.s"))) if os.path.isdir(item) else [item]
    for path in paths:
        b, f = parse(path)
        twice = sorted(set(b) & set(bodies))
        if twice:
            raise SystemExit("\n".join(f"TWICE: {k} in {where[k]} and {path}" for k in twice))
        bodies.update(b)
        figures.update(f)
        where.update(dict.fromkeys(b, path))
    return bodies, figures


def mnemonics(body):
    return collections.Counter(s.split()[0] for s in body if not s.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("first", help="listings and directories of listings, comma-separated")
    ap.add_argument("second")
    ap.add_argument("--only", default="", help="kernels whose symbol contains this")
    ap.add_argument("--all", action="store_true", help="list the identical kernels too")
    args = ap.parse_args()
    (b0, f0), (b1, f1) = parse_side(args.first), parse_side(args.second)
    bad = sorted(set(b0) ^ set(b1))
    for k in bad:
        print(f"ONLY IN {'first' if k in b0 else 'second'}: {k}")
    same = differ = 0
    for k in sorted(set(b0) & set(b1)):
        if args.only not in k:
            continue
        ident = b0[k] == b1[k]
        same, differ = same + ident, differ + (not ident)
        above = [n for n in FIGURES if f1[k][n] > f0[k][n]]
        m0, m1 = mnemonics(b0[k]), mnemonics(b1[k])
        d = {m: (m0[m], m1[m]) for m in sorted(set(m0) | set(m1)) if m0[m] != m1[m]}
        if any(m.startswith(CLASSES) for m in d):
            above.append("CLASS")
        if above:
            bad.append(k)
        if ident and not above and not args.all:
            continue
        print(f"{'identical' if ident else 'DIFFERENT'} {k}")
        print("    " + "  ".join(f"{n[1:]} {f0[k][n]}/{f1[k][n]}" for n in FIGURES) + ("   FAILS: " + ",".join(above) if above else ""))
        if not ident:
            print(f"    instructions {sum(m0.values())}/{sum(m1.values())}  " + "  ".join(f"{m} {a}/{b}" for m, (a, b) in d.items()))
    print(f"{same} identical, {differ} different, {len(bad)} with a kernel missing, a figure above the first listing's or a class count changed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
