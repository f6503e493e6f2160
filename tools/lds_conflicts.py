#!/usr/bin/env python3
"""ds_read_b128 bank-conflict count of the r512 kernels' pixel-operand reads (csrc/conv_x3_r512.h); --blocks: of the third
structure's 4 x 4-block fragments (csrc/conv_x3_t448.h); --q8: of the q-plane reads (csrc/conv_q8_r512.h); --wino: of the
Winograd raw-tile reads (csrc/wino_f32.h); --i8: of the int8 tier's pixel reads (csrc/conv_i8.h); --dec: of the composed
decoder step's parity fragments (csrc/conv_x3_dec.h).

A tile is TH x TWX pixels = 14 fragments of 16 consecutive pixels in row-major order; lane (li = lane & 15, lq = lane >> 4)
of fragment f reads 16 bytes of LDS pixel position pos = (i // TWX) * P + i % TWX + ky * P + kx (i = 16 f + li) at byte
address pos * 64 + ((lq ^ (((pos >> 2) & 1) << 1)) << 4).  ds_read_b128 is served in four 16-lane groups, one LDS cycle
each when the 16 lanes hit 16 distinct 16-byte slots of the 256-byte bank row (MI355X_MICROARCH.md, LDS): 4 cycles per
read is conflict free.  Prints (mean, worst) cycles per read over all fragments and taps for candidate pitches P."""
GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
          list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
          list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
          list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


def analyze(twx, pitch, npf=14):
    tot = worst = n = 0
    for f in range(npf):
        for ky in range(3):
            for kx in range(3):
                cyc = 0
                for g in GROUPS:
                    slots = {}
                    for lane in g:
                        li, lq = lane & 15, lane >> 4
                        i = 16 * f + li
                        pos = (i // twx) * pitch + i % twx + ky * pitch + kx
                        addr = pos * 64 + ((lq ^ (((pos >> 2) & 1) << 1)) << 4)
                        slots.setdefault((addr // 16) % 16, set()).add(addr)
                    cyc += max(len(v) for v in slots.values())
                tot += cyc
                n += 1
                worst = max(worst, cyc)
    return tot / n, worst


def analyze_q8(twx, pitch, npf=14):
    """The q-plane reads of csrc/conv_q8_r512.h: lane (li, lq) reads 32 contiguous bytes of a pixel as two ds_read_b128 -
    half (lq & 1) of the pixel's 64 bytes, 16-byte part r = 0, 1 at physical part (2 (lq & 1) + r) ^ ((pos >> 2) & 1) - and
    the lanes lq >= 2 read the step's second tap: one row down (steps 0-2), one column right (step 3), the zero slot
    (step 4)."""
    steps = [((0, 0), pitch), ((0, 1), pitch), ((0, 2), pitch), ((2, 0), 1), ((2, 2), None)]
    tot = worst = n = 0
    for f in range(npf):
        for (ky, kx), off in steps:
            for r in (0, 1):
                cyc = 0
                for g in GROUPS:
                    slots = {}
                    for lane in g:
                        li, lq = lane & 15, lane >> 4
                        i = 16 * f + li
                        pos = (i // twx) * pitch + i % twx + ky * pitch + kx
                        if lq >= 2:
                            pos = None if off is None else pos + off
                        if pos is None:
                            addr = (1 << 20) + ((2 * (lq & 1) + r) << 4)
                        else:
                            addr = pos * 64 + (((2 * (lq & 1) + r) ^ ((pos >> 2) & 1)) << 4)
                        slots.setdefault((addr // 16) % 16, set()).add(addr)
                    cyc += max(len(v) for v in slots.values())
                tot += cyc
                n += 1
                worst = max(worst, cyc)
    return tot / n, worst


def analyze_blocks(pitch, ncb=7, nrb=4):
    """The pixel-operand reads of csrc/conv_x3_t448.h: a fragment is a 4 x 4 block of pixels (lane li = pixel (li >> 2,
    li & 3) of block (rb, cb)), byte address (r * pitch + c) * 64 + ((lq ^ ((r & 1) << 1)) << 4) with (r, c) the halo
    position of the lane's pixel at tap (ky, kx): the swizzle depends on the halo row's parity only."""
    tot = worst = n = 0
    for rb in range(nrb):
        for cb in range(ncb):
            for ky in range(3):
                for kx in range(3):
                    cyc = 0
                    for g in GROUPS:
                        slots = {}
                        for lane in g:
                            li, lq = lane & 15, lane >> 4
                            r = 4 * rb + (li >> 2) + ky
                            c = 4 * cb + (li & 3) + kx
                            addr = (r * pitch + c) * 64 + ((lq ^ ((r & 1) << 1)) << 4)
                            slots.setdefault((addr // 16) % 16, set()).add(addr)
                        cyc += max(len(v) for v in slots.values())
                    tot += cyc
                    n += 1
                    worst = max(worst, cyc)
    return tot / n, worst


def analyze_wino(tht, twt, key):
    """The raw-tile patch reads of csrc/wino_f32.h: lane (li, lq) of wave w holds Winograd tile tb = 16 w + li of a tht x twt
    grid and reads patch pixel (i, j): halo row hr = 2 (tb // twt) + i, record s = tb % twt + (j >> 1) of half row (j & 1),
    16-byte part PERM[lq] ^ key(s) with PERM = {0, 3, 1, 2}."""
    perm = (0, 3, 1, 2)
    rw = 2 * twt + 2
    tot = worst = n = 0
    for wave in range(8):
        for i in range(4):
            for j in range(4):
                cyc = 0
                for g in GROUPS:
                    slots = {}
                    for lane in g:
                        li, lq = lane & 15, lane >> 4
                        tb = wave * 16 + li
                        if tb >= tht * twt:
                            continue
                        tr, tc = divmod(tb, twt)
                        s = tc + (j >> 1)
                        addr = (((2 * tr + i) * rw + (j & 1) * (rw // 2) + s) * 4 + (perm[lq] ^ key(s))) * 16
                        slots.setdefault((addr // 16) % 16, set()).add(addr)
                    cyc += max([len(v) for v in slots.values()] or [1])
                tot += cyc
                n += 1
                worst = max(worst, cyc)
    return tot / n, worst


def analyze_i8(cin, pad, taps):
    """The pixel-operand reads of csrc/conv_i8.h: fragment f = tile row f of an 18-wide halo tile (taps 9) or 16
    consecutive pixels (taps 1), lane (li, lq) reads 16 bytes at pixel * (cin + pad) + 16 lq + 64 chunk; cin 32 (pair
    layout): 16 (lq & 1) of the pixel at tap min(2 step + (lq >> 1), 8)."""
    pitch = cin + pad
    tot = worst = n = 0
    for f in range(8):
        for t in range(5 if cin == 32 else taps):
            for kc in range(max(1, cin // 64)):
                cyc = 0
                for g in GROUPS:
                    slots = {}
                    for lane in g:
                        li, lq = lane & 15, lane >> 4
                        if cin == 32:
                            tp = min(2 * t + (lq >> 1), 8)
                            addr = (f * 18 + li + (tp // 3) * 18 + tp % 3) * pitch + (lq & 1) * 16
                        elif taps == 9:
                            addr = (f * 18 + li + (t // 3) * 18 + t % 3) * pitch + lq * 16 + kc * 64
                        else:
                            addr = (f * 16 + li) * pitch + lq * 16 + kc * 64
                        slots.setdefault((addr // 16) % 16, set()).add(addr)
                    cyc += max(len(v) for v in slots.values())
                tot += cyc
                n += 1
                worst = max(worst, cyc)
    return tot / n, worst


def analyze_dec(half, pitch, swz):
    """The reads of csrc/conv_x3_dec.h: a fragment is 16 pixels of one parity class (a, b), lane li = (li >> 1, li & 1)
    of an 8 x 2 block of that class.  half "skip": high-resolution halo position (2 (li >> 1) + a + ky, 2 (li & 1) + 4 cb
    + b + kx); half "x": low-resolution (li >> 1) + a + di, (li & 1) + 2 cb + b + dj.  Byte address (r * pitch + c) * 64 +
    ((lq ^ swz(r)) << 4)."""
    tot = worst = n = 0
    taps = [(ky, kx) for ky in range(3) for kx in range(3)] if half == "skip" else [(d, e) for d in range(2) for e in range(2)]
    for a in range(2):
        for b in range(2):
            for cb in range(7):
                for ty, tx in taps:
                    cyc = 0
                    for g in GROUPS:
                        slots = {}
                        for lane in g:
                            li, lq = lane & 15, lane >> 4
                            if half == "skip":
                                r, c = 2 * (li >> 1) + a + ty, 2 * (li & 1) + 4 * cb + b + tx
                            else:
                                r, c = (li >> 1) + a + ty, (li & 1) + 2 * cb + b + tx
                            addr = (r * pitch + c) * 64 + ((lq ^ swz(r)) << 4)
                            slots.setdefault((addr // 16) % 16, set()).add(addr)
                        cyc += max(len(v) for v in slots.values())
                    tot += cyc
                    n += 1
                    worst = max(worst, cyc)
    return tot / n, worst


if __name__ == "__main__":
    import sys
    if "--i8" in sys.argv:
        for cin in (32, 64, 128, 256):
            for taps in ((9,) if cin == 32 else (9, 1)):
                for pad in (0, 16, 32, 48):
                    mean, worst = analyze_i8(cin, pad, taps)
                    print(f"int8 tier, {cin:3d} channels, {taps} tap(s), pad {pad:2d} bytes: {mean:.2f} cycles per read (worst {worst})" +
                          ("   <- conflict free" if worst == 4 else ""))
        sys.exit(0)
    if "--dec" in sys.argv:
        swzs = (("2 (r & 1)", lambda r: 2 * (r & 1)), ("2 ((r >> 1) & 1)", lambda r: 2 * ((r >> 1) & 1)))
        for half, pitches in (("skip", (30, 32, 34)), ("x", (16, 17, 18))):
            for p in pitches:
                for name, swz in swzs:
                    mean, worst = analyze_dec(half, p, swz)
                    print(f"decoder parity fragments, {half:4s} half, pitch {p:2d}, part ^ {name}: {mean:.2f} cycles per read "
                          f"(worst {worst})" + ("   <- conflict free" if worst == 4 else ""))
        sys.exit(0)
    if "--wino" in sys.argv:
        for tht, twt, where in ((16, 8, "224 x 224, 112 x 112"), (9, 14, "56 x 56, 28 x 28"), (18, 7, "14 x 14")):
            for name, key in (("rounds 1-3: (s >> 2) & 3", lambda s: (s >> 2) & 3), ("round 4: ((s >> 2) & 1) << 1", lambda s: ((s >> 2) & 1) << 1)):
                mean, worst = analyze_wino(tht, twt, key)
                print(f"Winograd raw tile, {tht:2d} x {twt:2d} tile grid ({where}), key {name}: {mean:.2f} cycles per read (worst {worst})")
        sys.exit(0)
    if "--blocks" in sys.argv:
        for ncb, pitches in ((7, (30, 32, 34, 36)), (8, (34, 36, 38, 40))):
            for p in pitches:
                mean, worst = analyze_blocks(p, ncb)
                print(f"4 x 4 blocks, {4 * ncb:2d}-wide tile, pitch {p:2d}: {mean:.2f} cycles per read (worst {worst})" +
                      ("   <- conflict free" if worst == 4 else ""))
        sys.exit(0)
    if "--q8" in sys.argv:
        for twx, pitches in ((28, (30, 32, 36, 40)), (14, (16, 18, 20, 22, 24))):
            for p in pitches:
                mean, worst = analyze_q8(twx, p)
                print(f"q plane, TWX {twx:2d} pitch {p:2d}: {mean:.2f} cycles per read (worst {worst})" +
                      ("   <- conflict free" if worst == 4 else ""))
        sys.exit(0)
    for twx, pitches in ((28, (30, 32, 36, 40, 44)), (14, (16, 18, 20, 22, 24)), (32, (34, 36, 40)), (16, (18, 20, 22)),
                         (8, (10, 12, 14, 16, 18, 20))):
        for p in pitches:
            mean, worst = analyze(twx, p)
            print(f"TWX {twx:2d} pitch {p:2d}: {mean:.2f} cycles per read (worst {worst})" + ("   <- conflict free" if worst == 4 else ""))
