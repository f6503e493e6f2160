// Split-operand ("f16x3") tier, the first encoder block as ONE kernel: enc1.conv1 (uint8 RGB frames -> normalise -> 3x3,
// 3 -> 64, + folded BN + ReLU; conv_first_x3.h) is computed per work item straight into the LDS halo image that
// enc1.conv2 (3x3, 64 -> 64, + folded BN + ReLU, planes + their 2 x 2 max-pool; conv_x3_t448.h's 64-channel form with the
// pooled epilogue) reads its input from.  The 64-channel tensor between the two layers is never stored: conv_first_x3's
// pass writes it as 2 x 128 bytes per pixel and the third structure reads it back by LDS-DMA; here an item reads 2 KB
// of uint8 instead of 138 KB of planes.
//
// Same arithmetic, packed weights and order of operations as the two kernels it stands for, so the planes and the pooled
// planes are THEIR bits (tests/test_x3_enc1_gpu.py):
//  * phase A, enc1.conv1 for the item's 18 x 30 halo pixels, 34 fragments of 16 consecutive halo pixels, 9 per wave
//    (waves 2 and 3 repeat fragment 33).  The operands come from a table of the item's 20 x 32 x 3 input bytes, each
//    normalised ((b - m) / s; 0 outside the image: the padding applies to the normalised tensor) and split into fp16
//    hi | lo (one 32-bit word per byte, looked up in the block's 3 x 256 table of normalised, split byte values).  Lane (li, lq) gathers k = 8 lq + [0, 8) of halo pixel li (k = 3 tap + ci,
//    27 .. 31 zero), the three MFMAs run in conv_first_x3's order on a zero accumulator, then fmaxf(fmaf(acc, scale,
//    shift), floor) and the hi / lo split.  A halo pixel outside the image (or below a ragged last tile's image) is 16
//    zero bytes in both planes: enc1.conv2's padding is of enc1.conv1's OUTPUT.  The lane's 16 channels 16 lq + [0, 16)
//    are parts 2 (lq & 1) and 2 (lq & 1) + 1 of chunk lq >> 1: two ds_write_b128 per plane at the swizzled position
//    part ^ ((haloRow & 1) << 1) of the third structure's halo image (pitch 30, 64 bytes per pixel and plane, chunk
//    buffers XST apart, lo plane XPL behind hi);
//  * phase B, the third structure's chunk loop over the two chunks, both resident: weights straight from L2 two taps
//    ahead in the ring of three, term and tap order unchanged, immediate-only read addresses; no LDS-DMA, no per-chunk
//    barrier, no buffer rotation;
//  * the third structure's pooled epilogue (EPI 1) as it is.
// Two barriers per item: after phase A, and after the last LDS read of phase B (the next item's table is written just
// before it: the table is only read in phase A).  The next item's byte loads go out after the first barrier and are in
// flight under phase B; enc1.conv2's first two taps of weights are asked for at the end of phase A.
//
// Needs uint8 input, Cout = 64 on both layers, W % 28 == 0, H and W even; any H (rows past the bottom are not stored).
#pragma once
#include "conv_x3_enc1_args.h"

namespace unet {

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv3x3_enc1_x3_kernel(
    const ConvEnc1X3Args a) {
  using E = X3Enc1Shape;
  using S = E::S;
  constexpr int P = S::P, CB = S::CB, NF = S::CB;   // 7 fragments of 4 x 4 pixels per wave (4 rows x 28 columns)

  extern __shared__ __attribute__((aligned(16))) f32x4 smemv[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int G = gridDim.x;   // multiple of 8 (wave_tile.h)
  const int lb = x3_logical_block(G);
  const int numWork = a.c.pixTiles;
  if (lb >= numWork) return;
  char* lds = reinterpret_cast<char*>(smemv);
  char* tbl = lds + E::TBL;

  struct Geo {
    int n, y0, x0;
  };
  auto geo_of = [&](int w) __attribute__((always_inline)) {
    Geo g;
    const int rowTile = w / a.c.tilesX;
    g.x0 = (w - rowTile * a.c.tilesX) * S::TWX;
    g.n = rowTile / a.c.tilesY;
    g.y0 = (rowTile - g.n * a.c.tilesY) * S::TH;
    return g;
  };

  // ---- the input patch: rows y0 - 2 .. y0 + 17, columns x0 - 2 .. x0 + 29; thread tid owns bytes it * 256 + tid.  A
  //      byte outside the image (or past the patch) is kept as ~0 ----
  auto load_patch = [&](const Geo& g, unsigned (&rawb)[E::N1]) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < E::N1; ++it) {
      const int i = it * 256 + tid;
      const int prow = i / (E::PC * 3), rem = i - prow * (E::PC * 3);
      const int pcol = rem / 3, ci = rem - pcol * 3;
      const int y = g.y0 - 2 + prow, x = g.x0 - 2 + pcol;
      rawb[it] = ~0u;
      if (i < E::NB && (unsigned)y < (unsigned)a.c.H && (unsigned)x < (unsigned)a.c.W)
        rawb[it] = a.frames[(((size_t)g.n * a.c.H + y) * a.c.W + x) * 3 + ci];
    }
  };
  // normalised and split once per block for every byte value and colour channel: hi in the low half of the word, lo in the
  // high half ((float)b - m) / s as conv_first_x3.h computes it); an item's table is then a lookup per input byte
  char* lut = tbl + E::NB * 4;
#pragma unroll
  for (int ci = 0; ci < 3; ++ci) {
    const float m = ci == 0 ? a.m0 : (ci == 1 ? a.m1 : a.m2);
    const float s = ci == 0 ? a.s0 : (ci == 1 ? a.s1 : a.s2);
    const float v = ((float)tid - m) / s;
    uint32_t h, l;
    split_pk_f16(v, 0.f, h, l);
    *reinterpret_cast<uint32_t*>(lut + (ci * 256 + tid) * 4) = (h & 0xffffu) | (l << 16);
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  auto stage_patch = [&](const unsigned (&rawb)[E::N1]) __attribute__((always_inline)) {
    uint32_t word[E::N1];
#pragma unroll
    for (int it = 0; it < E::N1; ++it) {
      const int ci = (it * 256 + tid) % 3;
      const unsigned b = rawb[it] > 255u ? 0u : rawb[it];
      word[it] = *reinterpret_cast<const uint32_t*>(lut + (ci * 256 + b) * 4);
    }
#pragma unroll
    for (int it = 0; it < E::N1; ++it) {
      const int i = it * 256 + tid;
      if (i < E::NB) *reinterpret_cast<uint32_t*>(tbl + i * 4) = rawb[it] > 255u ? 0u : word[it];
    }
  };

  // ---- phase A, per lane: the table offsets of k = 8 lq + j relative to the 3 x 3 window's first byte, and the masks
  //      that make k = 27 .. 31 zero ----
  int koff[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * lq + j;
    const int kk = k < 27 ? k : 0;
    const int ky = kk / 9;
    koff[j] = (ky * (E::PC * 3) + kk - 9 * ky) * 4;
  }
  const uint32_t kmask1 = lq == 3 ? 0x0000ffffu : ~0u;   // k = 8 lq + (2, 3)
  const uint32_t kmask23 = lq == 3 ? 0u : ~0u;           // k = 8 lq + (4 .. 7)

  // ---- phase B, LDS read side (conv_x3_t448_body.inc): fragment f = column block f of the wave's four rows; xa[k]: byte
  //      address (chunk buffer 0, hi plane) of the lane's 16 bytes of fragment 0 at tap (0, 0) for a tap row of parity k ----
  int xa[2];
  {
    const int pr = li >> 2, pc = li & 3;
    const int A0 = ((wave * 4 + pr) * P + pc) * 64;
#pragma unroll
    for (int k = 0; k < 2; ++k) xa[k] = A0 + ((lq ^ (((pr + k) & 1) << 1)) << 4);
  }
  const __amdgpu_buffer_rsrc_t wrsrc = x3_buffer_of(a.c.wt, 2 * kX3WChunk);
  const int laneW = lane * 16;
  auto w_load = [&](int blk, int tap, int plane, int cs) __attribute__((always_inline)) -> f32x4 {
    return x3_w_load(wrsrc, laneW, blk, tap, plane, cs);
  };

  // ---- prologue: the first item's table ----
  Geo gCur = geo_of(lb);
  unsigned rawb[E::N1];
  load_patch(gCur, rawb);
  f32x4 wreg[3][2][4];   // ring over taps: tap t of a chunk sits in set t % 3
  stage_patch(rawb);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  float amax = 0.f;   // largest |activation| this lane split into planes, of either layer (conv_x3_ws.h, range watch)
  const float floor1 = a.relu1 ? 0.f : -3.4e38f;
  const float floorV = a.c.relu ? 0.f : -3.4e38f;
  for (int w = lb; w < numWork; w += G) {
    const bool lastItem = w + G >= numWork;
    Geo gNext = gCur;
    if (!lastItem) gNext = geo_of(w + G);

    // ================= phase A: enc1.conv1 of the halo into the two chunk buffers =================
    // A pipeline over the wave's nine fragments, one MFMA per gap as in phase B: under the twelve MFMAs of fragment J
    // (the four channel subtiles' chains interleaved, so that no MFMA waits for the one before it) run the affine / split
    // / store of fragment J - 1 and the gather of fragment J + 1.  As straight text per fragment the compiler issued a
    // subtile's three dependent MFMAs back to back and then its VALU work with the matrix pipe idle (3.05 ms per launch
    // at batch 256 against 2.50 ms for enc1.conv2 alone; profiles/r18/enc1_ab.md)
    {
      f32x4 wh[4], wl[4], sc1[4], sh1[4];
      const f32x4* wp = reinterpret_cast<const f32x4*>(a.wt1) + lane;
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) {
        wh[cs] = wp[(cs * 2 + 0) * 64];
        wl[cs] = wp[(cs * 2 + 1) * 64];
        sc1[cs] = *reinterpret_cast<const f32x4*>(a.scale1 + lq * 16 + cs * 4);
        sh1[cs] = *reinterpret_cast<const f32x4*>(a.shift1 + lq * 16 + cs * 4);
      }
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      // three fragments are in flight (J - 1 stored, J multiplied, J + 1 gathered): what a fragment keeps from its gather
      // to its store sits in slot j % 3, what only two of them need at a time in slot j & 1
      int tpo[2];               // the window's table offset
      int dstA[3];              // the lane's first byte in chunk buffer lq >> 1
      uint32_t imask[3];        // all ones inside the image, 0 outside
      uint32_t wv[8];           // the gathered words of the fragment ahead
      u32x4 bh[2], bl[2];       // B operands, hi / lo
      f32x4 accA[2][4];
      uint32_t ph[8], pl[8];
      auto a_addr = [&](int j) __attribute__((always_inline)) {
        int fr = wave + 4 * j;
        fr = fr < E::NFA ? fr : E::NFA - 1;   // duplicates rewrite the same bytes
        int hp = fr * 16 + li;
        hp = hp < E::HP ? hp : E::HP - 1;
        const int hr = hp / P, hc = hp - hr * P;
        tpo[j & 1] = (hr * E::PC + hc) * 12;
        const int y = gCur.y0 - 1 + hr, x = gCur.x0 - 1 + hc;
        imask[j % 3] = ((unsigned)y < (unsigned)a.c.H && (unsigned)x < (unsigned)a.c.W) ? ~0u : 0u;
        dstA[j % 3] = (lq >> 1) * S::XST + hp * 64 + ((((lq & 1) ^ (hr & 1)) << 1) << 4);
      };
      auto a_read = [&](int j) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 8; ++k) wv[k] = *reinterpret_cast<const uint32_t*>(tbl + tpo[j & 1] + koff[k]);
      };
      auto a_pack = [&](int j) __attribute__((always_inline)) {
        uint32_t xh[4], xl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          xh[k] = __builtin_amdgcn_perm(wv[2 * k + 1], wv[2 * k], 0x05040100u);
          xl[k] = __builtin_amdgcn_perm(wv[2 * k + 1], wv[2 * k], 0x07060302u);
        }
        bh[j & 1] = (u32x4){xh[0], xh[1] & kmask1, xh[2] & kmask23, xh[3] & kmask23};
        bl[j & 1] = (u32x4){xl[0], xl[1] & kmask1, xl[2] & kmask23, xl[3] & kmask23};
      };
      // MFMA m of fragment j: term m / 4 (w_lo x_hi, w_hi x_lo, w_hi x_hi: conv_first_x3.h's order) of subtile m % 4
      auto a_mfma = [&](int j, int m) __attribute__((always_inline)) {
        const int cs = m & 3, k = m >> 2;
        const f16x8 wop = __builtin_bit_cast(f16x8, k == 0 ? wl[cs] : wh[cs]);
        const f16x8 xop = __builtin_bit_cast(f16x8, k == 1 ? bl[j & 1] : bh[j & 1]);
        const f32x4 c0 = k == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : accA[j & 1][cs];
        accA[j & 1][cs] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wop, xop, c0, 0, 0, 0);
      };
      // values 2 half, 2 half + 1 of subtile cs of fragment j
      auto a_epi = [&](int j, int cs, int half) __attribute__((always_inline)) {
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int r = 2 * half + e;
          const float t = fmaxf(fmaf(accA[j & 1][cs][r], sc1[cs][r], sh1[cs][r]), floor1);
          v[e] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, t) & imask[j % 3]);
        }
        amax3(amax, v[0], v[1]);
        split_pk_f16_mix(v[0], v[1], ph[cs * 2 + half], pl[cs * 2 + half]);
      };
      auto a_store = [&](int j) __attribute__((always_inline)) {
        char* dst = lds + dstA[j % 3];
        *reinterpret_cast<uint4*>(dst) = make_uint4(ph[0], ph[1], ph[2], ph[3]);
        *reinterpret_cast<uint4*>(dst + 16) = make_uint4(ph[4], ph[5], ph[6], ph[7]);
        *reinterpret_cast<uint4*>(dst + S::XPL) = make_uint4(pl[0], pl[1], pl[2], pl[3]);
        *reinterpret_cast<uint4*>(dst + S::XPL + 16) = make_uint4(pl[4], pl[5], pl[6], pl[7]);
      };
      a_addr(0);
      a_read(0);
      a_pack(0);
#define E1_GAP __builtin_amdgcn_sched_barrier(0)
      x3t_static_for(std::make_integer_sequence<int, E::NJA + 1>{}, [&](auto Jc) __attribute__((always_inline)) {
        constexpr int J = decltype(Jc)::value;
        constexpr bool hasM = J < E::NJA, hasE = J > 0, hasG = J + 1 < E::NJA;
        auto Mf = [&](int m) __attribute__((always_inline)) {
          if (hasM) a_mfma(J, m);
          E1_GAP;
        };
        Mf(0);
        if (hasG) a_addr(J + 1);
        E1_GAP;
        Mf(1);
        if (hasG) a_read(J + 1);
        E1_GAP;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          Mf(2 + q);
          if (hasE) a_epi(J - 1, q >> 1, q & 1);
          E1_GAP;
        }
        Mf(10);
        if (hasG) a_pack(J + 1);
        E1_GAP;
        Mf(11);
        if (hasE) a_store(J - 1);
        E1_GAP;
      });
#undef E1_GAP
    }
    // enc1.conv2's taps 0 and 1 of chunk 0: asked for here, not two taps ahead at the end of the previous item's chunk
    // loop, so that phase A has their 64 registers (held across it they cost it ~180 copies from the accumulator file)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int cs = 0; cs < 4; ++cs) wreg[t][p][cs] = w_load(0, t, p, cs);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (!lastItem) load_patch(gNext, rawb);   // in flight under phase B

    // ================= phase B: enc1.conv2 from the two resident chunks =================
    f32x4 acc[NF][4];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) acc[f][cs] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int cbase = lq * 16;
    f32x4 sc[4], sh[4];
    x3_scale_shift<true>(a.c.scale, a.c.shift, cbase, sc, sh);
    const size_t g0 = (size_t)gCur.n * a.c.H + gCur.y0;   // global row of the tile's first row

#pragma unroll 1
    for (int kc = 0; kc < 2; ++kc) {
      const int wCur = kc * kX3WChunk;
      const int wNxt = (kc ^ 1) * kX3WChunk;   // chunk 1, or chunk 0 of the next item
      int xc[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        xc[k] = xa[k] + kc * S::XST;
        asm volatile("" : "+v"(xc[k]));
      }
      f32x4 xh[3], xl[3];   // ring over (tap, fragment) in program order
      auto x_read = [&](int t, int f, int plane) __attribute__((always_inline)) -> f32x4 {
        const int ky = t / 3, kx = t - ky * 3;
        return *reinterpret_cast<const f32x4*>(lds + xc[ky & 1] + plane * S::XPL + f * 256 + (ky * P + kx) * 64);
      };
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        xh[f] = x_read(0, f, 0);
        xl[f] = x_read(0, f, 1);
      }
      constexpr int STEPS = 9 * NF;
#define E1_GAP __builtin_amdgcn_sched_barrier(0)
      x3t_static_for(std::make_integer_sequence<int, STEPS>{}, [&](auto Lc) __attribute__((always_inline)) {
        constexpr int L = decltype(Lc)::value;
        constexpr int t = L / NF, f = L % NF;
        // under this fragment's 12 MFMAs (three per channel subtile, small terms first): the operands of the step two
        // ahead, the weight fragments of the tap two ahead (two per fragment step)
        constexpr int L2 = L + 2;
        constexpr bool pre = L2 < STEPS;
        constexpr int pt = L2 / NF, pf = L2 % NF, ps = L2 % 3;
        auto M = [&](int m) __attribute__((always_inline)) {
          const int cs = m / 3, k = m - cs * 3;
          mfma_x3_acc(acc[f][cs], wreg[t % 3][k == 0 ? 1 : 0][cs], k == 1 ? xl[L % 3] : xh[L % 3]);
        };
        auto W = [&](int i) __attribute__((always_inline)) {
          if (i < 8) {
            const int tt = t + 2;
            wreg[tt % 3][i >> 2][i & 3] = w_load(tt < 9 ? wCur : wNxt, tt % 9, i >> 2, i & 3);
          }
        };
        M(0);
        E1_GAP;
        M(1);
        E1_GAP;
        if (pre) xh[ps] = x_read(pt, pf, 0);
        E1_GAP;
        M(2);
        M(3);
        E1_GAP;
        if (pre) xl[ps] = x_read(pt, pf, 1);
        E1_GAP;
        M(4);
        M(5);
        E1_GAP;
        W(2 * f);
        E1_GAP;
        M(6);
        M(7);
        E1_GAP;
        W(2 * f + 1);
        E1_GAP;
        M(8);
        M(9);
        E1_GAP;
        M(10);
        M(11);
        E1_GAP;
      });
#undef E1_GAP
      // The chunk's last MFMAs write acc[NF - 1][3] (and [2] just before): inline text, so the compiler knows of no wait
      // between them and a read of their results.  The pad takes those accumulators as operands: whatever reads them - the
      // copies at this loop's exit included - comes after it
      asm volatile("s_nop 15\n\ts_nop 15" : "+a"(acc[NF - 1][2]), "+a"(acc[NF - 1][3])::"memory");
    }
    // the next item's table (read in phase A only), then: every wave's reads of the chunk buffers are done
    if (!lastItem) stage_patch(rawb);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // ================= epilogue: the third structure's EPI 1, straight from the accumulators =================
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      // pixel offsets are recomputed per fragment from an opaque copy of the lane's index (conv_x3_r512.h)
      int liE = li;
      asm volatile("" : "+v"(liE));
      const int prE = liE >> 2, pcE = liE & 3;
      const int r = wave * 4 + prE, c = f * 4 + pcE;
      const bool ok = gCur.y0 + r < a.c.H;
      const size_t pix = (g0 + r) * a.c.W + gCur.x0 + c;
      float v[16];
      x3_affine16(acc[f], sc, sh, floorV, v);
      uint32_t ph[8], pl[8];
      x3_split16(v, amax, ph, pl);
      // MaxPool2d(2,2) on the fp32 values (the split is monotonic): both partners are in this fragment.  Valid in the
      // lanes of even block row and even block column: li = 0, 2, 8, 10
      uint32_t qh[8], ql[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float m0 = fmaxf(v[2 * i], dpp_xor1_f(v[2 * i])), m1 = fmaxf(v[2 * i + 1], dpp_xor1_f(v[2 * i + 1]));
        m0 = fmaxf(m0, dpp_rowshl4_f(m0));
        m1 = fmaxf(m1, dpp_rowshl4_f(m1));
        split_pk_f16_mix(m0, m1, qh[i], ql[i]);
      }
      const bool okp = gCur.y0 + r + 1 < a.c.H && (liE & 5) == 0;
      uint16_t* pp = a.c.pool + (((g0 + r) >> 1) * (size_t)(a.c.W >> 1) + ((gCur.x0 + c) >> 1)) * (size_t)a.c.Cout + cbase;
      if (okp) {
        uint4* o = reinterpret_cast<uint4*>(pp);
        o[0] = make_uint4(qh[0], qh[1], qh[2], qh[3]);
        o[1] = make_uint4(qh[4], qh[5], qh[6], qh[7]);
        uint4* ol = reinterpret_cast<uint4*>(pp + a.c.poolLo);
        ol[0] = make_uint4(ql[0], ql[1], ql[2], ql[3]);
        ol[1] = make_uint4(ql[4], ql[5], ql[6], ql[7]);
      }
      x3_swap_planes64(ph, pl);   // 64 contiguous bytes per pixel and store instruction
      uint16_t* rowp = a.c.out + pix * (size_t)a.c.ldo + a.c.co_off + lq * 8;
      if (ok) x3_store_planes64<true>(rowp, a.c.outLo, ph, pl);   // non-temporal, as the 64-channel forms (conv_x3_t448_body.inc)
      __builtin_amdgcn_sched_barrier(0);   // one fragment at a time: 16 values live
    }
    gCur = gNext;
  }
  x3_report_range(amax, a.c.err);
}

}  // namespace unet
