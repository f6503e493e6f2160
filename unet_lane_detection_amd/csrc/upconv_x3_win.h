// Windowed transposed convolution of the split-operand (f16x3) tier: ConvTranspose2d(2f -> f, k2, s2, bias) followed by
// the up half of the decoder's 3x3 convolution, composed on the host into a 2 x 2-tap convolution of the low-resolution
// input per output parity (compose_upcat):
//   P[2i+a][2j+b][co] = sum_{di,dj in {0,1}} sum_ci x[i+a-1+di][j+b-1+dj][ci] W'[a,b][co,ci,di,dj] + c[class(2i+a, 2j+b)][co]
// with taps outside the image contributing zero and c the border-class constant (row class x 3 + column class; 0 first
// row / column of the image, 1 interior, 2 last).  P goes, as hi/lo planes, where the transposed convolution's output
// goes on the two-kernel path: the up half of the concat buffer.  Its one reader is the addend epilogue of
// conv_x3_t448.h, which runs the skip half's 3x3 convolution.
//
// The arrangement is upconv_x3_r512.h's (read that header first): one wave per SIMD, wave = (a,b), a work item is 224
// consecutive low-resolution pixels (flattened n, y, x) x 64 output channels, 14 pixel fragments x 4 channel subtiles in
// AGPRs, weights straight from L2, pixels by LDS-DMA, one s_barrier per 64-channel stage.  What differs:
//  * K is 4 taps x 2f.  Tap (di,dj) of wave (a,b) is the flat shift (a-1+di) w + (b-1+dj) of the item's pixels, so a
//    stage holds the item's 224 pixels and PAD = WMAX + 1 more on either side (NP pieces of 16 pixels: 18 for widths up
//    to 28, 16 up to 14; 72 KiB per stage, double buffered).  The part swizzle is a function of the staged position, so a
//    shifted window of 16 pixels is as conflict free as the aligned one;
//  * a flat shift wraps round row ends and runs over frame borders (the batch is tiled flat: borders fall inside
//    items).  A wave's taps have row offset 0 or ro = 2a-1 and column offset 0 or co = 2b-1; per item every lane forms
//    two 14-bit masks - fragment f's pixel has no row neighbour at ro / no column neighbour at co - and a lane whose tap
//    is outside the image reads 16 zero bytes kept behind each plane buffer instead (one v_cndmask on the address per
//    read pair).  Staging zero pixels cannot do this: the pixel that is out of the image for one tap is a legitimate
//    operand of another tap of the same fragment.  Pixels before the first / past the last of the tensor are staged as
//    zeros as in upconv_x3_r512.h;
//  * a unit of the loop is (32-channel sub-chunk, tap): 14 fragment steps of 12 MFMAs against 8 weight fragments, which
//    are fetched one unit ahead into a ring of two (8 units per stage: the ring parity is a compile-time constant);
//  * the same two masks give the output pixel's border class in the epilogue.
// The summation order is fixed (stage -> sub-chunk -> tap -> (w_lo x_hi, w_hi x_lo, w_hi x_hi)): no atomics, results do
// not depend on the batch size or on graph replay.  Needs Cin % 64 == 0, 4 <= w <= WMAX, npix < 2^31.
#pragma once
#include "conv_x3_t448.h"
#include "upconv_x3_r512.h"

namespace unet {

template <int WMAX_>
struct UpconvX3WShape {
  static constexpr int WMAX = WMAX_, TP = 224, NPF = 14, PAD = WMAX_ + 1;
  static constexpr int NP = (TP + 2 * PAD + 15) / 16;   // 16-pixel pieces of one plane of one sub-chunk: 18 / 16
  static constexpr int ZB = 256;                        // zero bytes behind each plane buffer
  static constexpr int XPL = NP * 1024 + ZB;
  static constexpr int XST = 4 * XPL;                   // [sub-chunk][plane]
  static constexpr int LDS_BYTES = 2 * XST;             // 149,504 / 133,120
  static_assert(WMAX_ == 14 || WMAX_ == 28, "widths up to 14 and up to 28");
  static_assert(LDS_BYTES <= 160 * 1024, "");
};

// UpconvX3Args as upconv_x3_r512.h fills it, except: wt packed [coTile(64)][chunk(32)][tap(4)][plane(2)][ab(4)][cs(4)]
// [lane][8], tap = di * 2 + dj; bias = the nine class constants [class][Cout], already multiplied by the output's scale
template <int WMAX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void upconv2x2_x3_win_kernel(
    const UpconvX3Args a) {
  using S = UpconvX3WShape<WMAX>;
  constexpr int NF = S::NPF, NP = S::NP, PAD = S::PAD;
  extern __shared__ __attribute__((aligned(16))) f32x4 smemv[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int G = gridDim.x;
  const int lb = x3_logical_block(G);
  const int numWork = a.pixTiles * a.coTiles;   // consecutive items: the channel tiles of one pixel tile
  if (lb >= numWork) return;
  const unsigned ldsBase = lds_address(smemv);
  const char* lds = reinterpret_cast<const char*>(smemv);
  const int nStages = a.nChunks >> 1;           // 64 channels per stage
  const int npix = (int)a.npix;
  const int oa = wave >> 1, ob = wave & 1;

  // ---- the zero bytes behind the eight plane buffers ----
  *reinterpret_cast<uint2*>(reinterpret_cast<char*>(smemv) + (tid >> 5) * S::XPL + NP * 1024 + (tid & 31) * 8) =
      make_uint2(0u, 0u);

  // ---- LDS-DMA: wave k stages plane k & 1 of sub-chunk k >> 1: NP pieces of 16 pixels, staged position q * 16 +
  //      lane / 4 = pixel p0 - PAD + that; a lane's 16 bytes: part (lane & 3) ^ 2 * bit 2 of the position ----
  const int dPix = lane >> 2;
  const int dPart = (lane & 3) ^ (((lane >> 4) & 1) << 1);
  const char* zp = reinterpret_cast<const char*>(a.zeros) + (lane & 3) * 16;
  // the lane's part of the source address (bytes from the wave's plane and sub-chunk at pixel p0 - PAD); the rest is uniform
  const long laneOff = ((long)dPix * (long)a.Cin + dPart * 8) * 2;
  const char* srcWave = reinterpret_cast<const char*>(a.in) + ((wave >> 1) * 32 - (long)PAD * (long)a.Cin) * 2 +
                        ((wave & 1) ? (long)a.inLo * 2 : 0L);
  const long pieceStep = (long)a.Cin * 32;   // 16 pixels further on, bytes
  const unsigned dstWave = ldsBase + wave * S::XPL;
  auto issue_piece = [&](int p0, int kc64, int q, int buf) __attribute__((always_inline)) {
    const int p = p0 - PAD + q * 16 + dPix;
    const bool ok = (unsigned)p < (unsigned)npix;
    const char* src = srcWave + ((long)p0 * (long)a.Cin * 2 + (long)q * pieceStep + kc64 * 128) + laneOff;
    asm volatile("" : "+v"(src));   // formed whether or not it is used: a select, not a branch round the arithmetic
    lds_dma16(ok ? src : zp, dstWave + buf * S::XST + q * 1024);
  };

  // ---- LDS read side: tap t = di * 2 + dj reads staged position PAD + 16 f + li + di' w + dj' with (di', dj') =
  //      (a - 1 + di, b - 1 + dj); xa[t]: the lane's byte address for fragment 0 (+ f * 1024 + (sub-chunk * 2 + plane) *
  //      XPL + the buffer); zb: the zero bytes, minus nothing yet (the fragment's immediate is taken off per read) ----
  int xa[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int pos = PAD + li + (oa - 1 + (t >> 1)) * a.w + (ob - 1 + (t & 1));
    xa[t] = pos * 64 + ((lq ^ (((pos >> 2) & 1) << 1)) << 4);
  }
  const int zb = NP * 1024 + lq * 16;

  // ---- weights: wave w reads group (a,b) = w of [coTile][chunk][tap][plane][ab][cs][lane][8] ----
  constexpr int WCHUNK = 4 * 2 * 16 * 1024;   // bytes of one (channel tile, 32-channel chunk)
  const __amdgpu_buffer_rsrc_t wrsrc = x3_buffer_of(a.wt, a.coTiles * a.nChunks * WCHUNK);
  const int laneW = lane * 16 + wave * 4096;
  auto w_load = [&](int coTile, int kc32, int tap, int plane, int cs) __attribute__((always_inline)) -> f32x4 {
    return x3_buffer_load16(wrsrc, laneW + cs * 1024, (coTile * a.nChunks + kc32) * WCHUNK + (tap * 2 + plane) * 16384);
  };

  // ---- prologue: stage 0 of the first item, the weights of its first unit ----
  int tileCur = lb / a.coTiles, ctCur = lb - tileCur * a.coTiles;
  f32x4 wreg[2][2][4];   // [ring][plane][cs]
  {
#pragma unroll
    for (int j = 0; j < NP; ++j) issue_piece(tileCur * S::TP, 0, j, 0);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) wreg[0][p][cs] = w_load(ctCur, 0, 0, p, cs);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");

  int cc = 0;   // stages this block has gone through: buffer parity
  float amax = 0.f;
  for (int w = lb; w < numWork; w += G) {
    const bool lastItem = w + G >= numWork;
    int tileNext = tileCur, ctNext = ctCur;
    if (!lastItem) {
      tileNext = (w + G) / a.coTiles;
      ctNext = (w + G) - tileNext * a.coTiles;
    }

    f32x4 acc[NF][4];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) acc[f][cs] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- the item's border masks: bit f of mR - the lane's pixel of fragment f has no row neighbour at 2a - 1 (first
    //      row of its image for a = 0, last for a = 1); of mC - no column neighbour at 2b - 1 ----
    unsigned mR = 0, mC = 0;
    {
      const int pBase = tileCur * S::TP + li;
      const int pc = pBase < npix ? pBase : 0;
      int row = pc / a.w;
      int x = pc - row * a.w;
      int y = row % a.h;
      const int yEdge = oa ? a.h - 1 : 0, xEdge = ob ? a.w - 1 : 0;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        mR |= (y == yEdge ? 1u : 0u) << f;
        mC |= (x == xEdge ? 1u : 0u) << f;
        x += 16;
#pragma unroll
        for (int k = 0; k < 4; ++k)   // 16 pixels cross up to four row ends (w >= 4; the host checks)
          if (x >= a.w) {
            x -= a.w;
            ++y;
            y = y == a.h ? 0 : y;
          }
      }
    }
    // the mask of tap t: (0,0)-offset tap none; row-offset tap mR; column-offset tap mC; both mR | mC.  The tap with row
    // offset 2a - 1 is di = a, the one with column offset 2b - 1 is dj = b (wave-uniform: all-ones or zero selectors)
    auto tap_mask = [&](int t) __attribute__((always_inline)) -> unsigned {
      const unsigned rSel = 0u - (unsigned)((t >> 1) == oa), cSel = 0u - (unsigned)((t & 1) == ob);
      return (mR & rSel) | (mC & cSel);
    };

    for (int ks = 0; ks < nStages; ++ks, ++cc) {
      const bool lastStage = ks + 1 == nStages;
      const bool haveNext = !(lastStage && lastItem);
      const int p0Iss = (lastStage ? tileNext : tileCur) * S::TP;
      const int kIss = lastStage ? (lastItem ? ks : 0) : ks + 1;
      const int ctIss = lastStage ? ctNext : ctCur;
      const int xbuf = (cc & 1) * S::XST;   // this stage's buffer; the next stage goes to the other one
      const int nbuf = (cc + 1) & 1;
      int xc[4];
      unsigned mt[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        xc[t] = xa[t] + xbuf;
        mt[t] = tap_mask(t);
        asm volatile("" : "+v"(xc[t]), "+v"(mt[t]));
      }
      int zc = zb + xbuf;
      asm volatile("" : "+v"(zc));
      // the two plane reads of step L = (unit u = sub-chunk * 4 + tap) * 14 + fragment: one address, two immediates
      auto x_addr = [&](int L) __attribute__((always_inline)) -> int {
        const int u = L / NF, f = L - u * NF, t = u & 3;
        return (mt[t] >> f) & 1u ? zc - f * 1024 : xc[t];
      };
      auto x_read = [&](int addr, int L, int plane) __attribute__((always_inline)) -> f32x4 {
        const int u = L / NF, f = L - u * NF, sc = u >> 2;
        return *reinterpret_cast<const f32x4*>(lds + addr + (sc * 2 + plane) * S::XPL + f * 1024);
      };
      f32x4 xh[3], xl[3];
#pragma unroll
      for (int L = 0; L < 2; ++L) {
        const int ad = x_addr(L);
        xh[L] = x_read(ad, L, 0);
        xl[L] = x_read(ad, L, 1);
      }
      constexpr int STEPS = 8 * NF;
#define UW_GAP __builtin_amdgcn_sched_barrier(0)
      x3t_static_for(std::make_integer_sequence<int, STEPS>{}, [&](auto Lc) __attribute__((always_inline)) {
        constexpr int L = decltype(Lc)::value;
        constexpr int u = L / NF, f = L % NF;
        constexpr int L2 = L + 2;
        constexpr bool pre = L2 < STEPS;   // not across the stage's end: the other buffer is published by the barrier
        constexpr int ps = L2 % 3;
        auto M = [&](int m) __attribute__((always_inline)) {
          const int cs = m / 3, k = m - cs * 3;
          mfma_x3_acc(acc[f][cs], wreg[u & 1][k == 0 ? 1 : 0][cs], k == 1 ? xl[L % 3] : xh[L % 3]);
        };
        int ad = 0;
        M(0);
        UW_GAP;
        if (pre) ad = x_addr(L2 < STEPS ? L2 : 0);
        UW_GAP;
        M(1);
        UW_GAP;
        if (pre) xh[ps] = x_read(ad, L2 < STEPS ? L2 : 0, 0);
        UW_GAP;
        M(2);
        M(3);
        UW_GAP;
        if (pre) xl[ps] = x_read(ad, L2 < STEPS ? L2 : 0, 1);
        UW_GAP;
        M(4);
        M(5);
        UW_GAP;
        // the next unit's eight weight fragments, one per step; the last unit fetches the first of the next stage
        if (f < 8 && (u < 7 || haveNext)) {
          constexpr int un = (u + 1) & 7;
          wreg[(u + 1) & 1][f >> 2][f & 3] =
              w_load(u < 7 ? ctCur : ctIss, (u < 7 ? ks : kIss) * 2 + (un >> 2), un & 3, f >> 2, f & 3);
        }
        UW_GAP;
        M(6);
        M(7);
        UW_GAP;
        // the next stage's NP pieces, evenly spaced over the first six units
        {
          constexpr int jp = x3t_piece_at(L, NF, NP, 6);
          if (jp >= 0) issue_piece(p0Iss, kIss, jp, nbuf);
        }
        UW_GAP;
        M(8);
        M(9);
        M(10);
        M(11);
        UW_GAP;
      });
#undef UW_GAP
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }

    // ---- epilogue: lane (li, lq) holds columns 16 * lq + [0, 16) of its group for pixel li of each fragment ----
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    {
      int liE = li;
      asm volatile("" : "+v"(liE));
      const int pBase = tileCur * S::TP + liE;
      const int cbase = ctCur * 64 + lq * 16;
      // the class constants this wave's pixels can have: interior, row edge, column edge, corner
      const int rE = oa ? 2 : 0, cE = ob ? 2 : 0;
      const float* bI = a.bias + (size_t)4 * a.Cout + cbase;
      const float* bR = a.bias + (size_t)(rE * 3 + 1) * a.Cout + cbase;
      const float* bC = a.bias + (size_t)(3 + cE) * a.Cout + cbase;
      const float* bX = a.bias + (size_t)(rE * 3 + cE) * a.Cout + cbase;
      f32x4 sc4[4], cI[4], cR[4], cC[4], cX[4];
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) {
        sc4[cs] = *reinterpret_cast<const f32x4*>(a.scale + cbase + cs * 4);
        cI[cs] = *reinterpret_cast<const f32x4*>(bI + cs * 4);
        cR[cs] = *reinterpret_cast<const f32x4*>(bR + cs * 4);
        cC[cs] = *reinterpret_cast<const f32x4*>(bC + cs * 4);
        cX[cs] = *reinterpret_cast<const f32x4*>(bX + cs * 4);
      }
      // (row, x) of the lane's pixel of fragment 0; the fragments' pixels follow 16 apart
      const int pc = pBase < npix ? pBase : 0;
      int row = pc / a.w;   // n * h + y
      int x = pc - row * a.w;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const bool ok = pBase + 16 * f < npix;
        const bool eR = (mR >> f) & 1u, eC = (mC >> f) & 1u;
        uint32_t ph[8], pl[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int cs = e >> 1, r = (2 * e) & 3;
          const float b0 = eR ? (eC ? cX[cs][r] : cR[cs][r]) : (eC ? cC[cs][r] : cI[cs][r]);
          const float b1 = eR ? (eC ? cX[cs][r + 1] : cR[cs][r + 1]) : (eC ? cC[cs][r + 1] : cI[cs][r + 1]);
          const float v0 = fmaf(acc[f][cs][r], sc4[cs][r], b0), v1 = fmaf(acc[f][cs][r + 1], sc4[cs][r + 1], b1);
          amax3(amax, v0, v1);
          split_pk_f16_mix(v0, v1, ph[e], pl[e]);
        }
        x3_swap_planes64(ph, pl);   // 64 contiguous bytes per pixel and store instruction (wave_tile.h)
        uint16_t* op = a.out + (((size_t)(2 * row + oa) * (size_t)(2 * a.w)) + 2 * x + ob) * (size_t)a.ldo + a.co_off +
                       ctCur * 64 + lq * 8;
        if (ok) x3_store_planes64(op, a.outLo, ph, pl);
        x += 16;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x >= a.w) {
            x -= a.w;
            ++row;
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    tileCur = tileNext;
    ctCur = ctNext;
  }
  x3_report_range(amax, a.err);
}

}  // namespace unet
