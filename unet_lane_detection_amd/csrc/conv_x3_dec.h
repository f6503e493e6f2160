// Split-operand ("f16x3") decoder step with the transposed convolution composed into its 3x3 consumer:
//   ConvTranspose2d(2f -> f, k2, s2, bias) -> cat([skip, up]) -> Conv3x3(2f -> f) -> scale / shift (BatchNorm) -> ReLU
// as ONE operator on the skip (high resolution, f channels, 9 taps) and on the transposed convolution's LOW-resolution
// input x (2f channels, 4 taps per output parity).  Nothing non-linear sits between the two convolutions, so for the
// output pixel (2i + a, 2j + b) the up half is a 2 x 2-tap convolution of x at rows i + a - 1 + {0, 1} and columns
// j + b - 1 + {0, 1} with weights W'[a][b] that depend on the parity (a, b) (composed on the host in float64:
// compose_upcat in unet_x3.inc), and the transposed convolution's bias becomes a per-channel constant that depends on the
// pixel's border class only (top / interior / bottom x left / interior / right) - folded into the shift, the 8 border
// classes as deltas (dshift) added in the epilogue of the tiles that touch an image border.  The up half costs 8 f^2
// multiply-adds per output pixel instead of 9 f^2 + 2 f^2, and the transposed convolution's full-resolution output is
// neither written nor read back ("The decoder's composed first convolution").
//
// The third structure's recipe (conv_x3_t448.h): 16 x 28 block tiles, one wave per SIMD, accumulators in AGPRs, weights
// straight from L2 (a ring of four taps), the halo tiles staged in LDS by LDS-DMA from the four waves themselves, one
// barrier per 32-channel chunk, every LDS read one lane register plus an immediate.  What differs:
//
//  * a pixel fragment is 16 pixels of ONE parity class: lane li holds pixel (2 (li >> 1) + a, 4 cb + 2 (li & 1) + b) of
//    the tile - 8 low-resolution rows x 2 low-resolution columns (the 8 x 14 parity class of a 16 x 28 tile is seven of
//    them), so one weight fragment of W'[a][b] serves the whole fragment.  WCO = 1 (64 channels): wave wp owns parity
//    (wp >> 1, wp & 1), 7 fragments; WCO = 2 (128 channels): wave (wp, wc) owns row parity wp, both column parities,
//    14 fragments;
//  * the chunks of an item run in a fixed order: the skip's f / 32 chunks (9 taps over the high-resolution halo), then
//    x's 2f / 32 chunks (4 taps per parity over a 10 x 16 low-resolution halo; with WCO = 2 a chunk is 8 "taps", column
//    parity b then tap, of 7 fragments each) - the same order at every batch size and in graph replay;
//  * the skip's pixels in a fragment are 2 apart, so only half of a 256-byte bank row's 64-byte pixel positions occur:
//    the reads are 2-way conflicted whatever the swizzle within a pixel (8 LDS cycles per ds_read_b128 instead of 4;
//    2 reads per 12 MFMAs).  The swizzle (16-byte part XOR 2 x ((halo row >> 1) & 1)) keeps it at 2-way; x's halo, pitch
//    17 pixels with the part XOR 2 x (halo row & 1), is conflict free (tools/lds_conflicts.py --dec).
//
// EPI 0 only (plane output).  Needs f % 64 == 0 (WCO = 2: f % 128 == 0), W % 28 == 0, H even; any H (rows past the bottom
// read the zero page and are not stored).
#pragma once
#include <type_traits>
#include <utility>
#include "conv_x3_t448.h"

namespace unet {

struct UpcatX3Args {
  const uint16_t* skip;   // hi plane (N,H,W), pixel stride ldSkip, channels [0, f); lo plane at skip + skipLo
  size_t skipLo;
  const uint16_t* x;      // hi plane (N,H/2,W/2,2f); lo plane at x + xLo
  size_t xLo;
  const uint16_t* wt;     // packed per 64-channel tile: nS skip chunks [tap 9][plane][cs][lane][8], then nX x chunks
                          // [parity 4][tap 4][plane][cs][lane][8]
  const uint16_t* zeros;  // >= 64 zero halfs
  const float* scale;     // per channel, divided by the weights' power-of-two pre-scale
  const float* shift;     // per channel: the interior class
  const float* dshift;    // [9][F]: shift of border class c minus the interior's (class 4: zeros)
  uint16_t* out;          // hi plane (N,H,W), pixel stride ldo; lo plane at out + outLo
  size_t outLo;
  int N, H, W, F, ldSkip, ldo, tilesX, tilesY, nS, nX, relu, coTiles, pixTiles;
  unsigned* err;
};

struct X3DShape {
  static constexpr int TWX = 28, TH = 16, CB = 7;
  static constexpr int P = 30, HH2 = 18;                       // skip halo: 18 x 30, pitch 30
  static constexpr int NQS = (HH2 * P * 64 + 1023) / 1024;     // 34 pieces of 1 KiB per plane
  static constexpr int NJS = (NQS + 3) / 4;                    // 9 per wave
  static constexpr int PX = 17, HHX = 10, HWX = 16;            // x halo: 10 x 16 low-resolution pixels, pitch 17
  static constexpr int NQXX = (HHX * PX * 64 + 1023) / 1024;   // 11
  static constexpr int NJX = (NQXX + 3) / 4;                   // 3
  static constexpr int XPL = NQS * 1024, XST = 2 * XPL;
  static constexpr int LDS_BYTES = 2 * XST;
  static constexpr int SKIP_CHUNK = 9 * 2 * 4 * 1024, X_CHUNK = 4 * 4 * 2 * 4 * 1024;   // packed weight bytes
  static_assert(NQXX <= NQS, "");
  static_assert(LDS_BYTES <= 160 * 1024, "");
  static_assert(XPL + (4 * (CB - 1) + 3) * 64 < 65536, "ds_read offsets are 16 bits: the largest immediate");
};

// fragment of step fs of tap t: x chunks of the 128-channel form go column parity by column parity (7 fragments each)
template <bool XK, int WCO>
constexpr int x3d_frag(int t, int fs) {
  return (XK && WCO == 2) ? (t >> 2) * 7 + fs : fs;
}

template <int WCO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void upcat_conv3x3_dec_f16x3_kernel(
    const UpcatX3Args a) {
  using S = X3DShape;
  constexpr int P = S::P, PX = S::PX, NJ = S::NJS, CB = S::CB;
  constexpr int NF = 7 * WCO;   // fragments per wave: 7 (one parity) / 14 (two column parities)
  static_assert(WCO == 1 || WCO == 2, "64- and 128-channel block tiles");

  extern __shared__ __attribute__((aligned(16))) f32x4 smemv[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wp = wave / WCO, wc = wave - wp * WCO;
  const int pa = WCO == 1 ? wp >> 1 : wp;    // the wave's row parity
  const int pbw = WCO == 1 ? wp & 1 : 0;     // its first column parity
  const int li = lane & 15, lq = lane >> 4;
  const int G = gridDim.x;   // multiple of 8 (wave_tile.h)
  const int lb = x3_logical_block(G);
  const int numWork = a.pixTiles * a.coTiles;
  if (lb >= numWork) return;
  const unsigned ldsBase = lds_address(smemv);
  const char* lds = reinterpret_cast<const char*>(smemv);
  const int hX = a.H >> 1, wX = a.W >> 1, cX = 2 * a.F;
  const int nCh = a.nS + a.nX;

  // ---- LDS-DMA: this wave issues pieces q = wave + 4j of both planes; per-lane parts of the two halo layouts ----
  int hrcS[NJ];
  unsigned soffS[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    int q = wave + j * 4;
    q = q < S::NQS ? q : S::NQS - 1;   // duplicates rewrite the same bytes
    const int v = q * 64 + lane;
    const int qpix = v >> 2;
    const int hr = qpix / P, hc = qpix - hr * P;
    const int part = (v & 3) ^ (((hr >> 1) & 1) << 1);
    hrcS[j] = (hr << 8) | hc;
    soffS[j] = (unsigned)(((hr * a.W + hc) * a.ldSkip + part * 8) * 2);
  }
  int hrcX[S::NJX];
  unsigned soffX[S::NJX];
#pragma unroll
  for (int j = 0; j < S::NJX; ++j) {
    int q = wave + j * 4;
    q = q < S::NQXX ? q : S::NQXX - 1;
    const int v = q * 64 + lane;
    const int qpix = v >> 2;
    const int hr = qpix / PX, hc = qpix - hr * PX;
    const int part = (v & 3) ^ ((hr & 1) << 1);
    hrcX[j] = (hr << 8) | hc;
    soffX[j] = (unsigned)(((hr * wX + hc) * cX + part * 8) * 2);
  }
  // the zero page's 16 bytes of this lane: formed at each use (opaque laneW), a 64-bit lane pointer held instead costs two
  // of the registers the 128-channel form does not have
  auto zero_src = [&]() __attribute__((always_inline)) -> const char* {
    int lw = lane * 16;
    asm volatile("" : "+v"(lw));
    return reinterpret_cast<const char*>(a.zeros) + (lw & 48);
  };
  const size_t skipLoB = a.skipLo * 2, xLoB = a.xLo * 2;

  struct Geo {
    const char* tb;    // skip halo's top-left pixel (row y0 - 1, column x0 - 1), hi plane
    const char* txb;   // x halo's top-left pixel (row y0 / 2 - 1, column x0 / 2 - 1), hi plane
    int hrMin, hrSpan, hcMin, hcSpan;       // skip halo
    int n, y0, x0, cg;
  };
  auto geo_of = [&](int w) __attribute__((always_inline)) {
    Geo g;
    g.cg = w % a.coTiles;
    const int tile = w / a.coTiles;
    const int rowTile = tile / a.tilesX;
    g.x0 = (tile - rowTile * a.tilesX) * S::TWX;
    g.n = rowTile / a.tilesY;
    g.y0 = (rowTile - g.n * a.tilesY) * S::TH;
    const int hrMax = a.H - g.y0 < S::HH2 - 1 ? a.H - g.y0 : S::HH2 - 1;
    const int hcMax = a.W - g.x0 < P - 1 ? a.W - g.x0 : P - 1;
    g.hrMin = g.y0 == 0 ? 1 : 0;
    g.hcMin = g.x0 == 0 ? 1 : 0;
    g.hrSpan = hrMax - g.hrMin;
    g.hcSpan = hcMax - g.hcMin;
    g.tb = reinterpret_cast<const char*>(a.skip) + ((((long)g.n * a.H + g.y0 - 1) * a.W + g.x0 - 1) * (long)a.ldSkip) * 2;
    const int i0 = g.y0 >> 1, j0 = g.x0 >> 1;
    g.txb = reinterpret_cast<const char*>(a.x) + ((((long)g.n * hX + i0 - 1) * wX + j0 - 1) * (long)cX) * 2;
    return g;
  };
  // both planes of piece index j of (item g, chunk kc) -> halo buffer `buf`; x chunks have NJX pieces per wave
  auto issue_piece = [&](const Geo& g, int kc, int j, int buf) __attribute__((always_inline)) {
    const unsigned dstB = ldsBase + buf * S::XST;
    if (kc < a.nS) {
      int q = wave + j * 4;
      q = q < S::NQS ? q : S::NQS - 1;
      int hrc = hrcS[j];
      asm volatile("" : "+v"(hrc));   // unpacked here: hoisted out of the loops the two halves would double the table
      const int hr = hrc >> 8, hc = hrc & 255;
      const bool ok = (unsigned)(hr - g.hrMin) <= (unsigned)g.hrSpan && (unsigned)(hc - g.hcMin) <= (unsigned)g.hcSpan;
      unsigned so = soffS[j];
      asm volatile("" : "+v"(so));   // widened here: held as a 64-bit offset every entry carries a zero register
      const char* src = g.tb + so + (unsigned)(kc * 64);
      const char* zp = zero_src();
      lds_dma16(ok ? src : zp, dstB + q * 1024);
      lds_dma16(ok ? src + skipLoB : zp, dstB + q * 1024 + S::XPL);
    } else if (j < S::NJX) {
      int q = wave + j * 4;
      q = q < S::NQXX ? q : S::NQXX - 1;
      const int i0 = g.y0 >> 1, j0 = g.x0 >> 1;
      const int hrMinX = i0 == 0 ? 1 : 0, hcMinX = j0 == 0 ? 1 : 0;
      const int hrMaxX = hX - i0 < S::HHX - 1 ? hX - i0 : S::HHX - 1;
      const int hcMaxX = wX - j0 < S::HWX - 1 ? wX - j0 : S::HWX - 1;
      int hrc = hrcX[j];
      asm volatile("" : "+v"(hrc));
      const int hr = hrc >> 8, hc = hrc & 255;
      const bool ok = (unsigned)(hr - hrMinX) <= (unsigned)(hrMaxX - hrMinX) && (unsigned)(hc - hcMinX) <= (unsigned)(hcMaxX - hcMinX);
      unsigned so = soffX[j];
      asm volatile("" : "+v"(so));
      const char* src = g.txb + so + (unsigned)((kc - a.nS) * 64);
      const char* zp = zero_src();
      lds_dma16(ok ? src : zp, dstB + q * 1024);
      lds_dma16(ok ? src + xLoB : zp, dstB + q * 1024 + S::XPL);
    }
  };

  // ---- LDS read side.  Skip, tap row ky: xs[ky] = the lane's address of fragment 0 (cb 0, first column parity) at tap
  //      (ky, 0); x, tap row di: xr[di] likewise.  Column block, column parity and tap column are immediates ----
  int xs[3], xr[2];
  {
    const int pr = li >> 1, pc = li & 1;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int hr = 2 * pr + pa + ky;
      xs[ky] = (hr * P + 2 * pc + pbw) * 64 + ((lq ^ (((hr >> 1) & 1) << 1)) << 4);
    }
#pragma unroll
    for (int di = 0; di < 2; ++di) {
      const int hr = pr + pa + di;
      xr[di] = (hr * PX + pc + pbw) * 64 + ((lq ^ ((hr & 1) << 1)) << 4);
    }
  }

  // ---- weights: per 64-channel tile, skip chunks then x chunks (UpcatX3Args::wt) ----
  const int perCt = a.nS * S::SKIP_CHUNK + a.nX * S::X_CHUNK;
  const __amdgpu_buffer_rsrc_t wrsrc = x3_buffer_of(a.wt, (a.F / 64) * perCt);
  const int laneW = lane * 16;
  const int parOff = (WCO == 1 ? (pa * 2 + pbw) : pa * 2) * (4 * 8192);   // this wave's parity block of an x chunk
  auto w_block = [&](int cg, int kc) __attribute__((always_inline)) -> int {   // byte offset of (channel tile, chunk)
    const int ct = cg * WCO + wc;
    return ct * perCt + (kc < a.nS ? kc * S::SKIP_CHUNK : a.nS * S::SKIP_CHUNK + (kc - a.nS) * S::X_CHUNK + parOff);
  };
  auto w_load = [&](int blk, int vt, int plane, int cs) __attribute__((always_inline)) -> f32x4 {
    return x3_buffer_load16(wrsrc, laneW + cs * 1024, blk + (vt * 2 + plane) * 4096);
  };

  // ---- prologue: chunk 0 of the first item (a skip chunk), weights of its taps 0 and 1 ----
  Geo gCur = geo_of(lb);
  f32x4 wreg[4][2][4];   // ring over taps: skip chunks use sets t % 3, x chunks t % 4; a chunk's taps 0 / 1 in sets 0 / 1
  {
#pragma unroll
    for (int j = 0; j < NJ; ++j) issue_piece(gCur, 0, j, 0);
    const int blk = w_block(gCur.cg, 0);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int cs = 0; cs < 4; ++cs) wreg[t][p][cs] = w_load(blk, t, p, cs);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");

  int cc = 0;   // chunks this block has gone through: halo buffer parity
  float amax = 0.f;
  for (int w = lb; w < numWork; w += G) {
    const bool lastItem = w + G >= numWork;
    Geo gNext = gCur;
    if (!lastItem) gNext = geo_of(w + G);

    f32x4 acc[NF][4];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) acc[f][cs] = (f32x4){0.f, 0.f, 0.f, 0.f};

    auto chunk = [&](int kc, auto xkC) __attribute__((always_inline)) {
      constexpr bool XK = decltype(xkC)::value;
      constexpr int TAPS = XK ? 4 * WCO : 9;   // (WCO = 2, x: column parity b = t / 4, tap t % 4)
      constexpr int NFT = XK ? 7 : NF;         // fragments per tap
      constexpr int R = XK ? 4 : 3;            // weight ring length
      const bool lastChunk = kc + 1 == nCh;
      const bool haveNext = !(lastChunk && lastItem);
      const Geo& gIss = lastChunk ? gNext : gCur;
      const int kcIss = lastChunk ? (lastItem ? kc : 0) : kc + 1;
      const int wCur = w_block(gCur.cg, kc);
      const int wNxt = haveNext ? w_block(gIss.cg, kcIss) : wCur;
      const int bufOff = (cc & 1) * S::XST;
      const int nbuf = (cc + 1) & 1;

      int xb[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        xb[k] = (XK ? xr[k & 1] : xs[k]) + bufOff;
        asm volatile("" : "+v"(xb[k]));
      }
      f32x4 xh[3], xl[3];
      auto x_read = [&](int t, int f, int plane) __attribute__((always_inline)) -> f32x4 {
        const int bf = f / CB, cb = f % CB;
        if constexpr (XK) {
          const int tp = t & 3, di = tp >> 1, dj = tp & 1;
          return *reinterpret_cast<const f32x4*>(lds + xb[di] + plane * S::XPL + (2 * cb + bf + dj) * 64);
        }
        const int ky = t / 3, kx = t - ky * 3;
        return *reinterpret_cast<const f32x4*>(lds + xb[ky] + plane * S::XPL + (4 * cb + bf + kx) * 64);
      };
#pragma unroll
      for (int L = 0; L < 2; ++L) {
        xh[L] = x_read(L / NFT, x3d_frag<XK, WCO>(L / NFT, L % NFT), 0);
        xl[L] = x_read(L / NFT, x3d_frag<XK, WCO>(L / NFT, L % NFT), 1);
      }
      constexpr int STEPS = TAPS * NFT;
      constexpr int SPREAD = XK ? (TAPS == 4 ? 2 : 5) : 6;   // taps over which the next chunk's pieces go out
#define D4_GAP __builtin_amdgcn_sched_barrier(0)
      x3t_static_for(std::make_integer_sequence<int, STEPS>{}, [&](auto Lc) __attribute__((always_inline)) {
        constexpr int L = decltype(Lc)::value;
        constexpr int t = L / NFT, fs = L % NFT;
        constexpr int f = x3d_frag<XK, WCO>(t, fs);
        constexpr int L2 = L + 2;
        constexpr bool pre = L2 < STEPS;
        constexpr int pt = L2 / NFT, pf = x3d_frag<XK, WCO>(L2 / NFT, L2 % NFT), ps = L2 % 3;
        auto M = [&](int m) __attribute__((always_inline)) {
          const int cs = m / 3, k = m - cs * 3;
          mfma_x3_acc(acc[f][cs], wreg[t % R][k == 0 ? 1 : 0][cs], k == 1 ? xl[L % 3] : xh[L % 3]);
        };
        // the eight weight fragments of the tap two ahead: one per fragment step (14 per tap), or two (7 per tap)
        auto W = [&](int i) __attribute__((always_inline)) {
          if (i < 8) {
            constexpr int tt = t + 2;
            if constexpr (tt < TAPS)
              wreg[tt % R][i >> 2][i & 3] = w_load(wCur, tt, i >> 2, i & 3);
            else
              wreg[tt - TAPS][i >> 2][i & 3] = w_load(wNxt, tt - TAPS, i >> 2, i & 3);
          }
        };
        M(0);
        D4_GAP;
        M(1);
        D4_GAP;
        if (pre) xh[ps] = x_read(pt, pf, 0);
        D4_GAP;
        M(2);
        M(3);
        D4_GAP;
        if (pre) xl[ps] = x_read(pt, pf, 1);
        D4_GAP;
        M(4);
        M(5);
        D4_GAP;
        W(NFT >= 8 ? fs : 2 * fs);
        D4_GAP;
        M(6);
        M(7);
        D4_GAP;
        if (NFT < 8) W(2 * fs + 1);
        D4_GAP;
        M(8);
        M(9);
        D4_GAP;
        {
          constexpr int jp = x3t_piece_at(L, NFT, NJ, SPREAD);
          if (jp >= 0) issue_piece(gIss, kcIss, jp, nbuf);
        }
        D4_GAP;
        M(10);
        M(11);
        D4_GAP;
      });
#undef D4_GAP
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    // two loops in sequence, not one loop that branches between the two unrolled bodies: with a branch the
    // accumulators' live ranges join across both bodies and the allocator moves them about
    for (int kc = 0; kc < a.nS; ++kc, ++cc) chunk(kc, std::false_type{});
    for (int kc = a.nS; kc < nCh; ++kc, ++cc) chunk(kc, std::true_type{});
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // the last MFMAs' results before the first accumulator read

    // ---- epilogue: lane (li, lq) holds channels 16 lq + [0, 16) of its pixel of each fragment ----
    // the per-channel constants only now: 32 registers the chunk loop needs for its weight ring
    // the lane's part of the geometry again from the thread index, opaque to the compiler: held from the kernel's
    // start these values are live across both chunk loops, which the 128-channel form has no registers for
    int tidE = tid;
    asm volatile("" : "+v"(tidE));
    const int lqE = (tidE >> 4) & 3;
    const int cbase = (gCur.cg * WCO + wc) * 64 + lqE * 16;
    f32x4 sc[4], sh[4];
    x3_scale_shift<false>(a.scale, a.shift, cbase, sc, sh);
    int reluE = a.relu;
    asm volatile("" : "+s"(reluE));
    const float floorV = reluE ? 0.f : -3.4e38f;
    const bool border = gCur.y0 == 0 || gCur.y0 + S::TH >= a.H || gCur.x0 == 0 || gCur.x0 + S::TWX >= a.W;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      int liE = tidE & 15;
      asm volatile("" : "+v"(liE));
      const int r = 2 * (liE >> 1) + pa, c = (f % CB) * 4 + 2 * (liE & 1) + pbw + f / CB;
      const int gy = gCur.y0 + r, gx = gCur.x0 + c;
      const bool ok = gy < a.H;
      f32x4 shE[4];
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) shE[cs] = sh[cs];
      if (border) {   // the transposed convolution's bias by border class (uniform branch: border tiles only)
        const int cls = (gy == 0 ? 0 : gy == a.H - 1 ? 2 : 1) * 3 + (gx == 0 ? 0 : gx == a.W - 1 ? 2 : 1);
        if (cls != 4) {
#pragma unroll
          for (int cs = 0; cs < 4; ++cs)
            shE[cs] += *reinterpret_cast<const f32x4*>(a.dshift + (size_t)cls * a.F + cbase + cs * 4);
        }
      }
      const size_t pix = ((size_t)gCur.n * a.H + gy) * a.W + gx;
      float v[16];
      x3_affine16(acc[f], sc, shE, floorV, v);
      uint32_t ph[8], pl[8];
      x3_split16(v, amax, ph, pl);
      x3_swap_planes64(ph, pl);   // 64 contiguous bytes per pixel and store instruction
      uint16_t* rowp = a.out + pix * (size_t)a.ldo + (cbase - lqE * 16) + lqE * 8;
      // non-temporal as in conv_x3_t448.h's 64-channel form
      if (ok) x3_store_planes64<WCO == 1>(rowp, a.outLo, ph, pl);
      __builtin_amdgcn_sched_barrier(0);   // one fragment at a time: 16 values live
    }
    gCur = gNext;
  }
  x3_report_range(amax, a.err);
}

}  // namespace unet
