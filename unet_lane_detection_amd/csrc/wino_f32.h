// Winograd F(2x2, 3x3) convolution on the gfx950 fp32 matrix pipe.
//
// Same operator as igemm_f32.h with TAPS = 9 (3x3 cross-correlation, stride 1, pad 1, + per-channel
// scale/shift + ReLU; reference README.md:1452-1457), computed as
//     Y = A^T [ sum_ci (G g G^T) .* (B^T d B) ] A
// per 2x2 output tile: 16 element-wise products per (tile, ci, co) instead of 36 multiply-adds, i.e. 2.25x
// fewer MFMAs.  Everything stays fp32; the weight transform G g G^T is done once (host: double -> fp32,
// training: device kernel).  The transforms only add/subtract (the 1/2 factors live in the pre-transformed
// weights); against float64 an fp32 emulation of this kernel's order stays within 1.64 * 2^-24 * sqrt(K) * B of
// the convolution (K = 9 Cin, B = sqrt(conv(x^2, w^2))), the direct kernel's order within 2.57 (measured by
// tests/test_f32_model_cpu.py); tests/test_f32_ops_gpu.py holds both kernels to the same bound.
//
// Work decomposition (512 threads = 8 waves, one block per CU, two waves per SIMD):
//   block  = up to 128 Winograd tiles (THt x TWt tile grid = 2THt x 2TWt output pixels) x 32 output channels;
//   wave w = tiles [16w, 16w+16) x 32 channels x all 16 Winograd points: 16 x 2 accumulators of
//            v_mfma_f32_16x16x4_f32 (128 VGPRs).  For a fixed (tile, channel) the 16 products sit in the
//            SAME lane and register slot of the 16 accumulators, so the output transform A^T m A is pure
//            per-lane register arithmetic - no LDS round trip - and the 2x2 output tile is exactly one
//            MaxPool2d(2,2) window: the pooled tensor is written from the same registers for free.
//   LDS    = raw input halo tile [(2THt+2) x (2TWt+2) pixels][16 ci], double buffered, register-staged one
//            K-chunk ahead.  Each lane reads its tile's 4x4 patch (16 x ds_read_b128, invalid pixels
//            redirected to a zero slot), applies B^T d B in registers (128 v_add per chunk) and uses the
//            result directly as MFMA A operands: the transformed input never exists in memory.
//   B      = transformed weights packed [co_subtile][k_chunk][point(16)][lane][4]; the 32 KiB panel of a
//            K-chunk (16 points x 32 channels x 16 ci) is staged ONCE per block into LDS (double buffered)
//            and shared by the 8 waves: each fragment read is a conflict-free lane-linear ds_read_b128.
//            (Streaming B straight from L2 to VGPRs, as the direct kernel does, left only 8 MFMAs of
//            cover per load here and ran 3.5x below the MFMA bound.)
// Tiles are laid out on "global tile rows" (n*H/2 + ty), so a block may straddle images; all boundary
// handling is per-lane validity of the 16 patch pixels.
#pragma once
#include <hip/hip_runtime.h>

#include "lds_dma.h"
#include <stdint.h>

#include "igemm_f32.h"

namespace unet {

struct WinoArgs {
  const float* in;     // NHWC, pixel stride Cin (multiple of 16)
  const float* wt;     // packed transformed weights
  const float* scale;
  const float* shift;
  float* out;          // NHWC, pixel stride ldo, channel offset co_off
  float* pool;         // optional (N,H/2,W/2,Cout) dense max-pooled copy of the output, or nullptr
  int N, H, W;         // H, W even
  int Cin, Cout;
  int ldo, co_off;
  int THt, TWt;        // tile grid of one block, THt*TWt <= 128
  int tilesX;          // ceil((W/2) / TWt)
  int nChunks;         // Cin / 16
  int relu;
  int coTiles, coGroup, pixTiles;
  int xcdLocal;        // 1: channel tiles of one pixel tile on ONE XCD (small weight sets: the input tile is the L2 traffic)
  unsigned* err;       // device-visible error word (may be null): set when a bounded wave-progress wait gives up
};

constexpr int WINO_THREADS = 512;
constexpr int WINO_TILES = 128;                            // Winograd tiles per block (16 per wave)
constexpr int WINO_NLD = 5;                                // staged raw float4 per thread: up to 640 halo pixels
constexpr int WINO_RAW = WINO_NLD * WINO_THREADS * 4;      // floats of halo data per raw LDS buffer
constexpr int WINO_BUF = WINO_RAW + 16;                    // + a zero slot at the same place in both buffers, so a
                                                           // lane's 16 patch offsets (validity baked in) are chunk-invariant
constexpr int WINO_BN = 2;                                 // 16-channel subtiles per block (32 output channels)
constexpr int WINO_BFL = 16 * WINO_BN * 64 * 4;            // floats per B panel buffer (32 KiB)
constexpr int WINO_BLD = WINO_BFL / 4 / WINO_THREADS;      // staged B float4 per thread (4)
constexpr int WINO_BOFF = 2 * WINO_BUF;                    // B panels behind the two raw buffers
#ifndef WINO_P_ISSUE
#define WINO_P_ISSUE 4     // point of a chunk at which the next chunk's DMA is issued
#endif
#ifndef WINO_P_CONFIRM
#define WINO_P_CONFIRM 12  // ... and at which its arrival is confirmed
#endif
constexpr int WINO_CNT = WINO_BOFF + 2 * WINO_BFL;         // two wave-progress counters (see the chunk loop)
constexpr int WINO_LDS_BYTES = (WINO_CNT + 4) * 4;

// stage-end barrier: waits for this wave's LDS-DMA (lds_dma.h) and LDS reads, then joins the block barrier
__device__ __forceinline__ void wino_stage_barrier() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int NS>
__global__ __launch_bounds__(WINO_THREADS, 2) void wino_f32_kernel(const WinoArgs a) {
  static_assert(NS == WINO_BN, "the B panel staging assumes 32 channels per block");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;

  // blocks are dealt round-robin over the 8 XCDs: by default the coGroup channel tiles of a pixel tile sit on
  // different XCDs (each XCD keeps one weight panel in its L2); with xcdLocal consecutive logical ids share an
  // XCD instead, so one L2 serves the input tile to all of them.  Placement affects speed only.
  int bid = blockIdx.x;
  if (a.xcdLocal) {
    const int g8 = (int)gridDim.x & ~7;
    if (bid < g8) bid = (bid & 7) * (g8 >> 3) + (bid >> 3);
  }
  const int cInG = bid % a.coGroup;
  const int rest = bid / a.coGroup;
  const int tileBlk = rest % a.pixTiles;
  const int coTile = (rest / a.pixTiles) * a.coGroup + cInG;

  const int Ht = a.H >> 1, Wt = a.W >> 1;
  const int GT = a.N * Ht;            // global tile rows
  const int NH = a.N * a.H;
  const int gt0 = (tileBlk / a.tilesX) * a.THt;
  const int tx0 = (tileBlk % a.tilesX) * a.TWt;
  const int RW = 2 * a.TWt + 2, RH = 2 * a.THt + 2;
  const int g0 = 2 * gt0 - 1, x0 = 2 * tx0 - 1;   // top-left pixel of the raw halo tile

  // ---- staging plan (as in igemm_f32.h: clamped coordinates, no predicates) ----
  // LDS image of the raw tile, in 16-byte units: pixel (hr, hc), channel part v lives at
  //     (hr*RW + (hc&1)*RW/2 + (hc>>1))*4 + (PERM[v] ^ (((hc>>3)&1)<<1)),   PERM = {0, 3, 1, 2}
  // i.e. even and odd columns in separate half rows (tiles step two columns, so one patch column of 16
  // neighbouring tiles becomes 16 consecutive 64-byte pixels) and the 16-byte part XOR-swizzled by the
  // pixel's position (it was 4-way bank conflicted in pixel-linear order, 42 % of all LDS cycles).
  // Round 4: the key was ((hc>>3)&3) - chosen for lane groups of 16 CONSECUTIVE lanes.  ds_read_b128 is served in the
  // groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... (MI355X_MICROARCH.md, LDS), which mix two channel parts: under
  // them that key costs 6.0 LDS cycles per read on the 16 x 8 tile grid (224 x 224, 112 x 112; 4.0 = conflict free),
  // 10.0 on 9 x 14 (56 x 56, 28 x 28) and 8.0 on 18 x 7 (SQ_LDS_BANK_CONFLICT 0.244 of the kernel's LDS cycles); this
  // one 4.0 / 7.5 / 8.0 (tools/lds_conflicts.py --wino; no key of this family frees the grids whose width is no
  // multiple of 8: their 16 consecutive tiles wrap a grid row at a position that is no multiple of 4).
  // The tile is filled by LDS-DMA (global_load_lds_dwordx4: destination = wave base + lane*16, so the LDS
  // side is linear and the swizzle is applied to each lane's SOURCE address): thread `tid` owns LDS units
  // tid + j*512 and computes which (pixel, part) belongs there.  No staging registers, no ds_write.
  const int totalVec = RH * RW * 4;
  const int RWh = RW >> 1;
  unsigned srcOff[WINO_NLD];   // in float4 units (the host falls back to the direct kernel past 2^32)
#pragma unroll
  for (int j = 0; j < WINO_NLD; ++j) {
    int u = tid + j * WINO_THREADS;
    u = u < totalVec ? u : totalVec - 1;      // units past the tile duplicate its last vector (never read)
    const int hr = u / (RW * 4);
    const int rem = u - hr * RW * 4;
    const int colIdx = rem >> 2, pp = rem & 3;
    const int half = colIdx >= RWh ? 1 : 0;
    const int hc = 2 * (colIdx - half * RWh) + half;
    const int v = (0x1320 >> ((pp ^ (((hc >> 3) & 1) << 1)) * 4)) & 3;   // inverse of PERM
    int g = g0 + hr, x = x0 + hc;
    g = g < 0 ? 0 : (g > NH - 1 ? NH - 1 : g);
    x = x < 0 ? 0 : (x > a.W - 1 ? a.W - 1 : x);
    srcOff[j] = (unsigned)((((size_t)g * a.W + x) * (size_t)a.Cin) >> 2) + v;
  }

  // B panel staging: float4 index idx = tid + j*512 of the panel [ns][point][lane]; one (ns, chunk) slice is
  // 16 KiB contiguous in the packed weights.
  // wave-uniform bases of the two 16-channel weight streams (kept in SGPRs); a chunk's slice of one stream is
  // 1024 float4 = threads tid and tid+512
  const f32x4* in4 = reinterpret_cast<const f32x4*>(a.in);
  const f32x4* wb[NS];
#pragma unroll
  for (int ns = 0; ns < NS; ++ns)
    wb[ns] = reinterpret_cast<const f32x4*>(a.wt) + ((size_t)coTile * NS + ns) * a.nChunks * 16 * 64;

  // one K-chunk of operands -> LDS buffers `buf` by LDS-DMA (9 x 16 bytes per thread, asynchronous)
  const unsigned ldsBase = lds_address(smem);   // wave-uniform
  auto stageChunk = [&](int chunk, int buf) {
    const unsigned rawBase = ldsBase + (unsigned)(buf * WINO_BUF + wave * 64 * 4) * 4u;
#pragma unroll
    for (int j = 0; j < WINO_NLD; ++j)
      lds_dma16(in4 + srcOff[j] + (unsigned)chunk * 4, rawBase + (unsigned)(j * WINO_THREADS * 4) * 4u);
    const unsigned bBase = ldsBase + (unsigned)(WINO_BOFF + buf * WINO_BFL + wave * 64 * 4) * 4u;
#pragma unroll
    for (int j = 0; j < WINO_BLD; ++j)
      lds_dma16(wb[j >> 1] + (size_t)chunk * 1024 + tid + (j & 1) * WINO_THREADS,
                bBase + (unsigned)(j * WINO_THREADS * 4) * 4u);
  };
  // the first chunk goes out before anything else is computed: its HBM latency is the block's start-up cost (one block
  // per CU), and the patch offsets, masks and accumulator clears below fit under it
  stageChunk(0, 0);
  __builtin_amdgcn_sched_barrier(0);

  // ---- this lane's tile (A operand rows): patch base offset and 16-bit pixel validity ----
  const int tb = wave * 16 + li;
  const int tr = tb / a.TWt, tc = tb - tr * a.TWt;
  int patchOff;          // float4 offset of patch pixel (0,0), channel group lq
  unsigned pmask = 0;    // bit (i*4+j): patch pixel inside the image
  {
    const int gt = gt0 + tr, tx = tx0 + tc;
    const bool tvalid = tb < a.THt * a.TWt && gt < GT && tx < Wt;
    const int ty = gt % Ht;
    patchOff = ((2 * tr) * RW + tc) * 4;   // 16-byte units; column term and swizzled part are added per read
    if (tvalid) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int y = 2 * ty - 1 + i, x = 2 * tx - 1 + j;
          if (y >= 0 && y < a.H && x >= 0 && x < a.W) pmask |= 1u << (i * 4 + j);
        }
    } else {
      patchOff = 0;  // any in-bounds address; every pixel reads the zero slot
    }
  }

  // patch column j of this lane's tile is column 2*tc + j: half-row (j&1), index tc + (j>>1)
  int colOff[4];
  {
    const int permq = (0x2130 >> (lq * 4)) & 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int hc = 2 * tc + j;   // tile-local column of the raw tile (x0 is its column 0)
      colOff[j] = ((j & 1) * RWh + (j >> 1)) * 4 + (permq ^ (((hc >> 3) & 1) << 1));
    }
  }

  // float4 index (inside a raw buffer) of each of this lane's 16 patch pixels, the buffer's zero slot for pixels
  // outside the image: chunk-invariant, so the chunk loop does no mask tests and no address arithmetic but one add
  int poff[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      poff[i][j] = ((pmask >> (i * 4 + j)) & 1u) ? patchOff + i * RW * 4 + colOff[j] : WINO_RAW / 4;

  f32x4 acc[16][NS];
#pragma unroll
  for (int p = 0; p < 16; ++p)
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) acc[p][ns] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (tid < 8)   // the zero slots behind the halo data of both raw buffers (the DMA never writes them)
    *reinterpret_cast<f32x4*>(smem + (tid >> 2) * WINO_BUF + WINO_RAW + (tid & 3) * 4) = (f32x4){0.f, 0.f, 0.f, 0.f};
  volatile unsigned* cnt = reinterpret_cast<volatile unsigned*>(smem + WINO_CNT);
  if (tid == 8) {
    cnt[0] = 0;
    cnt[1] = 0;
  }
  wino_stage_barrier();   // waits for the DMA (vmcnt) as well as the barrier: chunk 0 is staged for everybody

  // After this one barrier the eight waves are only coupled through two counters, so they drift apart by up to a
  // quarter chunk and one wave's chunk-start bubble (patch reads, first transform) sits under its SIMD partner's MFMAs
  // instead of both idling behind the same s_barrier:
  //   cnt[0] += 1 by a wave once ITS DMA pieces of the next chunk have landed (three quarters into a chunk);
  //             chunk k may be read when cnt[0] >= 8 k;
  //   cnt[1] += 1 by a wave once it has issued its last LDS read of a chunk; the DMA of chunk k+1 (a quarter into
  //             chunk k, into the buffers of chunk k-1) may be issued when cnt[1] >= 8 k.
  // Spins are bounded, so a stalled partner (or a protocol bug) can never hang the GPU; a wait that gives up reports
  // through the error word, which the host turns into UNET_ERR_HIP: the launch's results are then invalid.
  auto waitCount = [&](int which, unsigned target) {
    unsigned spins = 0;
    while (cnt[which] < target && ++spins < (1u << 22)) __builtin_amdgcn_s_sleep(1);
    if (spins >= (1u << 22) && a.err && lane == 0) *reinterpret_cast<volatile unsigned*>(a.err) = 1u;
    asm volatile("" ::: "memory");
  };
  auto bump = [&](int which) {
    asm volatile("" ::: "memory");
    if (lane == 0) atomicAdd(const_cast<unsigned*>(&cnt[which]), 1u);
  };

  // two chunks per iteration: the buffer parity is a compile-time constant and folds into the ds_read immediates
  for (int kc2 = 0; kc2 < a.nChunks; kc2 += 2) {
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int kc = kc2 + par;
    if (kc >= a.nChunks) break;   // uniform (odd chunk counts)
    const bool more = kc + 1 < a.nChunks;   // uniform
    if (kc > 0) waitCount(0, 8u * (unsigned)kc);
    const f32x4* bLds = reinterpret_cast<const f32x4*>(smem + WINO_BOFF + par * WINO_BFL) + lane;

    // ---- raw 4x4 patch of this lane's tile, channels 4*lq..4*lq+3 of the chunk ----
    f32x4 d[4][4];
    const f32x4* smem4 = reinterpret_cast<const f32x4*>(smem);
    const int bufOff = par * (WINO_BUF / 4);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) d[i][j] = smem4[bufOff + poff[i][j]];
    // ---- t = B^T d (rows):  t0 = d0 - d2, t1 = d1 + d2, t2 = d2 - d1, t3 = d1 - d3 ----
    f32x4 t[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[0][j] = d[0][j] - d[2][j];
      t[1][j] = d[1][j] + d[2][j];
      t[2][j] = d[2][j] - d[1][j];
      t[3][j] = d[1][j] - d[3][j];
    }
    // ---- per Winograd point (pa, pb): v = (t B)[pa][pb], then 4*NS MFMAs; B fragments read from the
    //      LDS panel one point ahead so the ds_read latency sits under the previous point's MFMAs ----
    f32x4 bf[2][NS];   // indexed by point parity: the loop is fully unrolled, so both indices are static
    f32x4 vq[2];
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) bf[0][ns] = bLds[(ns * 16) * 64];
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int pa = p >> 2, pb = p & 3;
      if (p == WINO_P_ISSUE && more) {   // next chunk into the other buffers, once every wave is done with what they hold
        waitCount(1, 8u * (unsigned)kc);
        stageChunk(kc + 1, par ^ 1);
      }
      if (p == WINO_P_CONFIRM && more) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bump(0);
      }
      if (p < 15) {
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) bf[(p + 1) & 1][ns] = bLds[(ns * 16 + p + 1) * 64];
      } else {
        bump(1);   // the last LDS read of this chunk is in the queue (LDS operations of a wave execute in order)
      }
      // the A operand of point p + 1 is formed before point p's MFMAs go out, so the VALU -> MFMA operand hazard
      // (s_nop padding otherwise) sits under eight MFMAs
      auto tb = [&](int q) -> f32x4 {
        const int qa = q >> 2, qb = q & 3;
        if (qb == 0) return t[qa][0] - t[qa][2];
        if (qb == 1) return t[qa][1] + t[qa][2];
        if (qb == 2) return t[qa][2] - t[qa][1];
        return t[qa][1] - t[qa][3];
      };
      if (p == 0) vq[0] = tb(0);
      if (p < 15) vq[(p + 1) & 1] = tb(p + 1);
      const f32x4 v = vq[p & 1];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int ns = 0; ns < NS; ++ns)
          acc[p][ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[e], bf[p & 1][ns][e], acc[p][ns], 0, 0, 0);
      // pin the order: the next point's B-fragment reads go out BEFORE this point's MFMAs (left alone, the
      // scheduler sinks them to just before their use and waits lgkmcnt(0) in front of every second point);
      // the transform VALU stays free to float between the MFMAs
      if (p == 0) __builtin_amdgcn_sched_group_barrier(0x100, 16 + NS, 0);   // the raw patch and point 0's fragments
      if (p < 15) __builtin_amdgcn_sched_group_barrier(0x100, NS, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4 * NS, 0);
    }
  }
  }

  // ---- epilogue: Y = A^T m A per (tile, channel); A^T = [1 1 1 0; 0 1 -1 -1] ----
  // Addresses: one 64-bit base per accumulator row (tile) and lane; the four pixels of the tile and the two channel
  // subtiles are small offsets from it (formed per store, the epilogue used to spend ~90 v_mul_lo and ~300 moves).
  const float lo = a.relu ? 0.f : -3.4e38f;
  float sc[NS], sh[NS];
  bool okc[NS];
#pragma unroll
  for (int ns = 0; ns < NS; ++ns) {
    const int n = (coTile * NS + ns) * 16 + li;
    okc[ns] = n < a.Cout;
    sc[ns] = a.scale[n];
    sh[ns] = a.shift[n];
  }
  const size_t rowStride = (size_t)a.W * (size_t)a.ldo;   // floats between image rows
  const int nBase = coTile * NS * 16 + li;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int tbo = wave * 16 + lq * 4 + r;   // accumulator row = tile
    const int tro = tbo / a.TWt, tco = tbo - tro * a.TWt;
    const int gt = gt0 + tro, tx = tx0 + tco;
    const bool okt = tbo < a.THt * a.TWt && gt < GT && tx < Wt;
    float* o0 = a.out + ((size_t)(2 * gt) * a.W + 2 * tx) * (size_t)a.ldo + a.co_off + nBase;
    float* o1 = o0 + rowStride;
    float* pl = a.pool ? a.pool + ((size_t)gt * Wt + tx) * (size_t)a.Cout + nBase : nullptr;
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
      float s[4][2];
#pragma unroll
      for (int pa = 0; pa < 4; ++pa) {
        const float m0 = acc[pa * 4 + 0][ns][r], m1 = acc[pa * 4 + 1][ns][r], m2 = acc[pa * 4 + 2][ns][r],
                    m3 = acc[pa * 4 + 3][ns][r];
        s[pa][0] = m0 + m1 + m2;
        s[pa][1] = m1 - m2 - m3;
      }
      float v[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        v[0][j] = fmaxf(fmaf(s[0][j] + s[1][j] + s[2][j], sc[ns], sh[ns]), lo);
        v[1][j] = fmaxf(fmaf(s[1][j] - s[2][j] - s[3][j], sc[ns], sh[ns]), lo);
      }
      if (okt && okc[ns]) {
        o0[ns * 16] = v[0][0];
        o0[ns * 16 + a.ldo] = v[0][1];
        o1[ns * 16] = v[1][0];
        o1[ns * 16 + a.ldo] = v[1][1];
        if (pl) pl[ns * 16] = fmaxf(fmaxf(v[0][0], v[0][1]), fmaxf(v[1][0], v[1][1]));
      }
    }
  }
}


}  // namespace unet
