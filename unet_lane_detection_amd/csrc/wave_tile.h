// What the kernels built as "one wave per SIMD with the whole 512-register file" share: conv_x3_r512.h, conv_q8_r512.h,
// conv_x3_t448.h, conv_x3_dec.h, conv_bf16_r512.h, upconv_x3_r512.h and upconv_bf16_r512.h.  The block remap, the
// geometry of a work item, the weight loads and those pieces of the epilogue that could be shared without changing
// any kernel are written here once; the MFMA loops and their instruction placement stay in the headers.
//
// The rule for everything in this file: free __device__ __forceinline__ functions, per-lane arrays passed
// by reference, uniform values as plain arguments or in a struct of uniform values (X3Geo lives in SGPRs).  No object
// gathers per-lane state.  These kernels run at 371 - 512 registers with amdgpu_waves_per_eu(1, 1) and their register
// allocation answers to the order of unrelated statements, so a helper is accepted per call site by the assembly
// (tools/asm_compare.py against the commit before): as this file stands, every kernel that uses it is byte-identical to
// its inline text.  A call site where a helper changes the kernel keeps its inline text and says so;
// profiles/r13/wave_tile_refactor.md lists what was tried (the LDS-DMA staging, the FLAT row mask and the BatchNorm
// partial sums are shared nowhere for that reason, and this file does not define them).
#pragma once
#include "conv_x3_ws.h"

namespace unet {

// ---- logical block.  The hardware deals consecutive blockIdx.x to the 8 XCDs in turn; with a grid that is a multiple
//      of 8, logical blocks lb, lb + 1, ... (neighbouring tiles, the channel groups of one tile) run on ONE XCD and
//      share its L2 ----
__device__ __forceinline__ int x3_logical_block(int G) {   // G = gridDim.x
  return (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
}

// ---- geometry of a work item: uniform values only ----
struct X3Geo {
  const char* tb;   // address of the halo's top-left pixel, chunk 0, hi plane (not dereferenced where out of image)
  int hrMin, hrSpan, hcMin, hcSpan;   // halo rows / columns inside the image: [min, min + span]
  int n, y0, x0, cg;
};
// the input's pixel stride in elements: the channel count, unless the argument struct says otherwise (an overload)
template <class A>
__device__ __forceinline__ int x3_in_stride(const A& a) {
  return a.Cin;
}
// item w of ConvX3Args / ConvQ8Args / ConvBfRArgs: channel group innermost within a group of coGroup, then pixel tiles
template <class S, class A>
__device__ __forceinline__ X3Geo x3_geo_of(const A& a, int w) {
  X3Geo g;
  const int cInG = w % a.coGroup;
  const int rest = w / a.coGroup;
  const int tile = rest % a.pixTiles;
  g.cg = (rest / a.pixTiles) * a.coGroup + cInG;
  const int rowTile = tile / a.tilesX;
  g.x0 = (tile - rowTile * a.tilesX) * S::TWX;
  g.n = rowTile / a.tilesY;
  g.y0 = (rowTile - g.n * a.tilesY) * S::TH;
  const int hrMax = a.H - g.y0 < S::HH2 - 1 ? a.H - g.y0 : S::HH2 - 1;
  const int hcMax = a.W - g.x0 < S::HW2 - 1 ? a.W - g.x0 : S::HW2 - 1;
  g.hrMin = g.y0 == 0 ? 1 : 0;
  g.hcMin = g.x0 == 0 ? 1 : 0;
  g.hrSpan = hrMax - g.hrMin;
  g.hcSpan = hcMax - g.hcMin;
  g.tb = reinterpret_cast<const char*>(a.in) +
         ((((long)g.n * a.H + g.y0 - 1) * a.W + g.x0 - 1) * (long)x3_in_stride(a)) * 2;
  return g;
}

// ---- weights straight from L2: buffer loads with descriptor and block offset in SGPRs, the lane's 16 bytes as the
//      only vector operand ----
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x3_buffer_of(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 x3_buffer_load16(__amdgpu_buffer_rsrc_t rsrc, int laneOff, int blockOff) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  return __builtin_bit_cast(f32x4, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rsrc, laneOff, blockOff, 0));
}
// the f16x3 3x3 pack: [coTile(64)][chunk(32)][tapRow][plane][kx][cs][lane][8 halfs]
constexpr int kX3WChunk = 9 * 2 * 4 * 1024;
__device__ __forceinline__ f32x4 x3_w_load(__amdgpu_buffer_rsrc_t rsrc, int laneW, int blk, int tap, int plane, int cs) {
  const int ky = tap / 3, kx = tap - ky * 3;
  return x3_buffer_load16(rsrc, laneW + cs * 1024, blk + ((ky * 2 + plane) * 3 + kx) * 4096);
}

// ---- epilogue pieces.  Lane (li, lq) holds channels 16 lq + [0, 16) of its pixel of a fragment: acc[cs][r] is channel
//      16 lq + 4 cs + r of the wave's tile of 64 ----
// the per-channel constants of the lane's 16 channels.  PIN: the values are made opaque where they are fetched (ahead of
// the chunk loop), so that the loads stay there
template <bool PIN>
__device__ __forceinline__ void x3_scale_shift(const float* scale, const float* shift, int cbase, f32x4 (&sc)[4],
                                               f32x4 (&sh)[4]) {
#pragma unroll
  for (int cs = 0; cs < 4; ++cs) {
    sc[cs] = *reinterpret_cast<const f32x4*>(scale + cbase + cs * 4);
    sh[cs] = *reinterpret_cast<const f32x4*>(shift + cbase + cs * 4);
    if (PIN) asm volatile("" : "+v"(sc[cs]), "+v"(sh[cs]));
  }
}
__device__ __forceinline__ void x3_affine16(const f32x4 (&acc)[4], const f32x4 (&sc)[4], const f32x4 (&sh)[4],
                                            float floorV, float (&v)[16]) {
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = fmaxf(fmaf(acc[e >> 2][e & 3], sc[e >> 2][e & 3], sh[e >> 2][e & 3]), floorV);
}
// split_pk_f16 (values clamped to the fp16 range, as conv_x3_ws.h promises: an out-of-range value is stored as +-65504 and
// reported through amax, never as inf) in 6 instructions per pair: two v_med3_f32, hi = v_cvt_pk_f16_f32, lo = rn16(v - hi)
// as one mixed-precision FMA per value that reads hi as fp16 and writes its fp16 result into one half of the destination
// (v - hi is exact in fp32, so the single rounding is the same as in split_pk_f16: the kernel structures stay
// bit-identical, tests/test_x3_gpu.py).  Callers take amax from the unclamped values first.
__device__ __forceinline__ void split_pk_f16_mix(float v0, float v1, uint32_t& hi, uint32_t& lo) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  v0 = __builtin_amdgcn_fmed3f(v0, -65504.f, 65504.f);
  v1 = __builtin_amdgcn_fmed3f(v1, -65504.f, 65504.f);
  hi = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v0, v1}, f16x2));
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(lo)
      : "v"(hi), "v"(v0), "v"(v1));
}
// amax = max(amax, |v0|, |v1|) in one instruction
__device__ __forceinline__ void amax3(float& amax, float v0, float v1) {
  asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax) : "v"(v0), "v"(v1));
}
// 16 values -> the two planes' 8 packed pairs; amax before the clamp in split_pk_f16_mix
__device__ __forceinline__ void x3_split16(const float (&v)[16], float& amax, uint32_t (&ph)[8], uint32_t (&pl)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    amax3(amax, v[2 * e], v[2 * e + 1]);
    split_pk_f16_mix(v[2 * e], v[2 * e + 1], ph[e], pl[e]);
  }
}
// The four lanes of a pixel (lq = 0..3) hold bytes [32 lq, 32 lq + 32) of its 128 bytes per plane as two 16-byte halves
// p[0..3], p[4..7]; stored as they are, every store instruction writes 16-byte pieces 32 bytes apart.  Two lane-row swaps
// per register pair (rows of 16 lanes: odd <-> even rows, then upper <-> lower half wave) hand lane row q bytes
// [16 q, 16 q + 16) of the first 64 bytes in p[0..3] and of the second 64 in p[4..7]: each store instruction then writes 64
// contiguous bytes per pixel, at rowp = the pixel's first byte + 16 lq.
__device__ __forceinline__ void x3_swap64(uint32_t& a, uint32_t& b) {
  auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
  auto q = __builtin_amdgcn_permlane32_swap(r[0], r[1], false, false);
  a = q[0];
  b = q[1];
}
__device__ __forceinline__ void x3_swap_planes64(uint32_t (&ph)[8], uint32_t (&pl)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    x3_swap64(ph[k], ph[4 + k]);
    x3_swap64(pl[k], pl[4 + k]);
  }
}
// NT: non-temporal stores (conv_x3_t448.h says where and why)
template <bool NT = false>
__device__ __forceinline__ void x3_store_plane64(uint16_t* rowp, const uint32_t (&p)[8]) {
  if (NT) {
    typedef unsigned u32x4nt __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store((u32x4nt){p[0], p[1], p[2], p[3]}, reinterpret_cast<u32x4nt*>(rowp));
    __builtin_nontemporal_store((u32x4nt){p[4], p[5], p[6], p[7]}, reinterpret_cast<u32x4nt*>(rowp + 32));
  } else {
    *reinterpret_cast<uint4*>(rowp) = make_uint4(p[0], p[1], p[2], p[3]);
    *reinterpret_cast<uint4*>(rowp + 32) = make_uint4(p[4], p[5], p[6], p[7]);
  }
}
template <bool NT = false>
__device__ __forceinline__ void x3_store_planes64(uint16_t* rowp, size_t outLo, const uint32_t (&ph)[8],
                                                  const uint32_t (&pl)[8]) {
  x3_store_plane64<NT>(rowp, ph);
  x3_store_plane64<NT>(rowp + outLo, pl);
}
// fp32: 4 x 4 transpose of 16-byte pieces across the four lanes of a pixel (two swap stages): store k then writes bytes
// [64 k + 16 lq, + 16) of the pixel's 256 - 64 contiguous bytes per pixel and instruction; rowp = first float + 4 lq
__device__ __forceinline__ void x3_store_f32_64(float* rowp, bool ok, const float (&v)[16]) {
  uint32_t u[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) u[e] = __builtin_bit_cast(uint32_t, v[e]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    auto r01 = __builtin_amdgcn_permlane16_swap(u[j], u[4 + j], false, false);
    auto r23 = __builtin_amdgcn_permlane16_swap(u[8 + j], u[12 + j], false, false);
    auto s02 = __builtin_amdgcn_permlane32_swap(r01[0], r23[0], false, false);
    auto s13 = __builtin_amdgcn_permlane32_swap(r01[1], r23[1], false, false);
    u[j] = s02[0];
    u[8 + j] = s02[1];
    u[4 + j] = s13[0];
    u[12 + j] = s13[1];
  }
  if (ok) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      *reinterpret_cast<uint4*>(rowp + 16 * k) = make_uint4(u[4 * k], u[4 * k + 1], u[4 * k + 2], u[4 * k + 3]);
  }
}

}  // namespace unet
