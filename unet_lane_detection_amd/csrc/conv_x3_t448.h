// Split-operand ("f16x3") 3x3 convolution, third structure: the layers with FEW output channels (Cout = 64 / 128: the
// 224 x 224 and 112 x 112 levels of the network, reference README.md:1449-1458 at features[0:2] and their decoder
// mirrors :1476-1479 - 43 % of the forward's flops).
//
// Same arithmetic, packed weights and accumulation order as conv_x3_ws.h / conv_x3_r512.h (chunk -> tap row -> tap ->
// (w_lo x_hi, w_hi x_lo, w_hi x_hi)), so all three structures give bit-identical results.  The second structure's
// recipe (one wave per SIMD, accumulators in AGPRs, weights straight from L2, only the input halo tile in LDS, one
// barrier per chunk, one instruction per MFMA gap) needs 256 (or 128) output channels per block to give every wave a
// 64-channel slice of its own.  With 64 or 128 channels the waves have to share the channels and split the PIXELS, so
// the block tile grows along the pixels instead:
//
//  * block tile = 16 rows x TWX columns (TWX = 28: 448 pixels; TWX = 32: 512 pixels, for maps whose width is not a
//    multiple of 28: the 640 x 640 configuration) x 64 * WCO output channels.  WCO = 1: the four waves own four rows each
//    and all 64 channels (7 / 8 pixel fragments x 4 channel subtiles = 112 / 128 AGPRs); WCO = 2: wave (wp, wc) owns eight
//    rows x channels [64 wc, 64 wc + 64) (14 / 16 fragments x 4 subtiles = 224 / 256 AGPRs - the per-wave shape of the
//    second structure's 256-channel form: 2 LDS reads and 2/3 of a weight load per 12 MFMAs);
//  * a pixel fragment is a 4 x 4 BLOCK of pixels, not 16 consecutive pixels of a row: lane li holds pixel
//    (li >> 2, li & 3) of the block.  Every lane addresses its own pixel anyway, and with this shape
//      - all fragments of a wave are a constant number of bytes apart, as are the nine taps: the LDS address of every
//        read of a chunk is ONE lane register plus an instruction immediate (the second structure recomputes 63
//        addresses per chunk, 4 VALU operations each: 252 of its ~2,000 non-MFMA instructions per chunk);
//      - the bank swizzle - the 16-byte part of a pixel's 64 bytes XOR-ed with 2 x (halo row & 1) - is a constant of the
//        lane per tap-row parity, and makes every ds_read_b128 conflict free for ANY even row pitch
//        (tools/lds_conflicts.py --blocks), so the pitch is TWX + 2 with no padding columns: both planes of a
//        32-channel chunk's halo tile are 68 KiB (TWX = 28), double buffered 136 KiB;
//      - the 2 x 2 max-pool windows lie inside a fragment: horizontal partner lane li ^ 1, vertical partner li ^ 4, both
//        DPP operands - the pooled epilogue needs no second fragment and no LDS;
//  * the plane stores write 64 contiguous bytes per pixel and instruction (wave_tile.h).  Whole 128-byte lines - one
//    more exchange between the lanes of pixels li and li ^ 8 - were built and measured: the epilogue's 7.8k / 15.5k cycles
//    per item (7 / 14 fragments) did not move (profiles/r04/t448_experiments.md): a CU stores ~15 bytes per cycle whatever
//    the shape of the instruction;
//  * staging, weights, barrier and instruction placement as in the second structure: the halo tile of the next chunk by
//    LDS-DMA from the four waves themselves (9 / 10 piece indices per wave, spread over the first six taps), weights of
//    the tap two ahead by buffer loads
//    (every wave of a 64-channel group loads the group's 8 fragments: the block reads them WPXW times, from L1 / L2),
//    one s_barrier per chunk.
//
// EPI 0 stores the two planes, 1 the planes and their 2 x 2 max-pool, 2 runs the fused 1 x 1 head (Cout = 64; activation
// not stored), 3 stores fp32 (training; optional BatchNorm partial sums).  Needs Cin % 32 == 0, Cout % (64 WCO) == 0,
// W % TWX == 0; any H (rows past the bottom read the zero page and are not stored).
//
// Block remap, geometry, weight loads, split_pk_f16_mix and the plane swap / store are wave_tile.h's; the staging, scale /
// shift, affine, split, fp32 store and partial-sum text is repeated here: as helper calls each changed some instance.
#pragma once
#include <type_traits>
#include <utility>
#include "conv_x3_r512.h"

namespace unet {

template <int TWX_, int RB_>
struct X3TShape {
  static constexpr int TWX = TWX_, RB = RB_, TH = 4 * RB_;   // 16 rows (64 / 128 channels per block), 8 rows (256)
  static constexpr int CB = TWX_ / 4;                        // 4 x 4 pixel blocks per tile row: 7 / 8
  static constexpr int P = TWX_ + 2;                         // LDS row pitch in pixels = the halo's width
  static constexpr int HH2 = TH + 2, HW2 = TWX_ + 2;
  static constexpr int NQX = (HH2 * P * 64 + 1023) / 1024;   // 1 KiB DMA pieces of one plane's halo tile: 34 / 39 (19 / 22)
  static constexpr int XPL = NQX * 1024;                     // one plane buffer
  static constexpr int XST = 2 * XPL;                        // hi + lo of one chunk
  static constexpr int NJ = (NQX + 3) / 4;                   // piece indices per wave: 9 / 10 (5 / 6)
  static constexpr int TOFF = 2 * XST;                       // the fused head's 64 weights (EPI 2; never FLAT)
  // FLAT: two zero regions, one per plane (XPL apart like the planes), each as long as the span of a row block's read
  // immediates at one tap row: (CB - 1) * 256 + 2 * 64 + 64 bytes
  static constexpr int ZOFF = 2 * XST, ZLEN = 2048;
  static constexpr int LDS_BYTES_PLAIN = TOFF + 256;
  static constexpr int LDS_BYTES_FLAT = ZOFF + XPL + ZLEN;
  static_assert(TWX_ == 28 || TWX_ == 32, "tile widths 28 and 32");
  static_assert(RB_ == 2 || RB_ == 4, "8- and 16-row tiles");
  static_assert((CB - 1) * 256 + 3 * 64 <= ZLEN, "");
  static_assert(LDS_BYTES_PLAIN <= 160 * 1024 && (RB_ == 4 || LDS_BYTES_FLAT <= 160 * 1024), "");
  // the largest read immediate: lo plane + last row block + last column block + tap (2, 2)
  static_assert(XPL + 4 * P * 64 + (CB - 1) * 256 + (2 * P + 2) * 64 < 65536, "ds_read offsets are 16 bits");
};

// the DMA piece index that goes out at fragment step L of a chunk (NF steps per tap), or -1: the NJ indices evenly
// spaced over the first `taps` taps
constexpr int x3t_piece_at(int L, int NF, int NJ, int taps) {
  for (int j = 0; j < NJ; ++j)
    if (L == ((j + 1) * taps * NF) / NJ - 1) return j;
  return -1;
}

template <int... Is, class F>
__device__ __forceinline__ void x3t_static_for(std::integer_sequence<int, Is...>, F&& f) {
  (f(std::integral_constant<int, Is>{}), ...);
}

// v (lane li) -> v (lane li + 4 of the same row of 16 lanes): the pixel one row down in a 4 x 4 block
__device__ __forceinline__ float dpp_rowshl4_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x104, 0xF, 0xF, true));
}

// rows blocks of the block tile by the waves' layout: 16 rows where the waves split the pixels, 8 where they do not
constexpr int x3t_row_blocks(int WCO) { return WCO == 4 ? 2 : 4; }

// ADD (the decoder's split first convolution): the input is the skip half of a concat buffer - Cin
// channels at pixel stride ldi - and the epilogue adds the windowed transposed convolution's planes P (upconv_x3_win.h),
// read at the output pixel and channels: relu(acc s + (P_hi + P_lo) sP + t)
struct ConvX3AddArgs : ConvX3Args {
  int ldi;                // input pixel stride in halfs
  int ldAdd;              // P's pixel stride in halfs
  const uint16_t* add;    // P's hi plane at the layer's channel 0; lo plane at add + addLo
  size_t addLo;
  const float* addScale;  // sP per output channel
};
__device__ __forceinline__ int x3_in_stride(const ConvX3AddArgs& a) { return a.ldi; }
// what the shared text reads of the addend (nothing, without one)
struct X3AddView {
  const uint16_t* add;
  size_t addLo;
  int ldAdd;
  const float* addScale;
};
__device__ __forceinline__ X3AddView x3_add_view(const ConvX3Args&) { return {nullptr, 0, 0, nullptr}; }
__device__ __forceinline__ X3AddView x3_add_view(const ConvX3AddArgs& a) { return {a.add, a.addLo, a.ldAdd, a.addScale}; }

// The kernel's text is conv_x3_t448_body.inc, included once per argument struct: the instances on ConvX3Args are the
// text as it was (ADD false removes every addend statement before code is generated; tools/asm_compare.py), the addend
// instances are the 256-channel form with the plane epilogue
template <int TWX_, int WCO, int EPI, bool FLAT = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv3x3_x3_t448_kernel(
    const ConvX3Args a) {
  constexpr bool ADD = false;
#include "conv_x3_t448_body.inc"
}

template <bool FLAT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv3x3_x3_t448add_kernel(
    const ConvX3AddArgs a) {
  constexpr int TWX_ = 28, WCO = 4, EPI = 0;
  constexpr bool ADD = true;
#include "conv_x3_t448_body.inc"
}

}  // namespace unet
