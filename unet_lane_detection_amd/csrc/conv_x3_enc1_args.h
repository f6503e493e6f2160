// Argument struct and shape of conv_x3_enc1.h, apart from the kernel: that one is no template, so only its launch unit
// includes the header that defines it, and the host logic fills the arguments from here.
#pragma once
#include "conv_x3_t448.h"

namespace unet {

struct ConvEnc1X3Args {
  ConvX3Args c;            // enc1.conv2 as the third structure takes it (in / inLo / zeros unused; coTiles = 1, chunksTotal = 2)
  const uint8_t* frames;   // (N,H,W,3) uint8
  const uint16_t* wt1;     // enc1.conv1: conv_first_x3.h's pack, one channel tile
  const float* scale1;
  const float* shift1;
  int relu1;
  float m0, m1, m2, s0, s1, s2;   // (x - m) / s
};

struct X3Enc1Shape {
  using S = X3TShape<28, 4>;
  static constexpr int HP = S::HH2 * S::P;          // halo pixels of an item: 18 x 30 = 540
  static constexpr int NFA = (HP + 15) / 16;        // phase A fragments: 34
  static constexpr int NJA = (NFA + 3) / 4;         // per wave: 9
  static constexpr int PR = S::HH2 + 2, PC = 32;    // input patch: 20 rows x 32 pixels (30 + 2 used)
  static constexpr int NB = PR * PC * 3;            // its bytes = the table's words: 1920
  static constexpr int N1 = (NB + 255) / 256;       // byte loads per thread: 8
  static constexpr int TBL = 2 * S::XST;            // the table behind the two chunk buffers
  static constexpr int LDS_BYTES = TBL + NB * 4 + 3 * 256 * 4;   // ... and the 3 x 256 normalised, split byte values
  static_assert(HP * 64 <= S::XPL, "");
  static_assert(LDS_BYTES <= 160 * 1024, "");
};

}  // namespace unet
