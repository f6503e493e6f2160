// int8 tier, K-class head (2 <= K <= 8): the 1x1 head with K rows on the last int8 (or, in a hybrid model, fp16) tensor,
// with the outputs of the float tiers' K-way head (multiclass_kernels.h): logits (n, K, hw) fp32, their softmax, the
// argmax labels (n, hw) uint8 and the byte plane of one class.  Every output is optional; with labels or the plane alone a
// call writes one byte per pixel.  The kernels are described in i8_classes_kernels.cpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstddef>

namespace unet {

struct HeadKI8Args {
  const void* x;          // (npix, ld) int8, or fp16 for launch_headk_h16 with in16; ld in elements, a multiple of 16
  int ld, C, K;           // C real channels, C % 16 == 0, K * C <= 2048
  size_t npix, hw;        // npix = n * hw; hw % 4 == 0
  int xzp;
  // the int8 head: K rows of C int8 weights, per row zero point, bias (int32) and multiplier
  const int8_t* w;
  const int32_t* wzp;
  const int32_t* bias;
  const float* mult;
  // the hybrid head: K rows of C fp16 weights, per row m and b (quant.py, "hybrid quantisation")
  const uint16_t* wh;
  const float* hm;
  const float* hb;
  float* logits;          // 16-byte aligned
  float* probs;           // 16-byte aligned
  uint8_t* labels;        // 4-byte aligned
  uint8_t* mask;          // 4-byte aligned
  int maskClass;
};

// logit_k = float(dot(x, w_k) - wzp_k sum x + bias_k - xzp sum w_k + C xzp wzp_k) * mult_k: int32 arithmetic and one IEEE
// multiplication, the single-class head_i8_kernel's per row.  hipErrorInvalidValue for arguments outside the above.
hipError_t launch_headk_i8(const HeadKI8Args& a, hipStream_t s);
// logit_k = (sum_c w16[k][c] x[c]) m_k + b_k in fp32, c ascending, x = q - xzp from an int8 tensor or the stored fp16 value
hipError_t launch_headk_h16(const HeadKI8Args& a, bool in16, hipStream_t s);

}  // namespace unet
