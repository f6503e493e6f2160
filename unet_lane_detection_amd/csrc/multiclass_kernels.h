// Multi-class segmentation (out_channels = K, 2 <= K <= UNET_MAX_CLASSES): the K-way 1x1 head with softmax, argmax and
// class-mask outputs, the softmax cross-entropy + Dice loss with its logit gradient, the head's backward and the
// confusion matrix.  Plain HIP, memory bound, no atomics on global memory: every reduction runs on a grid that depends
// on the element count alone, block partials in a fixed order, one finalize launch that adds them in double - the same
// bits on every run.  The kernels and their index arithmetic are described in multiclass_kernels.cpp.
//
// Layouts.  Activations x / a / dA: (P, C) dense fp32, P = n * hw pixels, C % 4 == 0, 16-byte aligned.  Logits, probs and
// dlogits: (n, K, hw) fp32 - NCHW like the torch module.  Labels and class masks: (n, hw) uint8.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstddef>

namespace unet {

constexpr int MC_MAX_CLASSES = 8;       // == UNET_MAX_CLASSES

// The class rule of every K-way head (the fp32 and f16x3 heads here, the int8 tier's in i8_classes_kernels.cpp), on K
// logits in registers (KP = K rounded up).  argmax: scan from class 0 with `>` against -inf, so ties go to the lowest
// index and a NaN never wins.
template <int KP>
__device__ __forceinline__ int class_argmax(const float (&z)[KP], int K) {
  float best = -INFINITY;
  int label = 0;
#pragma unroll
  for (int k = 0; k < KP; ++k)
    if (k < K && z[k] > best) {
      best = z[k];
      label = k;
    }
  return label;
}

// softmax: exp(z_k - max z) / sum with expf and an IEEE division; returns the argmax.  Acc: the type the K exponentials
// are added and divided in.  float (the fp32 and f16x3 heads): up to K - 1 roundings of the sum on top of expf's.  double
// (the int8 tier's head, whose logits are exact and whose probabilities are held to 4 x 2^-24 of the float64 softmax at
// K = 8 as well): the sum and the quotient are exact to fp32's precision, which leaves expf's error and one rounding.
template <int KP, typename Acc = float>
__device__ __forceinline__ int softmax_argmax(const float (&z)[KP], int K, float (&p)[KP]) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < KP; ++k)
    if (k < K) m = fmaxf(m, z[k]);
  Acc sum = 0;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    p[k] = k < K ? expf(z[k] - m) : 0.f;
    sum += (Acc)p[k];
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) p[k] = (float)((Acc)p[k] / sum);
  return class_argmax<KP>(z, K);
}

constexpr int MC_MAX_WEIGHTS = 4096;    // K * C floats held in LDS by the head and its backward
constexpr int MC_RED_BLOCKS = 1024;     // the most blocks a reduction uses (4 per CU)

// blocks of a reduction over `items` elements: a function of the count alone
inline int mc_red_blocks(size_t items) {
  const size_t b = items / 64;
  return (int)(b < 1 ? 1 : (b > (size_t)MC_RED_BLOCKS ? (size_t)MC_RED_BLOCKS : b));
}

struct ClassLossParams {
  float ceW, diceW, smooth;
  float cw[MC_MAX_CLASSES];
  int ignore;   // -1: none
};

// weights >= 0 and not both 0, smooth > 0, class weights >= 0 and finite, ignore -1 or 0..255; NaN / Inf rejected
bool class_loss_params_valid(const ClassLossParams& p, int K);

// x (P, C) -> logits / probs (n, K, hw), labels / mask (n, hw); every output optional.  w (K, C) and b (K) on the device.
hipError_t launch_headk(const float* x, const float* w, const float* b, int n, size_t hw, int C, int K, float* logits,
                        float* probs, uint8_t* labels, int maskClass, uint8_t* mask, hipStream_t s);

// the same from the f16x3 tier's operand planes: x = fp16 hi plane (P, C), the lo plane xLo halfs behind it; C % 8 == 0
hipError_t launch_headk_planes(const uint16_t* x, size_t xLo, const float* w, const float* b, int n, size_t hw, int C, int K,
                               float* logits, float* probs, uint8_t* labels, int maskClass, uint8_t* mask, hipStream_t s);

// labels (n, hw) = argmax of stored logits (n, K, hw) as the head forms it, mask = 255 where the label is maskClass; either optional
hipError_t launch_class_labels(const float* logits, int n, size_t hw, int K, uint8_t* labels, int maskClass, uint8_t* mask,
                               hipStream_t s);

// bytes of `work` for launch_class_loss_grad (block partials in double, then the gradient's coefficients)
size_t class_loss_work_bytes();
// lossDev[4] = {total, ce, dice, labels >= K that are not the ignore index}; dlogits (n, K, hw) or null (loss only)
hipError_t launch_class_loss_grad(const float* logits, const uint8_t* labels, int n, size_t hw, int K,
                                  const ClassLossParams& prm, void* work, float* lossDev, float* dlogits, hipStream_t s);

// floats of `partial` for launch_headk_backward
size_t headk_backward_partial_floats(size_t P, int C, int K);
// dl (n, K, hw), a (P, C), w (K, C) -> dA (P, C) (optional), dW (K, C), db (K)
hipError_t launch_headk_backward(const float* dl, const float* a, const float* w, int n, size_t hw, int C, int K, float* dA,
                                 float* partial, float* dW, float* db, hipStream_t s);

size_t confusion_work_bytes();
// acc[t * K + p] += pixels with truth t and prediction p, over the pixels whose truth is < K and not `ignore` and
// whose prediction is < K
hipError_t launch_confusion(const uint8_t* pred, const uint8_t* truth, size_t numel, int K, int ignore, void* work,
                            unsigned long long* acc, hipStream_t s);

}  // namespace unet
