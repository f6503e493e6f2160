// Validation pass: the device reductions behind unet_train_eval_* and unet_seg_metrics_accumulate.  The kernels are in
// validate_kernels.cpp, a translation unit of their own: the code object of unet_hip.cpp, whose kernels are tuned and
// measured as laid out, does not change when kernels are added here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace unet {

constexpr int SEG_PARTIALS = 9;   // doubles per block of the metrics' first pass

// BatchNorm in eval form for one conv unit: see bn_eval_fold_kernel
struct BnFoldDesc {
  const float *gamma, *beta, *mean, *var;
  float *scale, *shift;
  int C, Cpad;
};

// one block per descriptor; descs is a device array
hipError_t launch_bn_eval_fold(const BnFoldDesc* descs, int nDescs, float eps, hipStream_t s);
// both passes of the metrics reduction; partial: nb * SEG_PARTIALS doubles of device scratch
hipError_t launch_seg_metrics(const float* logits, const void* targets, bool targetsU8, size_t numel, float thr,
                              int lossMode, float bceWeight, float diceWeight, float posWeight, float smooth,
                              double* partial, unsigned nb, double* acc, hipStream_t s);

}  // namespace unet
