// The general training loss  L = wb * BCE(pos_weight) + wf * Focal(alpha, gamma) + wd * Dice(smooth)  (loss mode 2 of
// include/unet_hip.h) and the mask statistics of the reference's class-imbalance section.  The kernels are in
// loss_kernels.cpp, a translation unit of their own like validate_kernels.cpp: the code objects of the tuned kernels do
// not change when kernels are added here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace unet {

struct LossParams {
  float wb, wf, wd;      // weights of the three terms in the total and in the gradient
  float pw;              // pos_weight of the BCE term
  float alpha, gamma;    // focal term
  float smooth;          // Dice term
};

// Domain of mode 2: weights >= 0 and not all zero, pos_weight > 0, 0 <= alpha <= 1, smooth > 0, gamma == 0 or
// gamma >= 1, everything finite.  0 < gamma < 1 is outside on purpose: d/dx q^gamma is unbounded at q = 0.
bool loss_params_valid(const LossParams& p);

// device scratch (8-byte aligned) the launchers below need for `numel` elements
size_t loss_scratch_bytes(size_t numel);
size_t seg_metrics_cfg_scratch_bytes(size_t numel);

// Partial pass, finalize, gradient pass.  out4: {total, bce, dice loss, focal}; dx: numel floats.
hipError_t launch_loss_grad(const float* logits, const float* targets, size_t numel, const LossParams& p, void* scratch,
                            float* out4, float* dx, hipStream_t s);
// The validation reduction (validate_kernels.h, launch_seg_metrics) with the general loss: accumulators 0-9 as there,
// acc[10] += this batch's focal term.  The loss sums are formed by the same code, in the same order, as
// launch_loss_grad forms them.
hipError_t launch_seg_metrics_cfg(const float* logits, const void* targets, bool targetsU8, size_t numel, float thr,
                                  const LossParams& p, void* scratch, double* acc, hipStream_t s);
// counts[i] = number of bytes > threshold among the pixelsPerImage bytes of image i; zeroes counts itself
hipError_t launch_mask_positive_counts(const uint8_t* masks, int n, size_t pixelsPerImage, int threshold,
                                       unsigned long long* counts, hipStream_t s);

}  // namespace unet
