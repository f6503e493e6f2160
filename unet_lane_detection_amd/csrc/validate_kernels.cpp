// Kernels of the validation pass (validate_kernels.h), in the style of train_kernels.h: two-stage deterministic
// reductions, plain C++, vector stores only.
#include "validate_kernels.h"

#include <stdint.h>

namespace unet {

// ---------------------------------------------------------------------------------------------------
// Validation pass (reference README.md:2087-2112): segmentation metrics and the validation loss of one batch in one
// read of logits and targets, added to 16 running accumulators (include/unet_hip.h, unet_seg_metrics_accumulate).
// Pass 1, per block: 9 doubles {TP, FP, FN, TN, BCE sum, sum s t, sum s, sum t, sum pred t}.  The four counts are
// kept as integers per thread and per block and become doubles only there (exact up to 2^53); the loss sums follow
// bce_dice_partial_kernel (mode 1) / bce_loss_grad_kernel (mode 0) term by term, the Dice sums dice_metric_partial_kernel.
// U8: targets are bytes, 0 = background, anything else = lane (the dataset's 0 / 255 masks before the division).
// ---------------------------------------------------------------------------------------------------
template <bool U8>
__global__ __launch_bounds__(256) void seg_metrics_partial_kernel(const float* __restrict__ x, const void* __restrict__ tRaw,
                                                                  size_t n, float thr, int lossMode, float pw,
                                                                  double* __restrict__ partial) {
  unsigned long long cnt[4] = {0, 0, 0, 0};
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float xv = x[i];
    const float tv = U8 ? (static_cast<const uint8_t*>(tRaw)[i] != 0 ? 1.f : 0.f) : static_cast<const float*>(tRaw)[i];
    const bool pred = xv > thr, truth = tv > 0.5f;
    cnt[0] += pred && truth;     // (constant indices: the counters stay in registers)
    cnt[1] += pred && !truth;
    cnt[2] += !pred && truth;
    cnt[3] += !pred && !truth;
    const float e = expf(-fabsf(xv));
    const float l1p = log1pf(e);
    if (lossMode == 1) {
      const float logs = fminf(xv, 0.f) - l1p, log1ms = -fmaxf(xv, 0.f) - l1p;
      acc[0] += -(pw * tv * logs + (1.f - tv) * log1ms);
    } else {
      acc[0] += fmaxf(xv, 0.f) - xv * tv + l1p;
    }
    const float sg = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    acc[1] += sg * tv;
    acc[2] += sg;
    acc[3] += tv;
    acc[4] += pred ? tv : 0.f;
  }
  __shared__ unsigned long long redC[4][256];
  __shared__ float redF[5][256];
#pragma unroll
  for (int k = 0; k < 4; ++k) redC[k][threadIdx.x] = cnt[k];
#pragma unroll
  for (int k = 0; k < 5; ++k) redF[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int k = 0; k < 4; ++k) redC[k][threadIdx.x] += redC[k][threadIdx.x + s];
#pragma unroll
      for (int k = 0; k < 5; ++k) redF[k][threadIdx.x] += redF[k][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) partial[(size_t)blockIdx.x * SEG_PARTIALS + threadIdx.x] = (double)redC[threadIdx.x][0];
  else if (threadIdx.x < SEG_PARTIALS)
    partial[(size_t)blockIdx.x * SEG_PARTIALS + threadIdx.x] = (double)redF[threadIdx.x - 4][0];
}

// Pass 2, one block: this batch's loss terms as bce_dice_finalize_kernel / scalar_sum_finalize_kernel form them
// (rounded to float like the values a training step reports) and its Dice score as dice_metric_finalize_kernel does,
// added to the accumulators; the counts are pooled.  Fixed summation order: the same inputs give the same bits.
__global__ __launch_bounds__(256) void seg_metrics_finalize_kernel(const double* __restrict__ partial, int nb, double n,
                                                                   int lossMode, float wb, float wd, float smooth,
                                                                   double* __restrict__ acc) {
  __shared__ double red[SEG_PARTIALS][256];
  double s[SEG_PARTIALS];
#pragma unroll
  for (int k = 0; k < SEG_PARTIALS; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int k = 0; k < SEG_PARTIALS; ++k) s[k] += partial[(size_t)b * SEG_PARTIALS + k];
#pragma unroll
  for (int k = 0; k < SEG_PARTIALS; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
#pragma unroll
      for (int k = 0; k < SEG_PARTIALS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < SEG_PARTIALS; ++k) s[k] = red[k][0];
  for (int k = 0; k < 4; ++k) acc[k] += s[k];
  const double bce = s[4] / n;
  if (lossMode == 1) {
    const double dice = (2.0 * s[5] + (double)smooth) / (s[6] + s[7] + (double)smooth);
    acc[4] += (double)(float)(wb * bce + wd * (1.0 - dice));
    acc[5] += (double)(float)bce;
    acc[6] += (double)(float)(1.0 - dice);
  } else {
    acc[4] += (double)(float)bce;
    acc[5] += (double)(float)bce;
  }
  // compute_dice: sum pred = TP + FP; sum t and sum pred t as the targets give them (0/1 targets: TP + FN and TP)
  acc[7] += (double)(float)((2.0 * s[8] + (double)smooth) / ((s[0] + s[1]) + s[7] + (double)smooth));
  acc[8] += 1.0;
  acc[9] += n;
}

// BatchNorm in eval form for every conv unit of the network in one launch (one block per unit):
// scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, from the live parameter and buffer
// arrays; channels [C, Cpad) get 0 (the exact-fp32 kernels read scale / shift for their padded columns).
__global__ __launch_bounds__(256) void bn_eval_fold_kernel(const BnFoldDesc* __restrict__ descs, float eps) {
  const BnFoldDesc d = descs[blockIdx.x];
  for (int c = threadIdx.x; c < d.Cpad; c += 256) {
    float sc = 0.f, sh = 0.f;
    if (c < d.C) {
      const double k = (double)d.gamma[c] / sqrt((double)d.var[c] + (double)eps);
      sc = (float)k;
      sh = (float)((double)d.beta[c] - (double)d.mean[c] * k);
    }
    d.scale[c] = sc;
    d.shift[c] = sh;
  }
}

hipError_t launch_bn_eval_fold(const BnFoldDesc* descs, int nDescs, float eps, hipStream_t s) {
  hipLaunchKernelGGL(bn_eval_fold_kernel, dim3(nDescs), dim3(256), 0, s, descs, eps);
  return hipGetLastError();
}

hipError_t launch_seg_metrics(const float* logits, const void* targets, bool targetsU8, size_t numel, float thr,
                              int lossMode, float bceWeight, float diceWeight, float posWeight, float smooth,
                              double* partial, unsigned nb, double* acc, hipStream_t s) {
  if (targetsU8)
    hipLaunchKernelGGL(seg_metrics_partial_kernel<true>, dim3(nb), dim3(256), 0, s, logits, targets, numel, thr, lossMode,
                       posWeight, partial);
  else
    hipLaunchKernelGGL(seg_metrics_partial_kernel<false>, dim3(nb), dim3(256), 0, s, logits, targets, numel, thr, lossMode,
                       posWeight, partial);
  hipLaunchKernelGGL(seg_metrics_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, (int)nb, (double)numel,
                     lossMode, bceWeight, diceWeight, smooth, acc);
  return hipGetLastError();
}

}  // namespace unet
