// Kernels of the histogram calibration pass and of compare_outputs (calib_kernels.h): integer counters and fixed-order
// sums, plain C++, vector stores only.
#include "calib_kernels.h"

#include <math.h>
#include <stdint.h>

namespace unet {

// ---------------------------------------------------------------------------------------------------
// Histogram of one activation tensor (x: npix pixels of c channels at pixel stride ld, as minmax_f32_kernel reads it).
// The binning rule - quant.histogram_model restates it in numpy, bit for bit:
//   t = (v - lo) * inv      one fp32 subtraction, one fp32 multiplication, each rounded on its own;
//                           inv = float(bins) / (hi - lo) comes from the host
//   b = 0 if t < 0;  bins - 1 if t >= bins (before any conversion: +inf is safe);  (int)t otherwise
//   NaN is counted nowhere; v == 0 (either sign) is counted in word `zbin` and in no bin.
// hist: bins + 1 words, zbin = bins.  The kernel adds and never clears.
//
// Exact zeros are about half of every post-ReLU tensor: they stay in a register.  Everything else goes to a
// block-private LDS histogram of 32-bit counters, one copy per wave (4 x 2048 x 4 B = 32 KB; two waves share a copy at
// 4096 bins), and after a barrier the block adds its non-empty bins to `hist` with one 64-bit atomic each.  All
// counters are integers: the result does not depend on the order of anything.
// ---------------------------------------------------------------------------------------------------
constexpr int HIST_LDS_WORDS = 8192;

__global__ __launch_bounds__(256) void histogram_f32_kernel(const float* __restrict__ x, size_t npix, int c, int ld,
                                                            float lo, float inv, int bins, int zbin,
                                                            unsigned long long* __restrict__ hist) {
  __shared__ unsigned sh[HIST_LDS_WORDS];
  __shared__ unsigned shZero;
  const int copies = HIST_LDS_WORDS / bins < 4 ? HIST_LDS_WORDS / bins : 4;
  for (int i = threadIdx.x; i < copies * bins; i += 256) sh[i] = 0;
  if (threadIdx.x == 0) shZero = 0;
  __syncthreads();
  unsigned* mine = sh + ((threadIdx.x >> 6) % copies) * bins;
  const float top = (float)bins;
  unsigned zeros = 0;
  auto count = [&](float v) {
    if (v == 0.f) {
      ++zeros;
      return;
    }
    if (v != v) return;
    const float t = __fmul_rn(__fsub_rn(v, lo), inv);
    const int b = t < 0.f ? 0 : (t >= top ? bins - 1 : (int)t);
    atomicAdd(&mine[b], 1u);
  };
  const size_t total = npix * (size_t)c;
  const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  if (c == ld) {
    // dense: 16-byte loads where the tensor is aligned for them, the last total % 4 elements one by one
    const size_t nvec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? total / 4 : 0;
    for (size_t i = first; i < nvec; i += stride) {
      const float4 v = reinterpret_cast<const float4*>(x)[i];
      count(v.x);
      count(v.y);
      count(v.z);
      count(v.w);
    }
    for (size_t i = nvec * 4 + first; i < total; i += stride) count(x[i]);
  } else {
    for (size_t i = first; i < total; i += stride) {
      const size_t p = i / c;
      count(x[p * ld + (i - p * c)]);
    }
  }
  for (int off = 32; off > 0; off >>= 1) zeros += __shfl_down(zeros, off);
  if ((threadIdx.x & 63) == 0 && zeros) atomicAdd(&shZero, zeros);
  __syncthreads();
  for (int b = threadIdx.x; b < bins; b += 256) {
    unsigned n = 0;
    for (int k = 0; k < copies; ++k) n += sh[k * bins + b];
    if (n) atomicAdd(&hist[b], (unsigned long long)n);
  }
  if (threadIdx.x == 0 && shZero) atomicAdd(&hist[zbin], (unsigned long long)shZero);
}

hipError_t launch_histogram_f32(const float* x, size_t npix, int c, int ld, float lo, float hi, int bins,
                                unsigned long long* hist, hipStream_t s) {
  const float inv = histogram_inv(lo, hi, bins);
  if (!histogram_bins_supported(bins) || !(hi > lo) || !isfinite(lo) || !isfinite(hi) || !isfinite(inv) || !(inv > 0.f) ||
      c < 1 || c > ld)
    return hipErrorInvalidValue;
  const size_t total = npix * (size_t)c;
  if (total == 0) return hipSuccess;
  if (total >> 41) return hipErrorInvalidValue;   // a block's 32-bit counters (histogram_grid)
  hipLaunchKernelGGL(histogram_f32_kernel, dim3(histogram_grid(total)), dim3(256), 0, s, x, npix, c, ld, lo, inv, bins,
                     bins, hist);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// compare_outputs (reference README.md:3512-3565): sum over one frame of |p_a - p_b|.  Pass 1: blockIdx.y = frame,
// MAE_BLOCKS_PER_FRAME blocks each reduce their stripes to one double.  Pass 2: one block per frame adds the partials
// in index order to the frame's accumulator.  Fixed summation order: the same inputs give the same bits.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prob_mae_partial_kernel(const float* __restrict__ pa, const float* __restrict__ pb,
                                                               size_t perFrame, double* __restrict__ partial) {
  const float* a = pa + (size_t)blockIdx.y * perFrame;
  const float* b = pb + (size_t)blockIdx.y * perFrame;
  double acc = 0.0;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < perFrame; i += stride) acc += (double)fabsf(a[i] - b[i]);
  __shared__ double red[256];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void prob_mae_finalize_kernel(const double* __restrict__ partial, int nb,
                                                               double* __restrict__ acc) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int k = 0; k < nb; ++k) s += partial[(size_t)blockIdx.x * nb + k];
  acc[blockIdx.x] += s;
}

hipError_t launch_prob_mae(const float* pa, const float* pb, int frames, size_t perFrame, double* partial, double* acc,
                           hipStream_t s) {
  hipLaunchKernelGGL(prob_mae_partial_kernel, dim3(MAE_BLOCKS_PER_FRAME, (unsigned)frames), dim3(256), 0, s, pa, pb,
                     perFrame, partial);
  hipLaunchKernelGGL(prob_mae_finalize_kernel, dim3((unsigned)frames), dim3(64), 0, s, (const double*)partial,
                     (int)MAE_BLOCKS_PER_FRAME, acc);
  return hipGetLastError();
}

}  // namespace unet
