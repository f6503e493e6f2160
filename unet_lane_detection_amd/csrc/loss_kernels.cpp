// Kernels of the general training loss and of the mask statistics (loss_kernels.h), in the style of
// validate_kernels.cpp: two-stage deterministic reductions, no float atomics, plain C++, vector stores only.
#include "loss_kernels.h"

#include <algorithm>
#include <cmath>

// One expression tree, one rounding sequence: the training step, the test operator and the validation pass instantiate
// the same element functions and must produce the same bits, so no instantiation may fuse a multiply-add another does not.
#pragma clang fp contract(off)

namespace unet {

namespace {

constexpr int LOSS_PARTIALS = 5;     // per block: {BCE(pos_weight) sum, focal sum, sum s t, sum s, sum t}
constexpr int SEG_CFG_PARTIALS = 10; // ... + {TP, FP, FN, TN, sum pred t}
constexpr unsigned LOSS_MAX_BLOCKS = 2048;   // 8 per CU
constexpr size_t SCRATCH_HEAD = 16;  // bytes in front of the partials: the two Dice coefficients of the gradient pass

// Elements are handled in groups of 4 consecutive ones per thread, as one 128-bit access where the pointers allow it and
// element by element otherwise (and in the last, incomplete group): the summation order depends on numel only, not on
// the alignment of the buffers or on the type of the targets.
inline size_t groups_of(size_t numel) { return (numel + 3) / 4; }
inline unsigned loss_blocks(size_t numel) {
  return (unsigned)std::min<size_t>(std::max<size_t>((groups_of(numel) + 255) / 256, 1), LOSS_MAX_BLOCKS);
}
inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

bool loss_params_valid(const LossParams& p) {
  const float v[7] = {p.wb, p.wf, p.wd, p.pw, p.alpha, p.gamma, p.smooth};
  for (float f : v)
    if (!std::isfinite(f)) return false;
  if (p.wb < 0.f || p.wf < 0.f || p.wd < 0.f || (p.wb == 0.f && p.wf == 0.f && p.wd == 0.f)) return false;
  if (!(p.pw > 0.f) || p.alpha < 0.f || p.alpha > 1.f || !(p.smooth > 0.f)) return false;
  return p.gamma == 0.f || p.gamma >= 1.f;
}

size_t loss_scratch_bytes(size_t numel) { return SCRATCH_HEAD + (size_t)loss_blocks(numel) * LOSS_PARTIALS * sizeof(double); }
size_t seg_metrics_cfg_scratch_bytes(size_t numel) {
  return SCRATCH_HEAD + (size_t)loss_blocks(numel) * SEG_CFG_PARTIALS * sizeof(double);
}

// ---------------------------------------------------------------------------------------------------
// Per element, x the logit, t the target in [0, 1] (reference README.md:1694-1709 BCE, :1781-1807 Dice,
// :1914-1939 FocalLoss):
//   e = exp(-|x|);  p = sigmoid(x) = x >= 0 ? 1/(1+e) : e/(1+e);  1-p = x >= 0 ? e/(1+e) : 1/(1+e)
//   ce  = max(x,0) - x t + log1p(e)                       BCE-with-logits, unweighted
//   q   = 1 - p_t = p (1-t) + (1-p) t                     a sum of products: no cancellation where p_t -> 1
//   a_t = alpha t + (1-alpha) (1-t)
//   focal_i = a_t q^gamma ce
//   d focal_i / dx = a_t ( gamma q^(gamma-1) p (1-p) (1-2t) ce + q^gamma (p - t) ),   p - t = p (1-t) - (1-p) t
// Where e underflows (|x| > ~104) p or 1-p is exactly 0 and every factor above stays finite: gamma >= 1 keeps the
// exponent gamma - 1 non-negative, gamma == 0 evaluates no power at all.
// ---------------------------------------------------------------------------------------------------
struct Sig {
  float p, omp, l1p;
};

__device__ __forceinline__ Sig sigmoid_parts(float x) {
  const float e = expf(-fabsf(x));
  const float inv = 1.f / (1.f + e), einv = e / (1.f + e);
  Sig s;
  s.p = x >= 0.f ? inv : einv;
  s.omp = x >= 0.f ? einv : inv;
  s.l1p = log1pf(e);
  return s;
}

// q^(gamma-1) and q^gamma for gamma >= 1, 0 <= q <= 1
__device__ __forceinline__ void focal_powers(float q, float gamma, float& qgm1, float& qg) {
  if (gamma == 2.f) qgm1 = q;
  else if (gamma == 1.f) qgm1 = 1.f;
  else qgm1 = powf(q, gamma - 1.f);
  qg = qgm1 * q;
}

// adds this element's five sums
__device__ __forceinline__ void loss_accumulate(float x, float t, const LossParams& P, float (&acc)[LOSS_PARTIALS]) {
  const Sig s = sigmoid_parts(x);
  // log s = min(x,0) - log1p(e),  log(1-s) = -max(x,0) - log1p(e)   (bce_dice_partial_kernel, term by term)
  const float logs = fminf(x, 0.f) - s.l1p, log1ms = -fmaxf(x, 0.f) - s.l1p;
  acc[0] += -(P.pw * t * logs + (1.f - t) * log1ms);
  const float ce = fmaxf(x, 0.f) - x * t + s.l1p;
  const float at = P.alpha * t + (1.f - P.alpha) * (1.f - t);
  float mod = 1.f;
  if (P.gamma != 0.f) {
    const float q = s.p * (1.f - t) + s.omp * t;
    float qgm1;
    focal_powers(q, P.gamma, qgm1, mod);
  }
  acc[1] += at * mod * ce;
  acc[2] += s.p * t;
  acc[3] += s.p;
  acc[4] += t;
}

__device__ __forceinline__ float loss_gradient(float x, float t, const LossParams& P, float wbOverN, float wfOverN,
                                               float invDen, float numOverDen2) {
  const Sig s = sigmoid_parts(x);
  float g = 0.f;
  if (P.wb != 0.f) g += wbOverN * (s.p * (1.f - t + P.pw * t) - P.pw * t);
  if (P.wf != 0.f) {
    const float at = P.alpha * t + (1.f - P.alpha) * (1.f - t);
    const float pmt = s.p * (1.f - t) - s.omp * t;
    float d = pmt;
    if (P.gamma != 0.f) {
      const float ce = fmaxf(x, 0.f) - x * t + s.l1p;
      const float q = s.p * (1.f - t) + s.omp * t;
      float qgm1, qg;
      focal_powers(q, P.gamma, qgm1, qg);
      d = P.gamma * qgm1 * (s.p * s.omp) * (1.f - 2.f * t) * ce + qg * pmt;
    }
    g += wfOverN * (at * d);
  }
  if (P.wd != 0.f) g -= P.wd * ((s.p * s.omp) * (2.f * t * invDen - numOverDen2));   // dDice/dx as bce_dice_grad_kernel
  return g;
}

// one group of up to 4 consecutive elements
template <bool U8>
__device__ __forceinline__ int load_group(const float* __restrict__ x, const void* __restrict__ tRaw, size_t g, size_t n,
                                          int vec, float (&xv)[4], float (&tv)[4]) {
  const size_t i0 = g * 4;
  const int cnt = n - i0 >= 4 ? 4 : (int)(n - i0);
  if (vec && cnt == 4) {
    const float4 a = *reinterpret_cast<const float4*>(x + i0);
    xv[0] = a.x, xv[1] = a.y, xv[2] = a.z, xv[3] = a.w;
    if (U8) {
      const uchar4 b = *reinterpret_cast<const uchar4*>(static_cast<const uint8_t*>(tRaw) + i0);
      tv[0] = b.x != 0 ? 1.f : 0.f, tv[1] = b.y != 0 ? 1.f : 0.f, tv[2] = b.z != 0 ? 1.f : 0.f, tv[3] = b.w != 0 ? 1.f : 0.f;
    } else {
      const float4 b = *reinterpret_cast<const float4*>(static_cast<const float*>(tRaw) + i0);
      tv[0] = b.x, tv[1] = b.y, tv[2] = b.z, tv[3] = b.w;
    }
  } else {
    for (int k = 0; k < 4; ++k) {
      xv[k] = tv[k] = 0.f;
      if (k < cnt) {
        xv[k] = x[i0 + k];
        tv[k] = U8 ? (static_cast<const uint8_t*>(tRaw)[i0 + k] != 0 ? 1.f : 0.f) : static_cast<const float*>(tRaw)[i0 + k];
      }
    }
  }
  return cnt;
}

// Pass 1: per block LOSS_PARTIALS doubles; with METRICS the validation pass's confusion counts and sum pred t as well
// (seg_metrics_partial_kernel: pred = x > thr, truth = t > 0.5), from the same read.  Threads accumulate in float, as
// the kernels of modes 0 and 1 do; everything across threads is added in double.
template <bool U8, bool METRICS>
__global__ __launch_bounds__(256) void loss_partial_kernel(const float* __restrict__ x, const void* __restrict__ tRaw,
                                                           size_t n, int vec, float thr, LossParams P,
                                                           double* __restrict__ partial) {
  constexpr int K = METRICS ? SEG_CFG_PARTIALS : LOSS_PARTIALS;
  float acc[LOSS_PARTIALS] = {0.f, 0.f, 0.f, 0.f, 0.f};
  unsigned long long cnt[4] = {0, 0, 0, 0};
  float predT = 0.f;
  const size_t groups = (n + 3) / 4, stride = (size_t)gridDim.x * 256;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += stride) {
    float xv[4], tv[4];
    const int c = load_group<U8>(x, tRaw, g, n, vec, xv, tv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < c) {
        loss_accumulate(xv[k], tv[k], P, acc);
        if (METRICS) {
          const bool pred = xv[k] > thr, truth = tv[k] > 0.5f;
          cnt[0] += pred && truth;
          cnt[1] += pred && !truth;
          cnt[2] += !pred && truth;
          cnt[3] += !pred && !truth;
          predT += pred ? tv[k] : 0.f;
        }
      }
    }
  }
  __shared__ double red[K][256];
#pragma unroll
  for (int k = 0; k < LOSS_PARTIALS; ++k) red[k][threadIdx.x] = (double)acc[k];
  if (METRICS) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[LOSS_PARTIALS + k][threadIdx.x] = (double)cnt[k];   // exact below 2^53
    red[K - 1][threadIdx.x] = (double)predT;
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < K) partial[(size_t)blockIdx.x * K + threadIdx.x] = red[threadIdx.x][0];
}

// column sums of the [nb][K] partials in a fixed order (the same for every K); the result is valid in thread 0
template <int K>
__device__ __forceinline__ void column_sums(const double* __restrict__ partial, int nb, double (&s)[K], double (*red)[256]) {
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += partial[(size_t)b * K + k];
#pragma unroll
  for (int k = 0; k < K; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
#pragma unroll
      for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = red[k][0];
}

// the four loss values, rounded to float as a training step reports them, and the Dice coefficients of the gradient:
// coef[0] = 1/(P+T+eps), coef[1] = (2I+eps)/(P+T+eps)^2  (bce_dice_finalize_kernel)
__device__ __forceinline__ void loss_values(const double* s, double n, const LossParams& P, float (&out)[4], float (&coef)[2]) {
  const double bce = s[0] / n, focal = s[1] / n;
  const double den = s[3] + s[4] + (double)P.smooth;
  const double dice = (2.0 * s[2] + (double)P.smooth) / den;
  out[0] = (float)((double)P.wb * bce + (double)P.wf * focal + (double)P.wd * (1.0 - dice));
  out[1] = (float)bce;
  out[2] = (float)(1.0 - dice);
  out[3] = (float)focal;
  coef[0] = (float)(1.0 / den);
  coef[1] = (float)((2.0 * s[2] + (double)P.smooth) / (den * den));
}

__global__ __launch_bounds__(256) void loss_finalize_kernel(const double* __restrict__ partial, int nb, double n,
                                                            LossParams P, float* __restrict__ out4,
                                                            float* __restrict__ coefOut) {
  __shared__ double red[LOSS_PARTIALS][256];
  double s[LOSS_PARTIALS];
  column_sums<LOSS_PARTIALS>(partial, nb, s, red);
  if (threadIdx.x != 0) return;
  float out[4], coef[2];
  loss_values(s, n, P, out, coef);
  for (int k = 0; k < 4; ++k) out4[k] = out[k];
  coefOut[0] = coef[0];
  coefOut[1] = coef[1];
}

// Pass 2 of the validation reduction (seg_metrics_finalize_kernel with the general loss)
__global__ __launch_bounds__(256) void seg_metrics_cfg_finalize_kernel(const double* __restrict__ partial, int nb, double n,
                                                                       LossParams P, double* __restrict__ acc) {
  __shared__ double red[SEG_CFG_PARTIALS][256];
  double s[SEG_CFG_PARTIALS];
  column_sums<SEG_CFG_PARTIALS>(partial, nb, s, red);
  if (threadIdx.x != 0) return;
  float out[4], coef[2];
  loss_values(s, n, P, out, coef);
  for (int k = 0; k < 4; ++k) acc[k] += s[LOSS_PARTIALS + k];
  acc[4] += (double)out[0];
  acc[5] += (double)out[1];
  acc[6] += (double)out[2];
  acc[10] += (double)out[3];
  // compute_dice: sum pred = TP + FP
  acc[7] += (double)(float)((2.0 * s[SEG_CFG_PARTIALS - 1] + (double)P.smooth) /
                            ((s[LOSS_PARTIALS] + s[LOSS_PARTIALS + 1]) + s[4] + (double)P.smooth));
  acc[8] += 1.0;
  acc[9] += n;
}

// Pass 3: dL/dx
__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ x, const float* __restrict__ t, size_t n,
                                                        int vec, LossParams P, float wbOverN, float wfOverN,
                                                        const float* __restrict__ coef, float* __restrict__ dx) {
  const float invDen = coef[0], numOverDen2 = coef[1];
  const size_t groups = (n + 3) / 4, stride = (size_t)gridDim.x * 256;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += stride) {
    float xv[4], tv[4], gv[4];
    const int c = load_group<false>(x, t, g, n, vec, xv, tv);
#pragma unroll
    for (int k = 0; k < 4; ++k) gv[k] = loss_gradient(xv[k], tv[k], P, wbOverN, wfOverN, invDen, numOverDen2);
    if (vec && c == 4) {
      *reinterpret_cast<float4*>(dx + g * 4) = make_float4(gv[0], gv[1], gv[2], gv[3]);
    } else {
      for (int k = 0; k < c; ++k) dx[g * 4 + k] = gv[k];
    }
  }
}

hipError_t launch_loss_grad(const float* logits, const float* targets, size_t numel, const LossParams& p, void* scratch,
                            float* out4, float* dx, hipStream_t s) {
  const unsigned nb = loss_blocks(numel);
  float* coef = static_cast<float*>(scratch);
  double* partial = reinterpret_cast<double*>(static_cast<char*>(scratch) + SCRATCH_HEAD);
  const int vecIn = aligned(logits, 16) && aligned(targets, 16);
  hipLaunchKernelGGL((loss_partial_kernel<false, false>), dim3(nb), dim3(256), 0, s, logits, (const void*)targets, numel, vecIn,
                     0.f, p, partial);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, (int)nb, (double)numel, p, out4,
                     coef);
  const unsigned gb = (unsigned)std::min<size_t>(std::max<size_t>((groups_of(numel) + 255) / 256, 1), 4 * LOSS_MAX_BLOCKS);
  hipLaunchKernelGGL(loss_grad_kernel, dim3(gb), dim3(256), 0, s, logits, targets, numel, vecIn && aligned(dx, 16) ? 1 : 0, p,
                     (float)((double)p.wb / (double)numel), (float)((double)p.wf / (double)numel), (const float*)coef, dx);
  return hipGetLastError();
}

hipError_t launch_seg_metrics_cfg(const float* logits, const void* targets, bool targetsU8, size_t numel, float thr,
                                  const LossParams& p, void* scratch, double* acc, hipStream_t s) {
  const unsigned nb = loss_blocks(numel);
  double* partial = reinterpret_cast<double*>(static_cast<char*>(scratch) + SCRATCH_HEAD);
  const int vec = aligned(logits, 16) && aligned(targets, targetsU8 ? 4 : 16);
  if (targetsU8)
    hipLaunchKernelGGL((loss_partial_kernel<true, true>), dim3(nb), dim3(256), 0, s, logits, targets, numel, vec, thr, p,
                       partial);
  else
    hipLaunchKernelGGL((loss_partial_kernel<false, true>), dim3(nb), dim3(256), 0, s, logits, targets, numel, vec, thr, p,
                       partial);
  hipLaunchKernelGGL(seg_metrics_cfg_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, (int)nb,
                     (double)numel, p, acc);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Positive pixels per mask (reference README.md:2514-2530 `calculate_pos_weight`: (mask > 127).sum(); :2544-2553
// `get_sample_weights`: the same count behind mask.mean() of a 0/1 mask).  One pass over the bytes; blockIdx.y walks
// the images, blockIdx.x the chunks of one image; a block's count is added to its image's counter with one integer
// atomic - integer addition is exact and order-free, so the result is deterministic.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_positive_counts_kernel(const uint8_t* __restrict__ masks, int n, size_t ppi,
                                                                   int threshold, int vec,
                                                                   unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long red[256];
  for (int img = blockIdx.y; img < n; img += gridDim.y) {
    const uint8_t* m = masks + (size_t)img * ppi;
    unsigned long long c = 0;
    const size_t stride = (size_t)gridDim.x * 256;
    if (vec) {   // ppi % 16 == 0 and a 16-byte aligned base: every image starts aligned
      const size_t words = ppi / 16;
      for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < words; w += stride) {
        const uint4 v = *reinterpret_cast<const uint4*>(m + w * 16);
        const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int b = 0; b < 4; ++b) c += (int)((u[k] >> (8 * b)) & 0xffu) > threshold;
      }
    } else {
      for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < ppi; i += stride) c += (int)m[i] > threshold;
    }
    red[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0 && red[0] != 0) atomicAdd(&counts[img], red[0]);
    __syncthreads();
  }
}

hipError_t launch_mask_positive_counts(const uint8_t* masks, int n, size_t pixelsPerImage, int threshold,
                                       unsigned long long* counts, hipStream_t s) {
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  const int vec = pixelsPerImage % 16 == 0 && aligned(masks, 16);
  const size_t perThread = vec ? 16 : 1;
  // about 64 bytes (4 words) per thread, at most 64 blocks per image
  const unsigned bx = (unsigned)std::min<size_t>(std::max<size_t>((pixelsPerImage + 256 * perThread * 4 - 1) / (256 * perThread * 4), 1), 64);
  const unsigned by = (unsigned)std::min(n, 32768);
  hipLaunchKernelGGL(mask_positive_counts_kernel, dim3(bx, by), dim3(256), 0, s, masks, n, pixelsPerImage, threshold, vec,
                     counts);
  return hipGetLastError();
}

}  // namespace unet
