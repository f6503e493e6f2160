// Multi-class segmentation kernels (multiclass_kernels.h) and their operator entry points.
//
// headk_kernel<LPP, KP, PLANES>.  LPP lanes share a pixel as in head1x1_kernel<LPP>: lane `sub` takes the float4 slices
// sub * 4, sub * 4 + LPP * 4, ... of the channel vector (16-byte loads), one fp32 FMA chain in ascending c per class,
// then the xor tree over the LPP lanes; the bias is added behind the tree.  The K * C weights (at most MC_MAX_WEIGHTS
// floats) are copied to LDS once per block.  KP is K rounded up to 2, 4 or 8: the accumulators are registers.  A block
// takes 256 / LPP consecutive pixels between two barriers (staging 64 pixels by unrolled rounds of the lane groups was
// measured and was slower: profiles/r30/multiclass.md); the first lane of a pixel puts its K logits (and, where asked, the
// softmax and the argmax) into LDS, and all 256 threads then store plane by plane, consecutive threads to consecutive
// pixels: coalesced along W for every K.  softmax: exp(z_k - max z) / sum with expf and an IEEE division.  argmax: scan
// from class 0 with `>` against -inf, so ties go to the lowest index and a NaN never wins.  PLANES: the same kernel on
// the f16x3 tier's fp16 hi + lo planes; a lane's step is then eight channels (16 bytes of each plane), x = hi + lo.
//
// class_loss_partial_kernel / class_loss_finalize_kernel / class_loss_grad_kernel.  One thread per pixel, grid stride
// over a grid that mc_red_blocks fixes.  Pass 1 adds, per thread in double, the 3 K + 3 sums (per class: sum of p_k over
// the valid pixels, sum of p_k over those labelled k, their number; the weighted cross-entropy numerator and
// denominator; the number of out-of-range labels), the block adds its threads' sums (xor tree per wave, the four waves
// in order) and stores one row.  The finalize - one block - adds the rows (thread t rows t, t + 256, ..., the same
// tree), forms the loss terms and the gradient's coefficients in double.  Pass 2 recomputes the softmax and writes
//   dl_k = ce_w cw[t] (p_k - [t = k]) / denom + p_k (g_k - sum_j p_j g_j),   g_k = dDice/dp_k = A_k [t = k] + B_k
// for a valid pixel and 0 for any other.  logsumexp is formed with the maximum subtracted: exp's arguments are <= 0 and
// the sum lies in [1, K], so no finite logit produces NaN or Inf.
//
// headk_bwd_kernel<KP> / headk_bwd_finalize_kernel.  Block b takes the pixels [b * per, (b + 1) * per); thread (r, c)
// takes float4 column c of the rows r, r + rows, ... of that range: dA = sum_k dl_k w_k (stored), dW_k += dl_k a and
// db_k += dl_k in registers.  The rows of a block are added through LDS in row order, the blocks' partials by the
// finalize in double (16 parts per output, parts in order).
//
// confusion_kernel / confusion_finalize_kernel.  Per-wave 32-bit counters in LDS (LDS atomics only), flushed as one row
// of K * K counts per block; the finalize adds the rows in 64-bit integers TO the caller's accumulators.
//
// Bounds.  Every pixel index is below P = n * hw by the loop conditions; plane offsets are (img * K + k) * hw + pix with
// img < n, k < K, pix < hw.  LDS: K * C <= MC_MAX_WEIGHTS is checked by every launcher; t * K + p < K * K <= 64.
#include "multiclass_kernels.h"

#include "op_entry.h"

#include <cmath>

namespace unet {

namespace {

typedef unsigned long long u64;
typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }

inline unsigned mc_grid(size_t items, size_t perBlock) {
  const size_t b = (items + perBlock - 1) / perBlock;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));   // 8 blocks per CU, then the grid stride
}

// ---------------------------------------------------------------------------------------------------------------------
// the K-way head
// ---------------------------------------------------------------------------------------------------------------------
struct HeadKArgs {
  const float* x;          // fp32 input, or
  const uint32_t* hi;      // fp16 hi plane of the f16x3 tier, two channels per word; the lo plane lo2 words behind
  size_t lo2;
  const float* w;
  const float* b;
  size_t npix, hw;
  int C, K, maskClass;
  float* logits;
  float* probs;
  uint8_t* labels;
  uint8_t* mask;
};

// softmax and argmax of K logits in registers: softmax_argmax of multiclass_kernels.h

// (hi, lo) packed fp16 pairs -> the two fp32 values they stand for (merge_pk_f16 of conv_x3_ws.h)
__device__ __forceinline__ void merge_pair(uint32_t hi, uint32_t lo, float& v0, float& v1) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  const f32x2 h = __builtin_convertvector(__builtin_bit_cast(f16x2, hi), f32x2);
  const f32x2 l = __builtin_convertvector(__builtin_bit_cast(f16x2, lo), f32x2);
  v0 = h[0] + l[0];
  v1 = h[1] + l[1];
}

// PLANES: the input is the f16x3 tier's operand planes (the layout head1x1_planes_kernel reads); a lane then takes eight
// channels per step, 16 bytes of each plane
template <int LPP, int KP, bool PLANES>
__global__ __launch_bounds__(256) void headk_kernel(const HeadKArgs a) {
  constexpr int PPB = 256 / LPP;
  constexpr int STEP = PLANES ? 8 : 4;
  constexpr int SPB = PPB;   // pixels staged between two barriers
  extern __shared__ f4 mcSmem[];
  float* sw = reinterpret_cast<float*>(mcSmem);   // K * C weights
  __shared__ float sz[KP][SPB];
  __shared__ float sp[KP][SPB];
  __shared__ uint8_t sl[SPB];
  __shared__ float sb[KP];
  const int tid = threadIdx.x, sub = tid % LPP, pl = tid / LPP;
  const int C = a.C, K = a.K;
  for (int i = tid; i < K * C; i += 256) sw[i] = a.w[i];
  if (tid < KP) sb[tid] = tid < K ? a.b[tid] : 0.f;
  __syncthreads();
  const bool soft = a.probs || a.labels || a.mask;
  for (size_t base = (size_t)blockIdx.x * SPB; base < a.npix; base += (size_t)gridDim.x * SPB) {
    const int pq = pl;
    const size_t p = base + pq;
    float acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.f;
    if (p < a.npix) {
      for (int ch = sub * STEP; ch < C; ch += LPP * STEP) {
        float xv[STEP];
        if constexpr (PLANES) {
          const uint32_t* q = a.hi + (p * (size_t)C + ch) / 2;
          const uint4 h4 = *reinterpret_cast<const uint4*>(q), l4 = *reinterpret_cast<const uint4*>(q + a.lo2);
          merge_pair(h4.x, l4.x, xv[0], xv[1]);
          merge_pair(h4.y, l4.y, xv[2], xv[3]);
          merge_pair(h4.z, l4.z, xv[4], xv[5]);
          merge_pair(h4.w, l4.w, xv[6], xv[7]);
        } else {
          const f4 v = ld4(a.x + p * (size_t)C + ch);
          xv[0] = v[0], xv[1] = v[1], xv[2] = v[2], xv[3] = v[3];
        }
#pragma unroll
        for (int k = 0; k < KP; ++k)
          if (k < K) {
#pragma unroll
            for (int e = 0; e < STEP; e += 4) {
              const f4 wv = ld4(sw + k * C + ch + e);
              acc[k] = fmaf(xv[e], wv[0], acc[k]);
              acc[k] = fmaf(xv[e + 1], wv[1], acc[k]);
              acc[k] = fmaf(xv[e + 2], wv[2], acc[k]);
              acc[k] = fmaf(xv[e + 3], wv[3], acc[k]);
            }
          }
      }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k)
#pragma unroll
      for (int d = LPP >> 1; d > 0; d >>= 1) acc[k] += __shfl_xor(acc[k], d, 64);
    if (sub == 0 && p < a.npix) {
      float z[KP], pr[KP];
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        z[k] = acc[k] + sb[k];
        sz[k][pq] = z[k];
      }
      if (soft) {
        const int label = softmax_argmax<KP>(z, K, pr);
#pragma unroll
        for (int k = 0; k < KP; ++k) sp[k][pq] = pr[k];
        sl[pq] = (uint8_t)label;
      }
    }
    __syncthreads();
    const size_t left = a.npix - base;
    const int cnt = left < (size_t)SPB ? (int)left : SPB;
    for (int i = tid; i < K * SPB; i += 256) {
      const int k = i / SPB, q = i - k * SPB;
      if (q < cnt) {
        const size_t pp = base + q, img = pp / a.hw, pix = pp - img * a.hw;
        const size_t o = (img * K + k) * a.hw + pix;
        if (a.logits) a.logits[o] = sz[k][q];
        if (a.probs) a.probs[o] = sp[k][q];
      }
    }
    if (tid < cnt) {
      if (a.labels) a.labels[base + tid] = sl[tid];
      if (a.mask) a.mask[base + tid] = sl[tid] == a.maskClass ? 255 : 0;
    }
    __syncthreads();
  }
}

template <int LPP, bool PLANES>
void launch_headk_lpp(const HeadKArgs& a, hipStream_t s) {
  const unsigned g = mc_grid(a.npix, 256 / LPP);
  const size_t lds = (size_t)a.K * a.C * sizeof(float);
  if (a.K <= 2)
    hipLaunchKernelGGL((headk_kernel<LPP, 2, PLANES>), dim3(g), dim3(256), lds, s, a);
  else if (a.K <= 4)
    hipLaunchKernelGGL((headk_kernel<LPP, 4, PLANES>), dim3(g), dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL((headk_kernel<LPP, 8, PLANES>), dim3(g), dim3(256), lds, s, a);
}

// the lanes of a pixel: as many as the channel vector has steps, 16 at the most (head1x1_kernel's rule for STEP = 4)
template <bool PLANES>
hipError_t launch_headk_any(const HeadKArgs& a, hipStream_t s) {
  constexpr int STEP = PLANES ? 8 : 4;
  int lpp = 1;
  while (lpp < 16 && lpp * 2 * STEP <= a.C) lpp *= 2;
  switch (lpp) {
    case 1: launch_headk_lpp<1, PLANES>(a, s); break;
    case 2: launch_headk_lpp<2, PLANES>(a, s); break;
    case 4: launch_headk_lpp<4, PLANES>(a, s); break;
    case 8: launch_headk_lpp<8, PLANES>(a, s); break;
    default: launch_headk_lpp<16, PLANES>(a, s); break;
  }
  return hipGetLastError();
}

// labels / class mask of stored logits (n, K, hw): the head's argmax, one thread per pixel
__global__ __launch_bounds__(256) void class_labels_kernel(const float* __restrict__ z, size_t P, size_t hw, int K,
                                                           uint8_t* __restrict__ labels, int maskClass,
                                                           uint8_t* __restrict__ mask) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < P; p += stride) {
    const size_t img = p / hw, pix = p - img * hw;
    const float* zp = z + img * K * hw + pix;
    float best = -INFINITY;
    int label = 0;
    for (int k = 0; k < K; ++k) {
      const float v = zp[(size_t)k * hw];
      if (v > best) {
        best = v;
        label = k;
      }
    }
    if (labels) labels[p] = (uint8_t)label;
    if (mask) mask[p] = label == maskClass ? 255 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the class loss
// ---------------------------------------------------------------------------------------------------------------------
constexpr int LOSS_NQ = 3 * MC_MAX_CLASSES + 3;   // row length of the partials, whatever K
constexpr int Q_S = 0, Q_I = MC_MAX_CLASSES, Q_T = 2 * MC_MAX_CLASSES, Q_NUM = 3 * MC_MAX_CLASSES, Q_DEN = Q_NUM + 1,
              Q_BAD = Q_NUM + 2;
// coefficients behind the partials: [0] ce_w / denom, [1 + k] A_k, [1 + MAX + k] B_k
constexpr int COEF_FLOATS = 1 + 2 * MC_MAX_CLASSES;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// the block's 256 values of each of NQ quantities into thread q's return value (threads 0 .. NQ - 1), in a fixed order
template <int NQ>
__device__ __forceinline__ double block_sums(const double (&acc)[NQ], double (*sh)[NQ]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double v = wave_sum(acc[q]);
    if (lane == 0) sh[wave][q] = v;
  }
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x < NQ) r = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
  __syncthreads();
  return r;
}

struct PixelSoftmax {
  bool valid, bad;
  int t;
  float cw;
};

// label of pixel p: valid (below K and not ignored) or counted as out of range
__device__ __forceinline__ PixelSoftmax classify(uint8_t lab, int K, const ClassLossParams& prm) {
  PixelSoftmax r;
  r.t = lab;
  const bool ign = (int)lab == prm.ignore;
  r.valid = (int)lab < K && !ign;
  r.bad = (int)lab >= K && !ign;
  r.cw = 0.f;
#pragma unroll
  for (int k = 0; k < MC_MAX_CLASSES; ++k) r.cw = (k == (int)lab) ? prm.cw[k] : r.cw;
  return r;
}

template <int KP>
__global__ __launch_bounds__(256) void class_loss_partial_kernel(const float* __restrict__ z, const uint8_t* __restrict__ lab,
                                                                 size_t P, size_t hw, int K, const ClassLossParams prm,
                                                                 double* __restrict__ partial) {
  constexpr int NQ = 3 * KP + 3;
  __shared__ double sh[4][NQ];
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < P; p += stride) {
    const PixelSoftmax px = classify(lab[p], K, prm);
    if (px.bad) acc[3 * KP + 2] += 1.0;
    if (!px.valid) continue;
    const size_t img = p / hw, pix = p - img * hw;
    const float* zp = z + img * K * hw + pix;
    float zz[KP], e[KP];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      zz[k] = k < K ? zp[(size_t)k * hw] : -INFINITY;
      m = fmaxf(m, zz[k]);
    }
    float sum = 0.f, zt = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      e[k] = k < K ? expf(zz[k] - m) : 0.f;
      sum += e[k];
      zt = (k == px.t) ? zz[k] : zt;
    }
    const float lse = m + logf(sum);
    acc[3 * KP] += (double)(px.cw * (lse - zt));
    acc[3 * KP + 1] += (double)px.cw;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const double pk = (double)(e[k] / sum);
      acc[k] += pk;
      if (k == px.t) {
        acc[KP + k] += pk;
        acc[2 * KP + k] += 1.0;
      }
    }
  }
  const double r = block_sums<NQ>(acc, sh);
  // thread q of the KP-sized row -> its place in the MC_MAX_CLASSES-sized row
  if (threadIdx.x < NQ) {
    const int q = threadIdx.x, grp = q / KP, k = q - grp * KP;
    const int dst = grp < 3 ? grp * MC_MAX_CLASSES + k : Q_NUM + (q - 3 * KP);
    partial[(size_t)blockIdx.x * LOSS_NQ + dst] = r;
  }
}

__global__ __launch_bounds__(256) void class_loss_finalize_kernel(const double* __restrict__ partial, int nb, int K,
                                                                  const ClassLossParams prm, float* __restrict__ lossDev,
                                                                  float* __restrict__ coef) {
  __shared__ double sh[4][LOSS_NQ];
  __shared__ double tot[LOSS_NQ];
  double acc[LOSS_NQ];
#pragma unroll
  for (int q = 0; q < LOSS_NQ; ++q) acc[q] = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) {
#pragma unroll
    for (int q = 0; q < LOSS_NQ; ++q) {
      const int grp = q / MC_MAX_CLASSES, k = q - grp * MC_MAX_CLASSES;
      if (grp == 3 || k < K) acc[q] += partial[(size_t)b * LOSS_NQ + q];   // rows hold nothing for k >= K
    }
  }
  const double r = block_sums<LOSS_NQ>(acc, sh);
  if (threadIdx.x < LOSS_NQ) tot[threadIdx.x] = r;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double den = tot[Q_DEN];
  const double ce = den > 0.0 ? tot[Q_NUM] / den : 0.0;
  const double sm = (double)prm.smooth;
  double mean = 0.0;
  for (int k = 0; k < K; ++k) {
    const double u = tot[Q_S + k] + tot[Q_T + k] + sm;
    const double d = (2.0 * tot[Q_I + k] + sm) / u;
    mean += d;
    coef[1 + k] = (float)(-(double)prm.diceW / K * 2.0 / u);
    coef[1 + MC_MAX_CLASSES + k] = (float)((double)prm.diceW / K * d / u);
  }
  const double dice = 1.0 - mean / K;
  coef[0] = den > 0.0 ? (float)((double)prm.ceW / den) : 0.f;
  lossDev[0] = (float)((double)prm.ceW * ce + (double)prm.diceW * dice);
  lossDev[1] = (float)ce;
  lossDev[2] = (float)dice;
  lossDev[3] = (float)tot[Q_BAD];
}

template <int KP>
__global__ __launch_bounds__(256) void class_loss_grad_kernel(const float* __restrict__ z, const uint8_t* __restrict__ lab,
                                                              size_t P, size_t hw, int K, const ClassLossParams prm,
                                                              const float* __restrict__ coef, float* __restrict__ dl) {
  const float ceScale = coef[0];
  float A[KP], B[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    A[k] = k < K ? coef[1 + k] : 0.f;
    B[k] = k < K ? coef[1 + MC_MAX_CLASSES + k] : 0.f;
  }
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < P; p += stride) {
    const PixelSoftmax px = classify(lab[p], K, prm);
    const size_t img = p / hw, pix = p - img * hw;
    const size_t o = img * K * hw + pix;
    float g[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) g[k] = 0.f;
    if (px.valid) {
      float zz[KP], pr[KP];
#pragma unroll
      for (int k = 0; k < KP; ++k) zz[k] = k < K ? z[o + (size_t)k * hw] : -INFINITY;
      softmax_argmax<KP>(zz, K, pr);
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        g[k] = B[k] + (k == px.t ? A[k] : 0.f);
        dot = fmaf(pr[k], g[k], dot);
      }
      const float cs = ceScale * px.cw;
#pragma unroll
      for (int k = 0; k < KP; ++k) g[k] = fmaf(cs, pr[k] - (k == px.t ? 1.f : 0.f), pr[k] * (g[k] - dot));
    }
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < K) dl[o + (size_t)k * hw] = g[k];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the head's backward
// ---------------------------------------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void headk_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ a,
                                                        const float* __restrict__ w, size_t P, size_t hw, int C, int K,
                                                        float* __restrict__ dA, float* __restrict__ partial) {
  extern __shared__ f4 mcSmem[];
  float* sw = reinterpret_cast<float*>(mcSmem);   // K * C weights (a multiple of four floats)
  f4* red = mcSmem + (K * C) / 4;                 // 256 float4
  float* redf = reinterpret_cast<float*>(red);
  const int tid = threadIdx.x;
  const int c4 = C >> 2, cols = c4 < 256 ? c4 : 256, rows = 256 / cols;
  const int r = tid / cols, c = tid - r * cols;
  const size_t per = (P + gridDim.x - 1) / gridDim.x;
  const size_t p0 = (size_t)blockIdx.x * per;
  const size_t p1 = p0 + per < P ? p0 + per : P;
  for (int i = tid; i < K * C; i += 256) sw[i] = w[i];
  __syncthreads();
  const int O = K * (C + 1);
  float* out = partial + (size_t)blockIdx.x * O;
  for (int colBase = 0; colBase < c4; colBase += 256) {
    const bool active = r < rows && colBase + c < c4;
    const int ch = (colBase + c) * 4;
    f4 acc[KP];
    float accb[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      acc[k] = (f4){0.f, 0.f, 0.f, 0.f};
      accb[k] = 0.f;
    }
    if (active) {
      f4 wv[KP];
#pragma unroll
      for (int k = 0; k < KP; ++k) wv[k] = k < K ? ld4(sw + k * C + ch) : (f4){0.f, 0.f, 0.f, 0.f};
      for (size_t p = p0 + r; p < p1; p += rows) {
        const size_t img = p / hw, pix = p - img * hw;
        const float* d = dl + img * K * hw + pix;
        const f4 av = ld4(a + p * (size_t)C + ch);
        f4 da = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KP; ++k)
          if (k < K) {
            const float dk = d[(size_t)k * hw];
            acc[k] += av * dk;
            accb[k] += dk;
            da += wv[k] * dk;
          }
        if (dA) *reinterpret_cast<f4*>(dA + p * (size_t)C + ch) = da;
      }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (k >= K) continue;   // uniform
      red[tid] = active ? acc[k] : (f4){0.f, 0.f, 0.f, 0.f};
      __syncthreads();
      if (r == 0 && colBase + c < c4) {
        f4 t = red[c];
        for (int rr = 1; rr < rows; ++rr) t += red[rr * cols + c];
        float* o = out + k * (C + 1) + ch;
        o[0] = t[0], o[1] = t[1], o[2] = t[2], o[3] = t[3];
      }
      __syncthreads();
      if (colBase == 0) {   // db: column 0's threads have seen every pixel of the block once
        redf[tid] = (active && c == 0) ? accb[k] : 0.f;
        __syncthreads();
        if (tid == 0) {
          float t = redf[0];
          for (int rr = 1; rr < rows; ++rr) t += redf[rr * cols];
          out[k * (C + 1) + C] = t;
        }
        __syncthreads();
      }
    }
  }
}

// output o = k * (C + 1) + c (c == C: db[k]) = the blocks' partials added in double: 16 parts, in order
__global__ __launch_bounds__(256) void headk_bwd_finalize_kernel(const float* __restrict__ partial, int nb, int C, int K,
                                                                 float* __restrict__ dW, float* __restrict__ db) {
  __shared__ double fin[16][16];
  const int O = K * (C + 1);
  const int i = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int o = blockIdx.x * 16 + i;
  double s = 0.0;
  if (o < O)
    for (int b = part; b < nb; b += 16) s += (double)partial[(size_t)b * O + o];
  fin[part][i] = s;
  __syncthreads();
  if (part == 0 && o < O) {
    double t = fin[0][i];
    for (int q = 1; q < 16; ++q) t += fin[q][i];
    const int k = o / (C + 1), c = o - k * (C + 1);
    if (c < C)
      dW[k * C + c] = (float)t;
    else
      db[k] = (float)t;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the confusion matrix
// ---------------------------------------------------------------------------------------------------------------------
constexpr int CONF_CELLS = MC_MAX_CLASSES * MC_MAX_CLASSES;

inline int confusion_blocks(size_t numel) {
  const size_t b = (numel + 2047) / 2048;
  return (int)(b < 1 ? 1 : (b > (size_t)MC_RED_BLOCKS ? (size_t)MC_RED_BLOCKS : b));
}

__global__ __launch_bounds__(256) void confusion_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth,
                                                        size_t numel, int K, int ignore, unsigned* __restrict__ work) {
  __shared__ unsigned cnt[4][CONF_CELLS];
  const int tid = threadIdx.x, wave = tid >> 6;
  cnt[wave][tid & 63] = 0u;
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + tid; i < numel; i += stride) {
    const int t = truth[i], p = pred[i];
    if (t < K && t != ignore && p < K) atomicAdd(&cnt[wave][t * K + p], 1u);   // LDS
  }
  __syncthreads();
  if (tid < CONF_CELLS) work[(size_t)blockIdx.x * CONF_CELLS + tid] = ((cnt[0][tid] + cnt[1][tid]) + cnt[2][tid]) + cnt[3][tid];
}

__global__ __launch_bounds__(64) void confusion_finalize_kernel(const unsigned* __restrict__ work, int nb, int K,
                                                                u64* __restrict__ acc) {
  const int q = threadIdx.x;
  if (q >= K * K) return;
  u64 s = 0ull;
  for (int b = 0; b < nb; ++b) s += (u64)work[(size_t)b * CONF_CELLS + q];
  acc[q] += s;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------------
bool class_loss_params_valid(const ClassLossParams& p, int K) {
  if (K < 2 || K > MC_MAX_CLASSES) return false;
  if (!(p.ceW >= 0.f) || !(p.diceW >= 0.f) || !std::isfinite(p.ceW) || !std::isfinite(p.diceW)) return false;
  if (p.ceW == 0.f && p.diceW == 0.f) return false;
  if (!(p.smooth > 0.f) || !std::isfinite(p.smooth)) return false;
  for (int k = 0; k < K; ++k)
    if (!(p.cw[k] >= 0.f) || !std::isfinite(p.cw[k])) return false;
  return p.ignore >= -1 && p.ignore <= 255;
}

static bool headk_shape_ok(int n, size_t hw, int C, int K) {
  return n > 0 && hw > 0 && C > 0 && C % 4 == 0 && K >= 2 && K <= MC_MAX_CLASSES && (size_t)K * C <= (size_t)MC_MAX_WEIGHTS;
}

hipError_t launch_headk(const float* x, const float* w, const float* b, int n, size_t hw, int C, int K, float* logits,
                        float* probs, uint8_t* labels, int maskClass, uint8_t* mask, hipStream_t s) {
  if (!headk_shape_ok(n, hw, C, K)) return hipErrorInvalidValue;
  HeadKArgs a;
  a.x = x, a.hi = nullptr, a.lo2 = 0, a.w = w, a.b = b, a.npix = (size_t)n * hw, a.hw = hw, a.C = C, a.K = K;
  a.maskClass = maskClass, a.logits = logits, a.probs = probs, a.labels = labels, a.mask = mask;
  return launch_headk_any<false>(a, s);
}

hipError_t launch_headk_planes(const uint16_t* x, size_t xLo, const float* w, const float* b, int n, size_t hw, int C, int K,
                               float* logits, float* probs, uint8_t* labels, int maskClass, uint8_t* mask, hipStream_t s) {
  if (!headk_shape_ok(n, hw, C, K) || C % 8 || xLo % 8) return hipErrorInvalidValue;
  HeadKArgs a;
  a.x = nullptr, a.hi = reinterpret_cast<const uint32_t*>(x), a.lo2 = xLo / 2, a.w = w, a.b = b, a.npix = (size_t)n * hw;
  a.hw = hw, a.C = C, a.K = K, a.maskClass = maskClass, a.logits = logits, a.probs = probs, a.labels = labels, a.mask = mask;
  return launch_headk_any<true>(a, s);
}

hipError_t launch_class_labels(const float* logits, int n, size_t hw, int K, uint8_t* labels, int maskClass, uint8_t* mask,
                               hipStream_t s) {
  if (n <= 0 || hw == 0 || K < 1 || K > MC_MAX_CLASSES) return hipErrorInvalidValue;
  const size_t P = (size_t)n * hw;
  hipLaunchKernelGGL(class_labels_kernel, dim3(mc_grid(P, 256)), dim3(256), 0, s, logits, P, hw, K, labels, maskClass, mask);
  return hipGetLastError();
}

size_t class_loss_work_bytes() { return (size_t)MC_RED_BLOCKS * LOSS_NQ * sizeof(double) + COEF_FLOATS * sizeof(float); }

hipError_t launch_class_loss_grad(const float* logits, const uint8_t* labels, int n, size_t hw, int K,
                                  const ClassLossParams& prm, void* work, float* lossDev, float* dlogits, hipStream_t s) {
  if (n <= 0 || hw == 0 || K < 2 || K > MC_MAX_CLASSES) return hipErrorInvalidValue;
  const size_t P = (size_t)n * hw;
  const int nb = mc_red_blocks(P);
  double* partial = reinterpret_cast<double*>(work);
  float* coef = reinterpret_cast<float*>(partial + (size_t)MC_RED_BLOCKS * LOSS_NQ);
#define MC_BY_K(KERNEL, GRID, ...)                                                            \
  do {                                                                                        \
    if (K <= 2)                                                                               \
      hipLaunchKernelGGL((KERNEL<2>), dim3(GRID), dim3(256), 0, s, __VA_ARGS__);              \
    else if (K <= 4)                                                                          \
      hipLaunchKernelGGL((KERNEL<4>), dim3(GRID), dim3(256), 0, s, __VA_ARGS__);              \
    else                                                                                      \
      hipLaunchKernelGGL((KERNEL<8>), dim3(GRID), dim3(256), 0, s, __VA_ARGS__);              \
  } while (0)
  MC_BY_K(class_loss_partial_kernel, nb, logits, labels, P, hw, K, prm, partial);
  hipLaunchKernelGGL(class_loss_finalize_kernel, dim3(1), dim3(256), 0, s, partial, nb, K, prm, lossDev, coef);
  if (dlogits) MC_BY_K(class_loss_grad_kernel, mc_grid(P, 256), logits, labels, P, hw, K, prm, coef, dlogits);
  return hipGetLastError();
}

size_t headk_backward_partial_floats(size_t P, int C, int K) { return (size_t)mc_red_blocks(P) * K * (C + 1); }

hipError_t launch_headk_backward(const float* dl, const float* a, const float* w, int n, size_t hw, int C, int K, float* dA,
                                 float* partial, float* dW, float* db, hipStream_t s) {
  if (!headk_shape_ok(n, hw, C, K)) return hipErrorInvalidValue;
  const size_t P = (size_t)n * hw;
  const int nb = mc_red_blocks(P);
  const size_t lds = (size_t)K * C * sizeof(float) + 256 * sizeof(f4);
  if (K <= 2)
    hipLaunchKernelGGL((headk_bwd_kernel<2>), dim3(nb), dim3(256), lds, s, dl, a, w, P, hw, C, K, dA, partial);
  else if (K <= 4)
    hipLaunchKernelGGL((headk_bwd_kernel<4>), dim3(nb), dim3(256), lds, s, dl, a, w, P, hw, C, K, dA, partial);
  else
    hipLaunchKernelGGL((headk_bwd_kernel<8>), dim3(nb), dim3(256), lds, s, dl, a, w, P, hw, C, K, dA, partial);
  const int O = K * (C + 1);
  hipLaunchKernelGGL(headk_bwd_finalize_kernel, dim3((O + 15) / 16), dim3(256), 0, s, partial, nb, C, K, dW, db);
  return hipGetLastError();
}

size_t confusion_work_bytes() { return (size_t)MC_RED_BLOCKS * CONF_CELLS * sizeof(unsigned); }

hipError_t launch_confusion(const uint8_t* pred, const uint8_t* truth, size_t numel, int K, int ignore, void* work,
                            unsigned long long* acc, hipStream_t s) {
  if (K < 1 || K > MC_MAX_CLASSES || numel == 0) return hipErrorInvalidValue;
  const int nb = confusion_blocks(numel);
  unsigned* w = reinterpret_cast<unsigned*>(work);
  hipLaunchKernelGGL(confusion_kernel, dim3(nb), dim3(256), 0, s, pred, truth, numel, K, ignore, w);
  hipLaunchKernelGGL(confusion_finalize_kernel, dim3(1), dim3(64), 0, s, w, nb, K, acc);
  return hipGetLastError();
}

}  // namespace unet

// ---------------------------------------------------------------------------------------------------------------------
// operator entry points (tests): host weights are uploaded, scratch is the call's own, the stream is synchronised
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct Scratch {   // device memory of one call
  void* p[4] = {nullptr, nullptr, nullptr, nullptr};
  int used = 0;
  ~Scratch() {
    for (int i = 0; i < used; ++i) hipFree(p[i]);
  }
  template <class T>
  hipError_t get(T** out, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes < 64 ? 64 : bytes);
    if (e == hipSuccess) p[used++] = q;
    *out = reinterpret_cast<T*>(q);
    return e;
  }
};

unet::ClassLossParams params_of(const unet_class_loss_config& c) {
  unet::ClassLossParams p;
  p.ceW = c.ce_weight, p.diceW = c.dice_weight, p.smooth = c.smooth, p.ignore = c.ignore_index;
  for (int k = 0; k < unet::MC_MAX_CLASSES; ++k) p.cw[k] = c.class_weight[k];
  return p;
}

const char* headk_refusal(int n, int h, int w, int c, int k) {
  if (n <= 0 || h <= 0 || w <= 0) return "n, h and w must be positive";
  if (k < 2 || k > UNET_MAX_CLASSES) return "the class count must be 2..UNET_MAX_CLASSES";
  if (c <= 0 || c % 4) return "the channel count must be a positive multiple of 4";
  if ((long long)k * c > unet::MC_MAX_WEIGHTS) return "classes * channels must not exceed 4096";
  return nullptr;
}

// the calling thread's synchronisation behind an operator's launches
hipError_t finish(hipError_t e, void* stream) {
  const hipError_t es = hipStreamSynchronize((hipStream_t)stream);
  return e == hipSuccess ? es : e;
}

}  // namespace

extern "C" {

int unet_op_headk(int device, const float* x, int n, int h, int w, int c, int k, const float* w_host, const float* b_host,
                  float* logits, float* probs, uint8_t* labels, int mask_class, uint8_t* mask, void* stream) {
  const unet::OpCall op{"unet_op_headk"};
  if (!x || !w_host || !b_host) return op.refuse("x, the weights and the bias must not be null");
  if (const char* why = headk_refusal(n, h, w, c, k)) return op.refuse(why);
  if (unet::misaligned(x, 16)) return op.refuse("x must be 16-byte aligned");
  if (unet::misaligned(logits, 4) || unet::misaligned(probs, 4)) return op.refuse("logits and probs must be 4-byte aligned");
  if (mask && (mask_class < 0 || mask_class >= k)) return op.refuse("mask_class must name a class");
  if (int rc = op.on(device)) return rc;
  Scratch sc;
  float *wd = nullptr, *bd = nullptr;
  hipError_t e = sc.get(&wd, (size_t)k * c * sizeof(float));
  if (e == hipSuccess) e = sc.get(&bd, k * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(wd, w_host, (size_t)k * c * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(bd, b_host, k * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = unet::launch_headk(x, wd, bd, n, (size_t)h * w, c, k, logits, probs, labels, mask_class, mask, (hipStream_t)stream);
  return op.done(finish(e, stream));
}

size_t unet_class_loss_work_bytes(void) { return unet::class_loss_work_bytes(); }

int unet_class_labels_f32(int device, const float* logits, int n, int k, size_t pixels_per_image, uint8_t* labels,
                          int mask_class, uint8_t* mask, void* stream) {
  const unet::OpCall op{"unet_class_labels_f32"};
  if (!logits || (!labels && !mask)) return op.refuse("logits and one of labels, mask must not be null");
  if (n <= 0 || pixels_per_image == 0) return op.refuse("n and pixels_per_image must be positive");
  if (k < 1 || k > UNET_MAX_CLASSES) return op.refuse("the class count must be 1..UNET_MAX_CLASSES");
  if (mask && (mask_class < 0 || mask_class >= k)) return op.refuse("mask_class must name a class");
  if (unet::misaligned(logits, 4)) return op.refuse("logits must be 4-byte aligned");
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_class_labels(logits, n, pixels_per_image, k, labels, mask_class, mask, (hipStream_t)stream));
}

int unet_class_loss_grad(int device, const float* logits, const uint8_t* labels, int n, int k, size_t pixels_per_image,
                         const unet_class_loss_config* cfg, float* loss_dev, float* dlogits, void* work, void* stream) {
  const unet::OpCall op{"unet_class_loss_grad"};
  if (!logits || !labels || !cfg || !loss_dev || !work)
    return op.refuse("logits, labels, the configuration, loss_dev and work_dev must not be null");
  if (unet::misaligned(work, 8)) return op.refuse("work_dev must be 8-byte aligned");
  if (n <= 0 || pixels_per_image == 0) return op.refuse("n and pixels_per_image must be positive");
  if (k < 2 || k > UNET_MAX_CLASSES) return op.refuse("the class count must be 2..UNET_MAX_CLASSES");
  if (!unet::class_loss_params_valid(params_of(*cfg), k)) return op.refuse("the loss configuration is outside its domain");
  if (unet::misaligned(logits, 4) || unet::misaligned(loss_dev, 4) || unet::misaligned(dlogits, 4))
    return op.refuse("logits, loss_dev and dlogits must be 4-byte aligned");
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_class_loss_grad(logits, labels, n, pixels_per_image, k, params_of(*cfg), work, loss_dev, dlogits,
                                              (hipStream_t)stream));
}

int unet_op_headk_x3_planes(int device, const uint16_t* x, size_t x_lo, int n, int h, int w, int c, int k, const float* w_host,
                            const float* b_host, float* logits, float* probs, uint8_t* labels, int mask_class, uint8_t* mask,
                            void* stream) {
  const unet::OpCall op{"unet_op_headk_x3_planes"};
  if (!x || !w_host || !b_host) return op.refuse("x, the weights and the bias must not be null");
  if (const char* why = headk_refusal(n, h, w, c, k)) return op.refuse(why);
  if (c % 8) return op.refuse("the channel count must be a multiple of 8");
  if (unet::misaligned(x, 16) || x_lo % 8 || x_lo < (size_t)n * h * w * c)
    return op.refuse("x must be 16-byte aligned and the lo plane a multiple of 8 halfs, at least the hi plane's length, behind it");
  if (unet::misaligned(logits, 4) || unet::misaligned(probs, 4)) return op.refuse("logits and probs must be 4-byte aligned");
  if (mask && (mask_class < 0 || mask_class >= k)) return op.refuse("mask_class must name a class");
  if (int rc = op.on(device)) return rc;
  Scratch sc;
  float *wd = nullptr, *bd = nullptr;
  hipError_t e = sc.get(&wd, (size_t)k * c * sizeof(float));
  if (e == hipSuccess) e = sc.get(&bd, k * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(wd, w_host, (size_t)k * c * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(bd, b_host, k * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = unet::launch_headk_planes(x, x_lo, wd, bd, n, (size_t)h * w, c, k, logits, probs, labels, mask_class, mask,
                                  (hipStream_t)stream);
  return op.done(finish(e, stream));
}

int unet_op_headk_backward(int device, const float* dlogits, const float* a, const float* w_host, int n, int h, int w, int c,
                           int k, float* d_a, float* d_w, float* d_b, void* stream) {
  const unet::OpCall op{"unet_op_headk_backward"};
  if (!dlogits || !a || !w_host || !d_w || !d_b) return op.refuse("dlogits, a, the weights, d_w and d_b must not be null");
  if (const char* why = headk_refusal(n, h, w, c, k)) return op.refuse(why);
  if (unet::misaligned(a, 16) || unet::misaligned(d_a, 16)) return op.refuse("a and d_a must be 16-byte aligned");
  if (unet::misaligned(dlogits, 4) || unet::misaligned(d_w, 4) || unet::misaligned(d_b, 4))
    return op.refuse("dlogits, d_w and d_b must be 4-byte aligned");
  if (int rc = op.on(device)) return rc;
  Scratch sc;
  float *wd = nullptr, *partial = nullptr;
  const size_t P = (size_t)n * h * w;
  hipError_t e = sc.get(&wd, (size_t)k * c * sizeof(float));
  if (e == hipSuccess) e = sc.get(&partial, unet::headk_backward_partial_floats(P, c, k) * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(wd, w_host, (size_t)k * c * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = unet::launch_headk_backward(dlogits, a, wd, n, (size_t)h * w, c, k, d_a, partial, d_w, d_b, (hipStream_t)stream);
  return op.done(finish(e, stream));
}

size_t unet_confusion_work_bytes(void) { return unet::confusion_work_bytes(); }

int unet_confusion_accumulate(int device, const uint8_t* pred, const uint8_t* truth, size_t numel, int k, int ignore_index,
                              unsigned long long* acc_dev, void* work_dev, void* stream) {
  const unet::OpCall op{"unet_confusion_accumulate"};
  if (!pred || !truth || !acc_dev || !work_dev) return op.refuse("pred, truth, acc_dev and work_dev must not be null");
  if (numel == 0 || numel > ((size_t)1 << 40)) return op.refuse("numel must be 1..2^40");
  if (k < 1 || k > UNET_MAX_CLASSES) return op.refuse("the class count must be 1..UNET_MAX_CLASSES");
  if (ignore_index < -1 || ignore_index > 255) return op.refuse("ignore_index must be -1 or 0..255");
  if (unet::misaligned(acc_dev, 8) || unet::misaligned(work_dev, 4)) return op.refuse("acc_dev must be 8-byte, work_dev 4-byte aligned");
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_confusion(pred, truth, numel, k, ignore_index, work_dev, acc_dev, (hipStream_t)stream));
}

}  // extern "C"
