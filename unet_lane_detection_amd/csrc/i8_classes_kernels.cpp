// K-class head of the int8 tier (i8_classes_kernels.h).  A code object of its own: the int8 kernels of unet_hip.cpp do
// not change with it.
//
// headk_i8_kernel<KP>.  KP is K rounded up to 2, 4 or 8: the accumulators are registers.  A block first copies the K * C
// weight bytes to LDS (16 bytes per thread and step) and threads 0 .. K - 1 form their row's constants there once:
//   cst_k = bias_k - xzp sum w_k + C xzp wzp_k   (sum w_k by v_dot4 against 0x01010101, exact in int32)
// A lane then owns PPL = 4 consecutive pixels (a "group"; npix and hw are multiples of 4, so a group lies in one image
// and starts on a 16-byte boundary of every plane).  Per 16 channels it loads 16 bytes of each of its pixels, adds
// their byte sum, and for every class reads the row's 16 weight bytes from LDS - one address for the whole wave, a
// broadcast - for four v_dot4 per pixel: the weights are read once per group, not per pixel.  Per pixel and class
//   t = dot - wzp_k sum x + cst_k   (int32),   z = __fmul_rn(float(t), mult_k)
// which is head_i8_kernel's arithmetic row by row.  Stores: per class one 16-byte store of the group's four logits
// (and probabilities), one 4-byte store of its four labels and of its four mask bytes.  Softmax and argmax are
// softmax_argmax (with the sum and the quotient in double: the logits are exact, the probabilities follow them to
// expf's error) / class_argmax of multiclass_kernels.h; without `probs` no exponential is formed.  There is no barrier
// behind the prologue, so the grid-stride loop may end at different trips in different lanes.
//
// headk_h16_kernel<KP, IN16>.  The same layout for the head of a hybrid model: K rows of fp16 weights in LDS, eight
// channels per step (head_h16_kernel's), one fp32 FMA chain per pixel and class in ascending c, v = a m_k + b_k.
//
// Bounds.  g < npix / 4, so every pixel 4 g + j < npix; reads x[(4 g + j) ld + i], i < C <= ld; plane offsets
// (img K + k) hw + pix with img < n, k < K, pix + 3 < hw; LDS words below K C / 16 (K C / 8), which the launchers cap.
#include "i8_classes_kernels.h"

#include "multiclass_kernels.h"

namespace unet {

namespace {

typedef int v4i32 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

constexpr int PPL = 4;              // consecutive pixels of a lane
constexpr int HEADK_MAX_KC = 2048;  // K * C: 8 classes of 256 channels

// the four outputs of one group from its logits
template <int KP>
__device__ __forceinline__ void store_group(const HeadKI8Args& a, size_t p0, const float (&z)[PPL][KP]) {
  const int K = a.K;
  const size_t img = p0 / a.hw, pix = p0 - img * a.hw;
  const size_t o = img * K * a.hw + pix;
  if (a.logits) {
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < K) {
        const f4 v = {z[0][k], z[1][k], z[2][k], z[3][k]};
        *reinterpret_cast<f4*>(a.logits + o + (size_t)k * a.hw) = v;
      }
  }
  uint32_t lab = 0;
  if (a.probs) {
    float p[PPL][KP];
#pragma unroll
    for (int j = 0; j < PPL; ++j) lab |= (uint32_t)softmax_argmax<KP, double>(z[j], K, p[j]) << (8 * j);
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < K) {
        const f4 v = {p[0][k], p[1][k], p[2][k], p[3][k]};
        *reinterpret_cast<f4*>(a.probs + o + (size_t)k * a.hw) = v;
      }
  } else if (a.labels || a.mask) {
#pragma unroll
    for (int j = 0; j < PPL; ++j) lab |= (uint32_t)class_argmax<KP>(z[j], K) << (8 * j);
  }
  if (a.labels) *reinterpret_cast<uint32_t*>(a.labels + p0) = lab;
  if (a.mask) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < PPL; ++j) m |= (((lab >> (8 * j)) & 0xFFu) == (uint32_t)a.maskClass ? 255u : 0u) << (8 * j);
    *reinterpret_cast<uint32_t*>(a.mask + p0) = m;
  }
}

template <int KP>
__global__ __launch_bounds__(256) void headk_i8_kernel(const HeadKI8Args a) {
  extern __shared__ v4i32 hkSmem[];   // K * C weight bytes
  __shared__ int sCst[KP], sWzp[KP];
  __shared__ float sMult[KP];
  const int C = a.C, K = a.K, tid = threadIdx.x;
  for (int i = tid; i < K * C / 16; i += 256) hkSmem[i] = reinterpret_cast<const v4i32*>(a.w)[i];
  __syncthreads();
  if (tid < KP) {
    int cst = 0, wz = 0;
    float mu = 0.f;
    if (tid < K) {
      const int* row = reinterpret_cast<const int*>(hkSmem) + tid * (C / 4);
      int sw = 0;
      for (int i = 0; i < C / 4; ++i) sw = __builtin_amdgcn_sdot4(row[i], 0x01010101, sw, false);
      wz = a.wzp[tid];
      mu = a.mult[tid];
      cst = a.bias[tid] - a.xzp * sw + C * a.xzp * wz;
    }
    sCst[tid] = cst;
    sWzp[tid] = wz;
    sMult[tid] = mu;
  }
  __syncthreads();
  const size_t groups = a.npix / PPL, stride = (size_t)gridDim.x * 256;
  for (size_t g = (size_t)blockIdx.x * 256 + tid; g < groups; g += stride) {
    const size_t p0 = g * PPL;
    const int8_t* xp = static_cast<const int8_t*>(a.x) + p0 * a.ld;
    int dot[PPL][KP], sx[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      sx[j] = 0;
#pragma unroll
      for (int k = 0; k < KP; ++k) dot[j][k] = 0;
    }
    for (int i = 0; i < C; i += 16) {
      v4i32 xv[PPL];
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        xv[j] = *reinterpret_cast<const v4i32*>(xp + (size_t)j * a.ld + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) sx[j] = __builtin_amdgcn_sdot4(xv[j][e], 0x01010101, sx[j], false);
      }
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k < K) {
          const v4i32 wv = hkSmem[(k * C + i) / 16];
#pragma unroll
          for (int j = 0; j < PPL; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) dot[j][k] = __builtin_amdgcn_sdot4(xv[j][e], wv[e], dot[j][k], false);
        }
    }
    float z[PPL][KP];
#pragma unroll
    for (int j = 0; j < PPL; ++j)
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const int t = dot[j][k] - sWzp[k] * sx[j] + sCst[k];
        z[j][k] = k < K ? __fmul_rn((float)t, sMult[k]) : 0.f;
      }
    store_group<KP>(a, p0, z);
  }
}

template <int KP, bool IN16>
__global__ __launch_bounds__(256) void headk_h16_kernel(const HeadKI8Args a) {
  extern __shared__ v4i32 hkSmem[];   // K * C fp16 weights
  __shared__ float sM[KP], sB[KP];
  const int C = a.C, K = a.K, tid = threadIdx.x;
  for (int i = tid; i < K * C / 8; i += 256) hkSmem[i] = reinterpret_cast<const v4i32*>(a.wh)[i];
  if (tid < KP) {
    sM[tid] = tid < K ? a.hm[tid] : 0.f;
    sB[tid] = tid < K ? a.hb[tid] : 0.f;
  }
  __syncthreads();
  const h16x8* sw = reinterpret_cast<const h16x8*>(hkSmem);
  const size_t groups = a.npix / PPL, stride = (size_t)gridDim.x * 256;
  for (size_t g = (size_t)blockIdx.x * 256 + tid; g < groups; g += stride) {
    const size_t p0 = g * PPL;
    float acc[PPL][KP];
#pragma unroll
    for (int j = 0; j < PPL; ++j)
#pragma unroll
      for (int k = 0; k < KP; ++k) acc[j][k] = 0.f;
    for (int i = 0; i < C; i += 8) {
      float xv[PPL][8];
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        if (IN16) {
          const h16x8 q = *reinterpret_cast<const h16x8*>(static_cast<const uint16_t*>(a.x) + (p0 + j) * a.ld + i);
#pragma unroll
          for (int e = 0; e < 8; ++e) xv[j][e] = (float)q[e];
        } else {
          const uint2 raw = *reinterpret_cast<const uint2*>(static_cast<const int8_t*>(a.x) + (p0 + j) * a.ld + i);
#pragma unroll
          for (int e = 0; e < 8; ++e)
            xv[j][e] = (float)((int)(int8_t)(((e < 4 ? raw.x : raw.y) >> (8 * (e & 3))) & 0xFF) - a.xzp);
        }
      }
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k < K) {
          const h16x8 wv = sw[(k * C + i) / 8];
#pragma unroll
          for (int j = 0; j < PPL; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[j][k] = fmaf((float)wv[e], xv[j][e], acc[j][k]);
        }
    }
    float z[PPL][KP];
#pragma unroll
    for (int j = 0; j < PPL; ++j)
#pragma unroll
      for (int k = 0; k < KP; ++k) z[j][k] = k < K ? acc[j][k] * sM[k] + sB[k] : 0.f;
    store_group<KP>(a, p0, z);
  }
}

bool headk_args_ok(const HeadKI8Args& a, int chanStep) {
  if (!a.x || a.C <= 0 || a.C % chanStep || a.ld < a.C || a.ld % 16 || a.K < 1 || a.K > MC_MAX_CLASSES ||
      a.K * a.C > HEADK_MAX_KC)
    return false;
  if (a.npix == 0 || a.hw == 0 || a.hw % PPL || a.npix % a.hw) return false;
  if (!a.logits && !a.probs && !a.labels && !a.mask) return false;
  if (a.mask && (a.maskClass < 0 || a.maskClass >= a.K)) return false;
  if ((reinterpret_cast<uintptr_t>(a.logits) | reinterpret_cast<uintptr_t>(a.probs) | reinterpret_cast<uintptr_t>(a.x)) % 16) return false;
  if ((reinterpret_cast<uintptr_t>(a.labels) | reinterpret_cast<uintptr_t>(a.mask)) % 4) return false;
  return true;
}

// eight blocks per CU, then the grid stride
unsigned headk_grid(size_t npix) {
  const size_t b = (npix / PPL + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

template <bool IN16>
void launch_h16(const HeadKI8Args& a, unsigned g, size_t lds, hipStream_t s) {
  if (a.K <= 2)
    hipLaunchKernelGGL((headk_h16_kernel<2, IN16>), dim3(g), dim3(256), lds, s, a);
  else if (a.K <= 4)
    hipLaunchKernelGGL((headk_h16_kernel<4, IN16>), dim3(g), dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL((headk_h16_kernel<8, IN16>), dim3(g), dim3(256), lds, s, a);
}

}  // namespace

hipError_t launch_headk_i8(const HeadKI8Args& a, hipStream_t s) {
  if (!headk_args_ok(a, 16) || !a.w || !a.wzp || !a.bias || !a.mult) return hipErrorInvalidValue;
  const unsigned g = headk_grid(a.npix);
  const size_t lds = (size_t)a.K * a.C;
  if (a.K <= 2)
    hipLaunchKernelGGL((headk_i8_kernel<2>), dim3(g), dim3(256), lds, s, a);
  else if (a.K <= 4)
    hipLaunchKernelGGL((headk_i8_kernel<4>), dim3(g), dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL((headk_i8_kernel<8>), dim3(g), dim3(256), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_headk_h16(const HeadKI8Args& a, bool in16, hipStream_t s) {
  if (!headk_args_ok(a, 8) || !a.wh || !a.hm || !a.hb) return hipErrorInvalidValue;
  const unsigned g = headk_grid(a.npix);
  const size_t lds = (size_t)a.K * a.C * 2;
  if (in16)
    launch_h16<true>(a, g, lds, s);
  else
    launch_h16<false>(a, g, lds, s);
  return hipGetLastError();
}

}  // namespace unet
