// int8 tier, hybrid quantisation (unet_lane_detection_amd/quant.py, section "hybrid quantisation"): the units a model
// names run on v_mfma_f32_16x16x32_f16 with fp32 accumulation, between int8 and / or fp16 tensors.  For every output
// pixel p and channel co
//     a[p,co] = sum_k w16[k,co] x[p,k]        k over taps x input channels; x = q - zx from an int8 tensor (an integer of
//                                             magnitude <= 255, exact in fp16), the stored value from an fp16 tensor;
//                                             0 outside the image; every product is exact in fp32
//     v       = a m[co] + b[co]               m = g[co] x_scale (int8 input) or g[co] (fp16 input), ReLU where the unit has it
//     int8 output:  clamp(rint(v / y_scale) + zy, lo, 127)          fp16 output:  fp16(min(v, 65504)), nearest even
// One kernel family, templated on the tap count (9: 3x3 convolution; 1: GEMM over pixel rows = the first layer on its
// 64-byte im2col rows and the transposed convolutions with the scatter epilogue of conv_i8.h) and on the input and
// output type.
//
// Structure: a block of 256 threads computes 128 pixels (TAPS = 9: 8 rows x 16 columns of one image; TAPS = 1: 128
// consecutive pixels) x 64 output columns.  The channel loop is split into chunks of 64 input channels: a chunk's
// halo tile (10 x 18 pixels) is staged to LDS ALREADY AS fp16 - int8 is converted to q - zx on the way, the halo and
// the channels beyond the real ones are zeros - so the MFMA loop is the same for both input types and 26 KiB of LDS
// serve every channel count (at 256 channels a whole fp16 halo tile would need 92 KiB).  Wave w owns pixel fragments
// 2w, 2w + 1 and all four 16-column subtiles.  Weights are the MFMA's A operand, packed on the host in fragment order
// with conv_i8.h's channel permutation (row j of subtile cs = column 16 (j >> 2) + 4 cs + (j & 3)), so an accumulator
// lane (li, lq) ends up with the 16 consecutive columns 16 lq .. 16 lq + 15 of pixel li: one 16-byte (int8) or two
// 16-byte (fp16) stores.  Layers of <= 32 output columns use a 32-column tile of two subtiles instead (NCS = 2 below):
// half the MFMAs, 8 columns per lane.  Weight fragments are read from global memory (L2) by every wave; the kernel is
// the accuracy remedy of the int8 tier, not its fast path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace unet {

struct ConvH16Args {
  const void* in;         // NHWC int8 or fp16, pixel stride ldi elements
  const uint16_t* wt;     // fp16 bits, packed [coTile(64)][chunk(64)][tap][kstep(2)][cs(4)][lane(64)][8]
  const float* mult;      // [colsPad] m
  const float* bias;      // [colsPad] b
  void* out;              // NHWC int8 or fp16, pixel stride ldo elements
  int N, H, W, ldi, ldo, co_off;
  int cinStage;           // input channels to stage (real channels rounded up to 8, <= ldi); the rest are zeros
  int chunks;             // ceil(cinStage / 64)
  int cols;               // valid GEMM columns (plain: Cout; scatter: 4 * coutPad)
  int coutReal, coutPad;  // scatter: real / padded channels per (a,b) group
  int tilesX, tilesY, pixTiles, coTiles;
  int xzp, yzp, lo, relu, scatter;
  int narrow;             // cols <= 32, not scatter: packed with cs(2) in the 32-column permutation (conv_h16_kernel, NCS = 2)
  float yscale;
};

// in16 / out16: the input / output tensor is fp16.  hipErrorInvalidValue for a shape the 32-bit pixel indices cannot hold.
hipError_t launch_conv_h16(ConvH16Args a, int taps, bool in16, bool out16, hipStream_t s);
// MaxPool2d(2,2) on fp16 NHWC: x (N,H,W,ldi) channels [0,c) -> y (N,H/2,W/2,ldo); c % 8 == 0
hipError_t launch_maxpool2x2_h16(const uint16_t* x, int n, int h, int w, int c, int ldi, uint16_t* y, int ldo, hipStream_t s);
// 1x1 head of a hybrid model: logit = (sum_c w16[c] x[c]) m + b in fp32, x as above; then sigmoid / mask as head_i8_kernel
hipError_t launch_head_h16(const void* x, bool in16, int ldx, int c, size_t npix, const uint16_t* w16, int xzp, float m,
                           float b, float* logits, float* probs, uint8_t* mask, float thr, hipStream_t s);

#ifdef UNET_CONV_H16_KERNELS   // conv_h16.cpp: the kernels are a code object of their own

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float h16f32x4 __attribute__((ext_vector_type(4)));

constexpr int H16_PITCH = 144;   // LDS bytes per staged pixel: 64 fp16 + 16 (consecutive pixels 9 slots of 16 bytes apart)

// NCS: 16-row weight subtiles per step.  4: a tile of 64 columns, lane (li, lq) ends with columns 16 lq .. 16 lq + 15.
// 2 (layers of <= 32 columns, the whole 224 x 224 level of model B): a tile of 32 columns in the permutation
// row j of subtile cs = column 8 (j >> 2) + 4 cs + (j & 3), so that no MFMA multiplies padding and lane (li, lq) ends with
// the 8 columns 8 lq .. 8 lq + 7.
template <int TAPS, bool IN16, bool OUT16, int NCS>
__global__ __launch_bounds__(256) void conv_h16_kernel(const ConvH16Args a) {
  constexpr int TW = TAPS == 9 ? 18 : 16, TH = TAPS == 9 ? 10 : 8;
  constexpr int NPIX = TW * TH;
  constexpr int NV = NCS * 4;   // columns per lane
  __shared__ __align__(16) unsigned char smem[NPIX * H16_PITCH];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const int coTile = blockIdx.y;
  const long npix = (long)a.N * a.H * a.W;
  int n = 0, y0 = 0, x0 = 0;
  long p0 = 0;
  if (TAPS == 9) {
    const int t = blockIdx.x;
    const int tx = t % a.tilesX, r = t / a.tilesX;
    n = r / a.tilesY;
    y0 = (r - n * a.tilesY) * 8;
    x0 = tx * 16;
  } else {
    p0 = (long)blockIdx.x * 128;
  }
  h16f32x4 acc[2][NCS];
#pragma unroll
  for (int ms = 0; ms < 2; ++ms)
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) acc[ms][cs] = h16f32x4{0.f, 0.f, 0.f, 0.f};

  for (int chunk = 0; chunk < a.chunks; ++chunk) {
    if (chunk) __syncthreads();   // the previous chunk's reads are done
    const int left = a.cinStage - chunk * 64;
    const int nks = left > 32 ? 2 : 1;     // K = 32 steps of this chunk; only their 4 nks groups of 8 channels are staged
    const int gsh = nks + 1, ng = 4 * nks;
    for (int i = tid; i < NPIX * ng; i += 256) {
      const int pix = i >> gsh, g = i & (ng - 1);
      const int c = chunk * 64 + g * 8;
      bool ok = c < a.cinStage;
      long src;
      if (TAPS == 9) {
        const int py = pix / TW, px = pix - py * TW;
        const int y = y0 + py - 1, x = x0 + px - 1;
        ok = ok && y >= 0 && y < a.H && x >= 0 && x < a.W;
        src = ((long)n * a.H + y) * a.W + x;
      } else {
        src = p0 + pix;
        ok = ok && src < npix;
      }
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (ok) {
        if (IN16) {
          val = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(a.in) + (size_t)src * a.ldi + c);
        } else {
          const uint2 raw = *reinterpret_cast<const uint2*>(static_cast<const int8_t*>(a.in) + (size_t)src * a.ldi + c);
          h16x8 hv;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int q = (int)(int8_t)(((e < 4 ? raw.x : raw.y) >> (8 * (e & 3))) & 0xFF);
            hv[e] = (_Float16)(float)(q - a.xzp);
          }
          val = *reinterpret_cast<const uint4*>(&hv);
        }
      }
      *reinterpret_cast<uint4*>(smem + pix * H16_PITCH + g * 16) = val;
    }
    __syncthreads();
    const uint16_t* wc = a.wt + ((size_t)coTile * a.chunks + chunk) * (size_t)(TAPS * 2 * NCS * 64 * 8);
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      const int dy = tap / 3, dx = tap - dy * 3;
      for (int ks = 0; ks < nks; ++ks) {
        h16x8 bf[2];
#pragma unroll
        for (int ms = 0; ms < 2; ++ms) {
          const int f = wave * 2 + ms;
          const int pidx = TAPS == 9 ? (f + dy) * TW + li + dx : f * 16 + li;
          bf[ms] = *reinterpret_cast<const h16x8*>(smem + pidx * H16_PITCH + ks * 64 + lq * 16);
        }
#pragma unroll
        for (int cs = 0; cs < NCS; ++cs) {
          const h16x8 af = *reinterpret_cast<const h16x8*>(wc + (size_t)(((tap * 2 + ks) * NCS + cs) * 64 + lane) * 8);
#pragma unroll
          for (int ms = 0; ms < 2; ++ms) acc[ms][cs] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[ms], acc[ms][cs], 0, 0, 0);
        }
      }
    }
  }

  // epilogue: lane (li, lq) holds columns colB .. colB + NV - 1 of pixel li of fragments 2 wave, 2 wave + 1
  const int colB = coTile * 64 + lq * NV;
  if (colB >= a.cols) return;
  int chOff = a.co_off + colB, ab = 0;
  if (a.scatter) {
    ab = colB / a.coutPad;
    const int co = colB - ab * a.coutPad;
    if (ab >= 4 || co >= a.coutReal) return;
    chOff = a.co_off + co;
  }
  float mv[NV], bv[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    mv[e] = a.mult[colB + e];
    bv[e] = a.bias[colB + e];
  }
#pragma unroll
  for (int ms = 0; ms < 2; ++ms) {
    const int f = wave * 2 + ms;
    size_t opix;
    if (TAPS == 9) {
      const int y = y0 + f, x = x0 + li;
      if (y >= a.H || x >= a.W) continue;
      opix = ((size_t)n * a.H + y) * a.W + x;
    } else {
      const long p = p0 + f * 16 + li;
      if (p >= npix) continue;
      if (a.scatter) {
        const int x = (int)(p % a.W);
        const long row = p / a.W;   // n*H + y
        opix = (size_t)(2 * row + (ab >> 1)) * (size_t)(2 * a.W) + 2 * x + (ab & 1);
      } else {
        opix = (size_t)p;
      }
    }
    float v[NV];
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float t = acc[ms][cs][r] * mv[cs * 4 + r] + bv[cs * 4 + r];
        if (a.relu) t = fmaxf(t, 0.f);
        v[cs * 4 + r] = t;
      }
    if (OUT16) {   // 16-byte stores of 8 columns
      uint16_t* dst = static_cast<uint16_t*>(a.out) + opix * (size_t)a.ldo + chOff;
#pragma unroll
      for (int k = 0; k < NV / 8; ++k) {
        h16x8 hv;
#pragma unroll
        for (int e = 0; e < 8; ++e) hv[e] = (_Float16)fminf(v[8 * k + e], 65504.f);
        *reinterpret_cast<h16x8*>(dst + 8 * k) = hv;
      }
    } else {       // one store of NV bytes
      uint32_t pk[NCS];
#pragma unroll
      for (int cs = 0; cs < NCS; ++cs) {
        uint32_t w = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float q = rintf(__fdiv_rn(v[cs * 4 + r], a.yscale)) + (float)a.yzp;
          q = fminf(fmaxf(q, (float)a.lo), 127.f);
          w |= (uint32_t)((int)q & 0xFF) << (8 * r);
        }
        pk[cs] = w;
      }
      int8_t* dst = static_cast<int8_t*>(a.out) + opix * (size_t)a.ldo + chOff;
      if constexpr (NCS == 4)
        *reinterpret_cast<uint4*>(dst) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
      else
        *reinterpret_cast<uint2*>(dst) = make_uint2(pk[0], pk[1]);
    }
  }
}

__global__ __launch_bounds__(256) void maxpool2x2_h16_kernel(const uint16_t* __restrict__ x, int n, int h, int w, int c, int ldi,
                                                             uint16_t* __restrict__ y, int ldo) {
  const int cv = c / 8;
  const size_t total = (size_t)n * (h / 2) * (w / 2) * cv;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int v = (int)(i % cv);
    size_t p = i / cv;
    const int xo = (int)(p % (w / 2));
    p /= (w / 2);
    const int yo = (int)(p % (h / 2));
    const int nn = (int)(p / (h / 2));
    h16x8 m;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const h16x8 q = *reinterpret_cast<const h16x8*>(x + (((size_t)nn * h + 2 * yo + dy) * w + 2 * xo + dx) * (size_t)ldi + v * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = (dy == 0 && dx == 0) ? q[e] : (q[e] > m[e] ? q[e] : m[e]);
      }
    *reinterpret_cast<h16x8*>(y + (((size_t)nn * (h / 2) + yo) * (w / 2) + xo) * (size_t)ldo + v * 8) = m;
  }
}

// One thread per pixel, 8 channels per step; c % 8 == 0
template <bool IN16>
__global__ __launch_bounds__(256) void head_h16_kernel(const void* __restrict__ x, int ldx, int c, size_t npix,
                                                       const uint16_t* __restrict__ w16, int xzp, float m, float b,
                                                       float* __restrict__ logits, float* __restrict__ probs,
                                                       uint8_t* __restrict__ mask, float thr) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += stride) {
    float acc = 0.f;
    for (int i = 0; i < c; i += 8) {
      const h16x8 wv = *reinterpret_cast<const h16x8*>(w16 + i);
      float xv[8];
      if (IN16) {
        const h16x8 q = *reinterpret_cast<const h16x8*>(static_cast<const uint16_t*>(x) + p * ldx + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = (float)q[e];
      } else {
        const uint2 raw = *reinterpret_cast<const uint2*>(static_cast<const int8_t*>(x) + p * ldx + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = (float)((int)(int8_t)(((e < 4 ? raw.x : raw.y) >> (8 * (e & 3))) & 0xFF) - xzp);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = fmaf((float)wv[e], xv[e], acc);
    }
    const float z = acc * m + b;
    if (logits) logits[p] = z;
    if (probs) probs[p] = 1.f / (1.f + __expf(-z));
    if (mask) mask[p] = z > thr ? 255 : 0;
  }
}

#endif   // UNET_CONV_H16_KERNELS

}  // namespace unet
