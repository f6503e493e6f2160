// Helper kernels beside the convolution structures: the split-K finish, the device-side weight packers, the plane
// split / merge / pooling / head fallbacks of the f16x3 tier, the q-plane passes of the f16q8 tier and the bf16 pooling
// pass.  None of them is a template, so each is defined wherever this header is included: unet_hip.cpp includes it and
// no other translation unit may (the structure headers, which the launch units share with unet_hip.cpp, define
// templates only).
#pragma once
#include "conv_q8_r512.h"
#include "upconv_x3_ws.h"

namespace unet {

// Second half of a split-K convolution: y = act(scale * sum_ks partial[ks] + shift) written as hi / lo planes (pixel
// stride ldo halfs, channel offset co_off).  partial: [kSplit][P][C] fp32, dense.
__global__ __launch_bounds__(256) void x3_splitk_finish_kernel(const float* __restrict__ partial, int kSplit, size_t P,
                                                               int C, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, int relu,
                                                               uint32_t* __restrict__ outHi, size_t outLo2, int ldo,
                                                               int co_off, unsigned* err) {
  float amax = 0.f;
  const int c4 = C >> 2;
  const size_t total = P * c4;
  const size_t stride = (size_t)gridDim.x * 256;
  const size_t slab = P * (size_t)C;
  const float floorV = relu ? 0.f : -3.4e38f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const size_t p = i / c4;
    const int c = (int)(i - p * c4) * 4;
    // kSplit is a power of two >= 2: pairs of independent loads in flight, added in a fixed order
    const float* src = partial + p * C + c;
    f32x4 v = *reinterpret_cast<const f32x4*>(src) + *reinterpret_cast<const f32x4*>(src + slab);
    for (int k = 2; k < kSplit; k += 4) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(src + k * slab);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(src + (k + 1) * slab);
      f32x4 a2 = (f32x4){0.f, 0.f, 0.f, 0.f}, a3 = a2;
      if (k + 2 < kSplit) {
        a2 = *reinterpret_cast<const f32x4*>(src + (k + 2) * slab);
        a3 = *reinterpret_cast<const f32x4*>(src + (k + 3) * slab);
      }
      v += (a0 + a1) + (a2 + a3);
    }
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c), sh = *reinterpret_cast<const f32x4*>(shift + c);
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = fmaxf(fmaf(v[e], sc[e], sh[e]), floorV);
    uint32_t h0, l0, h1, l1;
    split_pk_f16(y[0], y[1], h0, l0, amax);
    split_pk_f16(y[2], y[3], h1, l1, amax);
    const size_t o = (p * (size_t)ldo + co_off + c) >> 1;
    *reinterpret_cast<uint2*>(outHi + o) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(outHi + outLo2 + o) = make_uint2(l0, l1);
  }
  x3_report_range(amax, err);
}

// Device-side repack of fp32 PyTorch-layout 3x3 weights into this kernel's hi/lo fragment order (training: after every
// optimizer step).  mode 0: forward, W(co, ci, t) = w[(co*cin + ci)*9 + t] with w (cout, cin, 3, 3); mode 1: input
// gradient, a convolution with the roles of the channels swapped and the taps flipped: its "cout" is the forward
// cin and W(n, k, t) = w[(k*coutD + n)*9 + (8 - t)] with w (cin = k range, coutD = n range, 3, 3).  No pre-scaling: an
// fp16 subnormal lo part costs a few bits of the 22, far inside the training tolerance.
__global__ __launch_bounds__(256) void pack_x3_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int cout,
                                                      int cin, int mode) {
  const int nCh = cin / 32;
  const size_t total = (size_t)(cout / 64) * nCh * 9 * 4 * 64;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int lane = (int)(i & 63);
    size_t r0 = i >> 6;
    const int cs = (int)(r0 & 3);
    r0 >>= 2;
    const int t = (int)(r0 % 9);
    r0 /= 9;
    const int kc = (int)(r0 % nCh);
    const int ct = (int)(r0 / nCh);
    const int j = lane & 15, lq = lane >> 4;
    const int co = 64 * ct + 16 * (j >> 2) + 4 * cs + (j & 3);
    const int tr = t / 3, kx = t - tr * 3;
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      float v[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int ci = kc * 32 + lq * 8 + e2 * 2 + e;
        v[e] = mode == 0 ? w[((size_t)co * cin + ci) * 9 + t] : w[((size_t)ci * cout + co) * 9 + (8 - t)];
      }
      split_pk_f16(v[0], v[1], hi[e2], lo[e2]);
    }
    uint16_t* base = out + ((((size_t)ct * nCh + kc) * 3 + tr) * (size_t)(2 * 3 * 4 * 64 * 8));
    *reinterpret_cast<uint4*>(base + (((size_t)0 * 3 + kx) * 4 + cs) * 64 * 8 + lane * 8) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *reinterpret_cast<uint4*>(base + (((size_t)1 * 3 + kx) * 4 + cs) * 64 * 8 + lane * 8) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
}

// The same packing, one block per (channel tile of 64, chunk of 32) with the tile's 18,432 weights brought through LDS:
// they are 64 runs of 1,152 contiguous bytes (mode 0: rows co, 32 ci x 9 taps each) or 32 runs of 2,304 bytes (mode 1,
// the input-gradient operator: rows are the forward co = this operator's ci, 64 forward ci x 9 taps each), where
// pack_x3_kernel gathers them 4 bytes at a time (0.4 ms per training step for the 34 packs; this one is bound by the
// 0.5 GB it moves).  Launch with (cout / 64) * (cin / 32) blocks of 256 threads and kPackX3LdsBytes of dynamic LDS.
constexpr int kPackX3LdsBytes = 64 * (288 + 4) * 4;   // 74,752 (mode 1: 32 x (576 + 4) x 4 = 74,240)
__device__ __forceinline__ void pack_x3_lds_tile(const float* __restrict__ w, uint16_t* __restrict__ out, int cout, int cin,
                                                 int mode, int tileIdx, float* tileW) {
  const int nCh = cin / 32;
  const int ct = tileIdx / nCh, kc = tileIdx - ct * nCh;
  const int tid = threadIdx.x;
  // rows x rowLen floats of the source, row pitch rowLen + 4 in LDS
  const int rows = mode == 0 ? 64 : 32, rowLen = mode == 0 ? 288 : 576, pitch = rowLen + 4;
  for (int i = tid; i < rows * (rowLen / 4); i += 256) {
    const int r = i / (rowLen / 4), q = i - r * (rowLen / 4);
    // mode 0: w[(co * cin + ci) * 9 + t], co = 64 ct + r, ci from 32 kc; mode 1: w[(ci * cout + co) * 9 + t] with this
    // operator's ci = 32 kc + r as the forward co (row) and its co from 64 ct as the forward ci
    const size_t src = mode == 0 ? ((size_t)(64 * ct + r) * cin + 32 * kc) * 9 : ((size_t)(32 * kc + r) * cout + 64 * ct) * 9;
    *reinterpret_cast<float4*>(tileW + r * pitch + 4 * q) = *reinterpret_cast<const float4*>(w + src + 4 * q);
  }
  __syncthreads();
  for (int i = tid; i < 9 * 4 * 64; i += 256) {
    const int lane = i & 63;
    const int cs = (i >> 6) & 3;
    const int t = i >> 8;
    const int j = lane & 15, lq = lane >> 4;
    const int col = 16 * (j >> 2) + 4 * cs + (j & 3);   // this operator's co within the tile
    const int tr = t / 3, kx = t - tr * 3;
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      float v[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int k = lq * 8 + e2 * 2 + e;   // this operator's ci within the chunk
        v[e] = mode == 0 ? tileW[col * pitch + k * 9 + t] : tileW[k * pitch + col * 9 + (8 - t)];
      }
      split_pk_f16(v[0], v[1], hi[e2], lo[e2]);
    }
    uint16_t* base = out + ((((size_t)ct * nCh + kc) * 3 + tr) * (size_t)(2 * 3 * 4 * 64 * 8));
    *reinterpret_cast<uint4*>(base + (((size_t)0 * 3 + kx) * 4 + cs) * 64 * 8 + lane * 8) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *reinterpret_cast<uint4*>(base + (((size_t)1 * 3 + kx) * 4 + cs) * 64 * 8 + lane * 8) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
}

__global__ __launch_bounds__(256) void pack_x3_lds_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int cout,
                                                          int cin, int mode) {
  extern __shared__ __attribute__((aligned(16))) float tileW[];
  pack_x3_lds_tile(w, out, cout, cin, mode, (int)blockIdx.x, tileW);
}

// All of a network's packs in one launch: block b belongs to the table entry e with start[e] <= b < start[e + 1] and
// is tile b - start[e] of it (the training step re-packs 34 operators after every optimizer step: as 34 launches they
// cost their launch gaps)
struct PackX3Desc {
  const float* w;
  uint16_t* out;
  int cout, cin, mode;
};
__global__ __launch_bounds__(256) void pack_x3_lds_multi_kernel(const PackX3Desc* __restrict__ descs,
                                                                const unsigned* __restrict__ start, int n) {
  extern __shared__ __attribute__((aligned(16))) float tileW[];
  int lo = 0, hi = n - 1;   // the entry whose block range holds blockIdx.x
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= blockIdx.x)
      lo = mid;
    else
      hi = mid - 1;
  }
  const PackX3Desc d = descs[lo];
  pack_x3_lds_tile(d.w, d.out, d.cout, d.cin, d.mode, (int)(blockIdx.x - start[lo]), tileW);
}

// ---- plane helpers (test entry points and the unfused fallbacks) ----

// fp32 NHWC (pixel stride ld, `c` channels used) -> hi/lo planes with the same geometry
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, size_t nvec2,
                                                           uint32_t* __restrict__ hi, uint32_t* __restrict__ lo,
                                                           unsigned* err = nullptr) {
  float amax = 0.f;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec2; i += stride) {
    const float2 v = reinterpret_cast<const float2*>(x)[i];
    uint32_t h, l;
    split_pk_f16(v.x, v.y, h, l, amax);
    hi[i] = h;
    lo[i] = l;
  }
  x3_report_range(amax, err);
}

// The same split for a tensor whose magnitudes sit far below the fp16 range (activation gradients: ~1e-7): every
// value is first multiplied by 2^k with k chosen from the tensor's max |x| (`absmaxKey`: its float bits, produced by
// the kernel that wrote x) so that the maximum lands in [2^13, 2^14); 2^-k goes to *invOut for the consumer's epilogue.
// Power-of-two scaling is exact.
__global__ __launch_bounds__(256) void split_planes_scaled_kernel(const float* __restrict__ x, size_t nvec2,
                                                                  uint32_t* __restrict__ hi, uint32_t* __restrict__ lo,
                                                                  const unsigned* __restrict__ absmaxKey,
                                                                  float* __restrict__ invOut) {
  const unsigned key = *absmaxKey;
  int k = 0;
  if ((key >> 23) != 0 && (key >> 23) < 255) k = 13 - ((int)(key >> 23) - 127);   // normal, finite maximum
  k = k > 100 ? 100 : (k < -100 ? -100 : k);
  const float up = ldexpf(1.f, k);
  if (blockIdx.x == 0 && threadIdx.x == 0) *invOut = ldexpf(1.f, -k);
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec2; i += stride) {
    const float2 v = reinterpret_cast<const float2*>(x)[i];
    uint32_t h, l;
    split_pk_f16(v.x * up, v.y * up, h, l);
    hi[i] = h;
    lo[i] = l;
  }
}

__global__ __launch_bounds__(256) void merge_planes_kernel(const uint32_t* __restrict__ hi,
                                                           const uint32_t* __restrict__ lo, size_t nvec2,
                                                           float* __restrict__ y) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec2; i += stride) {
    float a, b;
    merge_pk_f16(hi[i], lo[i], a, b);
    reinterpret_cast<float2*>(y)[i] = make_float2(a, b);
  }
}

// MaxPool2d(2,2) on planes (fallback when the producer could not fuse it): x (N,H,W,ldi) -> y (N,H/2,W/2,C)
__global__ __launch_bounds__(256) void maxpool2x2_planes_kernel(const uint32_t* __restrict__ hi, size_t inLo2, int n,
                                                                int h, int w, int c, int ldi,
                                                                uint32_t* __restrict__ out, size_t outLo2) {
  const int c2 = c / 2, ld2 = ldi / 2;
  const size_t total = (size_t)n * (h / 2) * (w / 2) * c2;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int cc = (int)(i % c2);
    size_t p = i / c2;
    const int xo = (int)(p % (w / 2));
    p /= (w / 2);
    const int yo = (int)(p % (h / 2));
    const int nn = (int)(p / (h / 2));
    float m0 = -3.4e38f, m1 = -3.4e38f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const size_t o = (((size_t)nn * h + 2 * yo + dy) * w + 2 * xo + dx) * ld2 + cc;
        float a, b;
        merge_pk_f16(hi[o], hi[o + inLo2], a, b);
        m0 = fmaxf(m0, a);
        m1 = fmaxf(m1, b);
      }
    uint32_t qh, ql;
    split_pk_f16(m0, m1, qh, ql);
    out[i] = qh;
    out[i + outLo2] = ql;
  }
}

// 1x1 head on planes (fallback when the last convolution could not fuse it): x (npix, C) planes -> logits
__global__ __launch_bounds__(256) void head1x1_planes_kernel(const uint32_t* __restrict__ hi, size_t inLo2,
                                                             const float* __restrict__ w, float bias, size_t npix,
                                                             int c, float* __restrict__ logits,
                                                             float* __restrict__ probs, uint8_t* __restrict__ mask,
                                                             float thr) {
  const size_t stride = (size_t)gridDim.x * 256;
  const int c2 = c / 2;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += stride) {
    float z = bias;
    for (int i = 0; i < c2; ++i) {
      float a, b;
      merge_pk_f16(hi[p * c2 + i], hi[p * c2 + i + inLo2], a, b);
      z = fmaf(a, w[2 * i], z);
      z = fmaf(b, w[2 * i + 1], z);
    }
    if (logits) logits[p] = z;
    if (probs) probs[p] = 1.f / (1.f + __expf(-z));
    if (mask) mask[p] = z > thr ? 255 : 0;
  }
}

// ConvTranspose2d weight (Cin, Cout, 2, 2) fp32 -> the kernel's operand layout
// [coTile(64)][chunk(32)][plane(2)][ab(4)][cs(4)][lane][8], un-prescaled (training: re-derived on the device after every
// optimizer step; the host packer of the inference tier pre-scales per output channel)
// Operand of the transposed convolution's INPUT gradient as a MODE 1 GEMM: K = 4 * cout rows k = ab * cout + co,
// N = cin columns n = ci, W_d[k][n] = w[ci][co][ab]; layout [tile(256 columns)][chunk(32 k)][plane][group(4)][cs][lane][8]
// with zeros for columns >= cin (cin = 128 fills half a tile).
__global__ __launch_bounds__(256) void pack_upconv_dgrad_x3_kernel(const float* __restrict__ w, uint16_t* __restrict__ out,
                                                                   int cin, int cout) {
  const int K = 4 * cout, nCh = K / 32;
  const int nT = (cin + 255) / 256;
  const size_t total = (size_t)nT * nCh * 16 * 64;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int lane = (int)(i & 63);
    size_t r0 = i >> 6;
    const int cs = (int)(r0 & 3);
    const int grp = (int)((r0 >> 2) & 3);
    r0 >>= 4;
    const int kc = (int)(r0 % nCh);
    const int ct = (int)(r0 / nCh);
    const int j = lane & 15, lq = lane >> 4;
    const int n = 256 * ct + 64 * grp + 16 * (j >> 2) + 4 * cs + (j & 3);   // = ci
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      float v[2] = {0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int k = kc * 32 + lq * 8 + e2 * 2 + e;
        const int ab = k / cout, co = k - ab * cout;
        if (n < cin) v[e] = w[((size_t)n * cout + co) * 4 + ab];
      }
      split_pk_f16(v[0], v[1], hi[e2], lo[e2]);
    }
    uint16_t* base = out + ((size_t)ct * nCh + kc) * (size_t)(2 * 16 * 64 * 8);
    *reinterpret_cast<uint4*>(base + ((size_t)0 * 16 + grp * 4 + cs) * 64 * 8 + lane * 8) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *reinterpret_cast<uint4*>(base + ((size_t)1 * 16 + grp * 4 + cs) * 64 * 8 + lane * 8) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
}

__global__ __launch_bounds__(256) void pack_upconv_x3_kernel(const float* __restrict__ w, uint16_t* __restrict__ out,
                                                             int cin, int cout) {
  const int nCh = cin / 32;
  const size_t total = (size_t)(cout / 64) * nCh * 16 * 64;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int lane = (int)(i & 63);
    size_t r0 = i >> 6;
    const int cs = (int)(r0 & 3);
    const int ab = (int)((r0 >> 2) & 3);
    r0 >>= 4;
    const int kc = (int)(r0 % nCh);
    const int ct = (int)(r0 / nCh);
    const int j = lane & 15, lq = lane >> 4;
    const int co = 64 * ct + 16 * (j >> 2) + 4 * cs + (j & 3);
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      const int ci = kc * 32 + lq * 8 + e2 * 2;
      split_pk_f16(w[((size_t)ci * cout + co) * 4 + ab], w[((size_t)(ci + 1) * cout + co) * 4 + ab], hi[e2], lo[e2]);
    }
    uint16_t* base = out + ((size_t)ct * nCh + kc) * (size_t)(2 * 16 * 64 * 8);
    *reinterpret_cast<uint4*>(base + ((size_t)0 * 16 + ab * 4 + cs) * 64 * 8 + lane * 8) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *reinterpret_cast<uint4*>(base + ((size_t)1 * 16 + ab * 4 + cs) * 64 * 8 + lane * 8) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
}

// ---- f16q8 tier: q plane from the two fp16 planes: one thread per (pixel, 16 channels) ----
__global__ __launch_bounds__(256) void planes_to_q8_kernel(const uint16_t* __restrict__ hi, size_t loOff, size_t nPix,
                                                           int C, int ld, uint8_t* __restrict__ q) {
  // hi / lo planes: pixel stride ld halfs, C channels used (C % 32 == 0); q: pixel stride ld * 2 bytes
  const size_t per = (size_t)(C / 16);
  const float hs = __builtin_ldexpf(1.f, kQ8HiShift), ls = __builtin_ldexpf(1.f, kQ8LoShift);
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < nPix * per; t += (size_t)gridDim.x * 256) {
    const size_t p = t / per;
    const int g = (int)(t - p * per);   // 16-channel group
    const uint16_t* src = hi + p * ld + g * 16;
    typedef _Float16 f16x8v __attribute__((ext_vector_type(8)));
    const f16x8v h0 = *reinterpret_cast<const f16x8v*>(src), h1 = *reinterpret_cast<const f16x8v*>(src + 8);
    const f16x8v l0 = *reinterpret_cast<const f16x8v*>(src + loOff), l1 = *reinterpret_cast<const f16x8v*>(src + loOff + 8);
    uint4 oh, ol;
    oh.x = q8_pack4((float)h0[0] * hs, (float)h0[1] * hs, (float)h0[2] * hs, (float)h0[3] * hs);
    oh.y = q8_pack4((float)h0[4] * hs, (float)h0[5] * hs, (float)h0[6] * hs, (float)h0[7] * hs);
    oh.z = q8_pack4((float)h1[0] * hs, (float)h1[1] * hs, (float)h1[2] * hs, (float)h1[3] * hs);
    oh.w = q8_pack4((float)h1[4] * hs, (float)h1[5] * hs, (float)h1[6] * hs, (float)h1[7] * hs);
    ol.x = q8_pack4((float)l0[0] * ls, (float)l0[1] * ls, (float)l0[2] * ls, (float)l0[3] * ls);
    ol.y = q8_pack4((float)l0[4] * ls, (float)l0[5] * ls, (float)l0[6] * ls, (float)l0[7] * ls);
    ol.z = q8_pack4((float)l1[0] * ls, (float)l1[1] * ls, (float)l1[2] * ls, (float)l1[3] * ls);
    ol.w = q8_pack4((float)l1[4] * ls, (float)l1[5] * ls, (float)l1[6] * ls, (float)l1[7] * ls);
    uint8_t* dst = q + p * (size_t)ld * 2 + (g >> 1) * 64 + (g & 1) * 16;
    *reinterpret_cast<uint4*>(dst) = oh;
    *reinterpret_cast<uint4*>(dst + 32) = ol;
  }
}

// MaxPool2d(2,2) on planes for the f16q8 tier: x (N,H,W,ldi: the first `c` channels) -> y (N,H/2,W/2,c), as
// maxpool2x2_planes_kernel (same values: the maximum of hi + lo, split again), and the q planes of either tensor while
// their bytes are in registers anyway: srcQ - the input's q plane is written over its lo plane, in place (its remaining
// consumer is a convolution of this tier; a thread owns a whole 32-channel block, whose 64 lo bytes are exactly the
// block's q bytes); dstQ - the output gets its q plane instead of its lo plane.  One thread per output pixel and block.
__global__ __launch_bounds__(256) void maxpool2x2_planes_q8_kernel(uint16_t* __restrict__ src, size_t srcLo, int n, int h,
                                                                   int w, int c, int ldi, uint16_t* __restrict__ dst,
                                                                   size_t dstLo, int srcQ, int dstQ) {
  const int nb = c / 32;
  const size_t total = (size_t)n * (h / 2) * (w / 2) * nb;
  const size_t stride = (size_t)gridDim.x * 256;
  const float hs = __builtin_ldexpf(1.f, kQ8HiShift), ls = __builtin_ldexpf(1.f, kQ8LoShift);
  auto q_block = [&](const uint32_t* ph, const uint32_t* pl, uint4* out) __attribute__((always_inline)) {
    // 16 packed pairs hi, 16 packed pairs lo -> [hi8 x 32][lo8 x 32]
    uint32_t qh[8], ql[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a0, a1, a2, a3, b0, b1, b2, b3;
      merge_pk_f16(ph[2 * e], 0u, a0, a1);
      merge_pk_f16(ph[2 * e + 1], 0u, a2, a3);
      merge_pk_f16(pl[2 * e], 0u, b0, b1);
      merge_pk_f16(pl[2 * e + 1], 0u, b2, b3);
      qh[e] = q8_pack4(a0 * hs, a1 * hs, a2 * hs, a3 * hs);
      ql[e] = q8_pack4(b0 * ls, b1 * ls, b2 * ls, b3 * ls);
    }
    out[0] = make_uint4(qh[0], qh[1], qh[2], qh[3]);
    out[1] = make_uint4(qh[4], qh[5], qh[6], qh[7]);
    out[2] = make_uint4(ql[0], ql[1], ql[2], ql[3]);
    out[3] = make_uint4(ql[4], ql[5], ql[6], ql[7]);
  };
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int b = (int)(i % nb);
    size_t p = i / nb;
    const int xo = (int)(p % (w / 2));
    p /= (w / 2);
    const int yo = (int)(p % (h / 2));
    const int nn = (int)(p / (h / 2));
    float m[32];
#pragma unroll
    for (int e = 0; e < 32; ++e) m[e] = -3.4e38f;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      uint16_t* sp = src + ((((size_t)nn * h + 2 * yo + (d >> 1)) * w + 2 * xo + (d & 1)) * (size_t)ldi + b * 32);
      uint32_t ph[16], pl[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint4 vh = reinterpret_cast<const uint4*>(sp)[q], vl = reinterpret_cast<const uint4*>(sp + srcLo)[q];
        ph[4 * q] = vh.x, ph[4 * q + 1] = vh.y, ph[4 * q + 2] = vh.z, ph[4 * q + 3] = vh.w;
        pl[4 * q] = vl.x, pl[4 * q + 1] = vl.y, pl[4 * q + 2] = vl.z, pl[4 * q + 3] = vl.w;
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float a, bb;
        merge_pk_f16(ph[e], pl[e], a, bb);
        m[2 * e] = fmaxf(m[2 * e], a);
        m[2 * e + 1] = fmaxf(m[2 * e + 1], bb);
      }
      if (srcQ) q_block(ph, pl, reinterpret_cast<uint4*>(sp + srcLo));
    }
    uint32_t oh[16], ol[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) split_pk_f16(m[2 * e], m[2 * e + 1], oh[e], ol[e]);
    uint16_t* dp = dst + ((((size_t)nn * (h / 2) + yo) * (w / 2) + xo) * (size_t)c + b * 32);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      reinterpret_cast<uint4*>(dp)[q] = make_uint4(oh[4 * q], oh[4 * q + 1], oh[4 * q + 2], oh[4 * q + 3]);
    if (dstQ) {
      q_block(oh, ol, reinterpret_cast<uint4*>(dp + dstLo));
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        reinterpret_cast<uint4*>(dp + dstLo)[q] = make_uint4(ol[4 * q], ol[4 * q + 1], ol[4 * q + 2], ol[4 * q + 3]);
    }
  }
}

// MaxPool2d(2,2) on bf16 NHWC (8 channels = 16 bytes per thread); max of bf16 values is exact.
__global__ __launch_bounds__(256) void maxpool2x2_bf16_kernel(const uint16_t* __restrict__ in,
                                                              uint16_t* __restrict__ out, int n, int h, int w, int c,
                                                              int ldi) {
  const int c8 = c >> 3;
  const int oh = h >> 1, ow = w >> 1;
  const size_t total = (size_t)n * oh * ow * c8;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int cv = (int)(i % c8);
    size_t t = i / c8;
    const int ox = (int)(t % ow);
    t /= ow;
    const int oy = (int)(t % oh);
    const size_t img = t / oh;
    const uint16_t* p = in + ((img * h + (size_t)oy * 2) * w + (size_t)ox * 2) * (size_t)ldi + cv * 8;
    bf16x8 v[4];
    v[0] = *reinterpret_cast<const bf16x8*>(p);
    v[1] = *reinterpret_cast<const bf16x8*>(p + ldi);
    v[2] = *reinterpret_cast<const bf16x8*>(p + (size_t)w * ldi);
    v[3] = *reinterpret_cast<const bf16x8*>(p + (size_t)w * ldi + ldi);
    bf16x8 m;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float best = -3.4e38f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float f = __builtin_bit_cast(float, (uint32_t)(uint16_t)v[k][e] << 16);
        best = f > best ? f : best;
      }
      m[e] = (short)(__builtin_bit_cast(uint32_t, best) >> 16);
    }
    *reinterpret_cast<bf16x8*>(out + i * 8) = m;
  }
}

}  // namespace unet
