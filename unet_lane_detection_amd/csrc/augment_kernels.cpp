// The augmentation stage (augment_kernels.h): one launch per batch, plain C++, vector stores only.
//
// A block owns one 32 x 16 tile of one output sample.  32 pixels are 96 output bytes, so a tile row leaves as 24
// aligned dwords (plus at most 3 single bytes at either end where the row does not start on a dword), and two tile
// rows fill a 64-lane wave.  Blur size and enable bits come from the sample's record and are uniform in the block:
//   blur off  every thread gathers, interpolates and colours its pixels straight into the output tile in LDS;
//   blur on   the block stages tile + halo (1, 2 or 3 pixels; outside the image the reflect-101 pixel is recomputed)
//             as packed RGBX dwords - 38 x 22 at most, 3.3 KB -, runs the horizontal pass into 16-bit sums and the
//             vertical pass out of LDS, and rounds the 2-D sum once.
// Either way the tile is then written as whole dwords, and the sample's targets in the same launch.
//
// Every source coordinate passes through reflect101() and the source index is clamped, so no parameter table can make
// the kernel read outside the data set; the LDS extents depend on the blur radius only through r in {0,1,2,3}.
#include "augment_kernels.h"
#include "hsv8.h"

#include "op_entry.h"

// The model rounds every floating-point operation on its own (numpy has no fused multiply-add); so does this file.
#pragma clang fp contract(off)

namespace unet {

namespace {

constexpr int TW = 32, TH = 16, HALO = 3, SW = TW + 2 * HALO, SH = TH + 2 * HALO, THREADS = 256;
constexpr double COORD_LIMIT = 1073741824.0;   // 2^30 in 1/32 pixel

__device__ const int BLUR_TAPS[4][7] = {{1, 0, 0, 0, 0, 0, 0}, {1, 2, 1, 0, 0, 0, 0}, {1, 4, 6, 4, 1, 0, 0}, {2, 7, 14, 18, 14, 7, 2}};

// BORDER_REFLECT_101 for any p, n >= 2:  ... 2 1 | 0 1 2 ... n-1 | n-2 ...
__device__ __forceinline__ int reflect101(int p, int n) {
  const int period = 2 * (n - 1);
  int t = p % period;
  if (t < 0) t += period;
  return t < n ? t : period - t;
}

// output pixel -> source coordinate in 1/32 pixel
__device__ __forceinline__ void fixed_coords(const AugmentParams& P, int height, int width, int x, int y, int& X, int& Y) {
  const double cx = (double)(width - 1) * 0.5, cy = (double)(height - 1) * 0.5;
  const double dx = (double)x - cx, dy = (double)y - cy;
  double fx = ((P.m[0] * dx + P.m[1] * dy + P.m[2]) + cx) * 32.0;
  double fy = ((P.m[3] * dx + P.m[4] * dy + P.m[5]) + cy) * 32.0;
  fx = fmin(fmax(fx, -COORD_LIMIT), COORD_LIMIT);   // a NaN comes out as -COORD_LIMIT
  fy = fmin(fmax(fy, -COORD_LIMIT), COORD_LIMIT);
  X = (int)rint(fx);
  Y = (int)rint(fy);
}

__device__ __forceinline__ int lut_clip255(float v) { return (int)fminf(fmaxf(v, 0.f), 255.f); }

// RGB -> 8-bit HSV -> the three shifts -> RGB (augment.py: rgb_to_hsv, hue_lut, shift_lut, hsv_to_rgb)
__device__ __forceinline__ void hue_saturation_value(int (&c)[3], float dh, float ds, float dv) {
  int h, s, v;
  rgb_to_hsv8(c[0], c[1], c[2], h, s, v);
  float t = (float)h + dh;
  const float k = floorf(t / 180.f);
  t = t - k * 180.f;
  if (t >= 180.f) t = t - 180.f;
  if (t < 0.f) t = t + 180.f;
  h = min(max((int)t, 0), 179);
  s = lut_clip255((float)s + ds);
  v = lut_clip255((float)v + dv);
  const int sector = h / 30, fr = h - 30 * sector;
  const int p = (2 * v * (255 - s) + 255) / 510;
  const int q = (2 * v * (7650 - s * fr) + 7650) / 15300;
  const int u = (2 * v * (7650 - s * (30 - fr)) + 7650) / 15300;
  switch (sector) {
    case 0: c[0] = v, c[1] = u, c[2] = p; break;
    case 1: c[0] = q, c[1] = v, c[2] = p; break;
    case 2: c[0] = p, c[1] = v, c[2] = u; break;
    case 3: c[0] = p, c[1] = q, c[2] = v; break;
    case 4: c[0] = u, c[1] = p, c[2] = v; break;
    default: c[0] = v, c[1] = p, c[2] = q; break;
  }
}

// one output pixel before the blur: gather, bilinear interpolation, brightness / contrast, HSV; packed R | G<<8 | B<<16
__device__ __forceinline__ uint32_t augment_pixel(const uint8_t* __restrict__ img, int height, int width,
                                                  const AugmentParams& P, int x, int y) {
  int X, Y;
  fixed_coords(P, height, width, x, y, X, Y);
  const int sx = X >> 5, sy = Y >> 5, fa = X & 31, fb = Y & 31;
  const int wgt[4] = {(32 - fb) * (32 - fa) * 32, (32 - fb) * fa * 32, fb * (32 - fa) * 32, fb * fa * 32};
  int c[3] = {0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (wgt[t] != 0) {   // integer coordinates (identity, flip, 90 degrees) read one tap
      const int yy = reflect101(sy + (t >> 1), height), xx = reflect101(sx + (t & 1), width);
      const uint8_t* p = img + ((size_t)yy * width + xx) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] += wgt[t] * (int)p[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = (c[k] + (1 << 14)) >> 15;
  if (P.flags & AUG_BC) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = (float)c[k] * P.alpha;
      v = v + P.beta255;
      c[k] = lut_clip255(v);
    }
  }
  if (P.flags & AUG_HSV) hue_saturation_value(c, P.dh, P.ds, P.dv);
  return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
}

// LABELS: `targets` is a uint8 (n, H, W) plane that receives the nearest-sampled mask byte itself (class labels) instead
// of the float (n, 1, H, W) plane of thresholded values; everything else is the same code
template <bool LABELS>
__global__ __launch_bounds__(THREADS) void augment_kernel(const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks,
                                                          int nSource, int height, int width,
                                                          const AugmentParams* __restrict__ params, int tilesX, int tilesY,
                                                          int maskThreshold, uint8_t* __restrict__ out,
                                                          void* __restrict__ targets) {
  __shared__ uint32_t stage[SH * SW];   // tile + halo before the blur
  __shared__ uint2 rows[SH * TW];       // horizontal sums: x = R | G << 16, y = B (each <= 255 * 64)
  __shared__ uint32_t tile[TH * TW];    // the finished tile
  const int tilesPer = tilesX * tilesY;
  const int n = (int)(blockIdx.x / (unsigned)tilesPer), tIdx = (int)(blockIdx.x - (unsigned)n * tilesPer);
  const int ty0 = (tIdx / tilesX) * TH, tx0 = (tIdx % tilesX) * TW;
  const int tw = min(TW, width - tx0), th = min(TH, height - ty0);
  const AugmentParams P = params[n];
  const int src = min(max(P.src, 0), nSource - 1);
  const int r = P.blur == 3 ? 1 : P.blur == 5 ? 2 : P.blur == 7 ? 3 : 0;
  const size_t plane = (size_t)height * width;
  const uint8_t* img = images + (size_t)src * plane * 3;
  const int tid = threadIdx.x;

  if (r == 0) {
    for (int i = tid; i < TW * TH; i += THREADS) {
      const int lx = i % TW, ly = i / TW;
      if (lx < tw && ly < th) tile[i] = augment_pixel(img, height, width, P, tx0 + lx, ty0 + ly);
    }
  } else {
    const int sw = tw + 2 * r, sh = th + 2 * r;   // <= SW, SH
    for (int i = tid; i < sw * sh; i += THREADS) {
      const int ly = i / sw, lx = i - ly * sw;
      stage[ly * SW + lx] = augment_pixel(img, height, width, P, reflect101(tx0 + lx - r, width), reflect101(ty0 + ly - r, height));
    }
    __syncthreads();
    const int* taps = BLUR_TAPS[r];
    for (int i = tid; i < sh * TW; i += THREADS) {
      const int lx = i % TW, ly = i / TW;
      if (lx < tw) {
        unsigned a0 = 0, a1 = 0, a2 = 0;
        for (int k = 0; k <= 2 * r; ++k) {
          const uint32_t px = stage[ly * SW + lx + k];
          const unsigned w = (unsigned)taps[k];
          a0 += w * (px & 255u), a1 += w * ((px >> 8) & 255u), a2 += w * ((px >> 16) & 255u);
        }
        rows[i] = make_uint2(a0 | (a1 << 16), a2);
      }
    }
    __syncthreads();
    const int shift = 4 * r;
    const unsigned half = 1u << (shift - 1);
    for (int i = tid; i < TW * TH; i += THREADS) {
      const int lx = i % TW, ly = i / TW;
      if (lx < tw && ly < th) {
        unsigned a0 = 0, a1 = 0, a2 = 0;
        for (int k = 0; k <= 2 * r; ++k) {
          const uint2 v = rows[(ly + k) * TW + lx];
          const unsigned w = (unsigned)taps[k];
          a0 += w * (v.x & 0xffffu), a1 += w * (v.x >> 16), a2 += w * v.y;
        }
        tile[i] = ((a0 + half) >> shift) | (((a1 + half) >> shift) << 8) | (((a2 + half) >> shift) << 16);
      }
    }
  }
  __syncthreads();

  // the tile's rows as dwords: 32 lanes per row; lanes 0..23 one aligned dword each, 24..26 the bytes in front of the
  // first aligned dword, 27..29 the bytes behind the last one
  for (int i = tid; i < TH * 32; i += THREADS) {
    const int ly = i >> 5, lane = i & 31;
    if (ly >= th) continue;
    uint8_t* rowp = out + (((size_t)n * height + (ty0 + ly)) * width + tx0) * 3;
    const uint32_t* trow = tile + ly * TW;
    const int len = tw * 3;
    const int head = min((int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(rowp) & 3u)) & 3u), len);
    const int ndw = (len - head) >> 2;
    auto byteAt = [&](int b) -> uint32_t {
      const int px = b / 3;
      return (trow[px] >> (8 * (b - 3 * px))) & 255u;
    };
    if (lane < ndw) {
      const int b = head + 4 * lane;
      *reinterpret_cast<uint32_t*>(rowp + b) = byteAt(b) | (byteAt(b + 1) << 8) | (byteAt(b + 2) << 16) | (byteAt(b + 3) << 24);
    } else if (lane >= 24 && lane < 27) {
      const int b = lane - 24;
      if (b < head) rowp[b] = (uint8_t)byteAt(b);
    } else if (lane >= 27 && lane < 30) {
      const int b = head + 4 * ndw + (lane - 27);
      if (b < len) rowp[b] = (uint8_t)byteAt(b);
    }
  }

  // targets: the mask at the nearest source pixel, thresholded
  if (masks != nullptr) {
    const uint8_t* msk = masks + (size_t)src * plane;
    for (int i = tid; i < TW * TH; i += THREADS) {
      const int lx = i % TW, ly = i / TW;
      if (lx < tw && ly < th) {
        int X, Y;
        fixed_coords(P, height, width, tx0 + lx, ty0 + ly, X, Y);
        const int xx = reflect101((X + 16) >> 5, width), yy = reflect101((Y + 16) >> 5, height);
        const size_t o = ((size_t)n * height + (ty0 + ly)) * width + tx0 + lx;
        const uint8_t m = msk[(size_t)yy * width + xx];
        if constexpr (LABELS)
          static_cast<uint8_t*>(targets)[o] = m;
        else
          static_cast<float*>(targets)[o] = (int)m > maskThreshold ? 1.f : 0.f;
      }
    }
  }
}

}  // namespace

hipError_t launch_augment(const uint8_t* images, const uint8_t* masks, int nSource, int height, int width,
                          const AugmentParams* params, int nOut, int maskThreshold, uint8_t* out, float* targets,
                          uint8_t* labels, hipStream_t s) {
  const int tilesX = (width + TW - 1) / TW, tilesY = (height + TH - 1) / TH;
  const unsigned long long blocks = (unsigned long long)tilesX * tilesY * (unsigned long long)nOut;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  if (labels)
    hipLaunchKernelGGL(augment_kernel<true>, dim3((unsigned)blocks), dim3(THREADS), 0, s, images, masks, nSource, height, width,
                       params, tilesX, tilesY, maskThreshold, out, (void*)labels);
  else
    hipLaunchKernelGGL(augment_kernel<false>, dim3((unsigned)blocks), dim3(THREADS), 0, s, images, masks, nSource, height, width,
                       params, tilesX, tilesY, maskThreshold, out, (void*)targets);
  return hipGetLastError();
}

}  // namespace unet

extern "C" {

size_t unet_augment_param_bytes(void) { return sizeof(unet::AugmentParams); }

int unet_augment_u8(int device, const uint8_t* imagesDev, const uint8_t* masksDev, int nSource, int height, int width,
                    const void* paramsDev, int nOut, int maskThreshold, uint8_t* imagesOutDev, float* targetsOutDev,
                    void* stream) {
  const unet::OpCall op{"unet_augment_u8"};
  if (!imagesDev || !paramsDev || !imagesOutDev || (masksDev == nullptr) != (targetsOutDev == nullptr) ||
      nOut <= 0 || nSource <= 0)
    return op.refuse("refused by the entry point's checks");
  if (height < unet::AUG_MIN_SIDE || width < unet::AUG_MIN_SIDE || height > unet::AUG_MAX_SIDE || width > unet::AUG_MAX_SIDE)
    return op.refuse("height and width must lie between AUG_MIN_SIDE and AUG_MAX_SIDE", UNET_ERR_SHAPE);
  if (int rc = op.on(device)) return rc;
  const hipError_t e = unet::launch_augment(imagesDev, masksDev, nSource, height, width,
                                            static_cast<const unet::AugmentParams*>(paramsDev), nOut, maskThreshold,
                                            imagesOutDev, targetsOutDev, nullptr, (hipStream_t)stream);
  const int rc = op.done(e);
  return e == hipErrorInvalidValue ? UNET_ERR_INVALID_ARG : rc;   // a grid the launch itself refuses
}

// the label mode: the warped mask's byte itself (a class label) to a uint8 (nOut, H, W) plane
int unet_augment_u8_labels(int device, const uint8_t* imagesDev, const uint8_t* labelsDev, int nSource, int height, int width,
                           const void* paramsDev, int nOut, uint8_t* imagesOutDev, uint8_t* labelsOutDev, void* stream) {
  const unet::OpCall op{"unet_augment_u8_labels"};
  if (!imagesDev || !labelsDev || !paramsDev || !imagesOutDev || !labelsOutDev || nOut <= 0 || nSource <= 0)
    return op.refuse("refused by the entry point's checks");
  if (height < unet::AUG_MIN_SIDE || width < unet::AUG_MIN_SIDE || height > unet::AUG_MAX_SIDE || width > unet::AUG_MAX_SIDE)
    return op.refuse("height and width must lie between AUG_MIN_SIDE and AUG_MAX_SIDE", UNET_ERR_SHAPE);
  if (int rc = op.on(device)) return rc;
  const hipError_t e = unet::launch_augment(imagesDev, labelsDev, nSource, height, width,
                                            static_cast<const unet::AugmentParams*>(paramsDev), nOut, 0, imagesOutDev, nullptr,
                                            labelsOutDev, (hipStream_t)stream);
  const int rc = op.done(e);
  return e == hipErrorInvalidValue ? UNET_ERR_INVALID_ARG : rc;   // a grid the launch itself refuses
}

}  // extern "C"
