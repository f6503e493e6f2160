// The video path's two batched kernels (video_kernels.h): plain C++, 16-byte loads and stores.
//
// Both treat the whole batch as one flat run of destination pixels and give a thread RUN = 16 consecutive ones: 48 bytes
// of a 3-channel image (three 16-byte accesses) and 16 bytes of a 1-channel one.  The thread divides its first pixel
// into (image, y, x) once and steps from there, so a run may cross rows and images.  The last, partial run of a batch is
// read and written byte by byte, and so is every run when a base pointer is not 16-byte aligned (the slow path).
//
// Resampling is cv::resize INTER_LINEAR as camera_stage.h states it (resize_coeff is restated here, the integers are
// the same): the column coefficients of a launch are computed once per block into LDS, the row coefficients when a
// thread's row changes.  Every source index is clamped to the source image by resize_coeff, and a pixel past the end
// of the batch is neither sampled nor stored, so no argument the entry points accept makes a kernel read or write
// outside its buffers.
#include "video_kernels.h"

#include "op_entry.h"

#include <cmath>
#include <cstring>


// The model rounds every floating-point operation on its own (numpy has no fused multiply-add); so does this file.
#pragma clang fp contract(off)

namespace unet {

namespace {

constexpr int THREADS = 256, RUN = 16, MAX_BLOCKS = 2048;

// cv::resize INTER_LINEAR, 8-bit: source index and the two 2^11 fixed-point coefficients of destination index d
__device__ __forceinline__ void resize_coeff(int d, double scale, int srcSize, int& s, int& c0, int& c1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int si = (int)floorf(f);
  f = f - (float)si;
  if (si < 0) {
    si = 0;
    f = 0.f;
  }
  if (si >= srcSize - 1) {
    si = srcSize - 1;
    f = 0.f;
  }
  s = si;
  c1 = (int)rintf(f * 2048.f);
  c0 = (int)rintf((1.f - f) * 2048.f);
}

struct Resample {
  double scale_x, scale_y;
  int src_h, src_w, dst_h, dst_w;
  int copy;   // equal sizes: cv::resize's early exit
};

struct ResizeArgs {
  const uint8_t* src;
  uint8_t* dst;
  unsigned long long pixels;   // n * dst_h * dst_w
  Resample g;
  int swap_rb, aligned;
};

struct OverlayArgs {
  const uint8_t* frames;
  const uint8_t* masks;
  uint8_t* out;
  uint8_t* mask_out;
  unsigned long long pixels;   // n * height * width
  Resample g;                  // the mask's way up: src = mask, dst = frame
  float alpha, beta, gamma;
  int aligned;
};

struct RowState {
  int r0, r1, b0, b1;   // byte offsets of the two source rows inside their image, vertical coefficients
};

template <int CN>
__device__ __forceinline__ RowState row_state(const Resample& g, int y) {
  int sy, b0, b1;
  resize_coeff(y, g.scale_y, g.src_h, sy, b0, b1);
  const int sy1 = sy + 1 < g.src_h ? sy + 1 : g.src_h - 1;
  return RowState{sy * g.src_w * CN, sy1 * g.src_w * CN, b0, b1};
}

// one word per column: x = source column, y = c0 | c1 << 16
__device__ __forceinline__ void build_columns(const Resample& g, uint2* cols) {
  for (int x = threadIdx.x; x < g.dst_w; x += THREADS) {
    int s, c0, c1;
    resize_coeff(x, g.scale_x, g.src_w, s, c0, c1);
    cols[x] = make_uint2((uint32_t)s, (uint32_t)c0 | ((uint32_t)c1 << 16));
  }
}

template <int CN>
__device__ __forceinline__ void sample(const uint8_t* __restrict__ img, const Resample& g, const uint2* cols,
                                       const RowState& r, int x, int (&v)[CN]) {
  const uint2 c = cols[x];
  const int s = (int)c.x, a0 = (int)(c.y & 0xffffu), a1 = (int)(c.y >> 16);
  const int sx = s * CN, sx1 = (s + 1 < g.src_w ? s + 1 : g.src_w - 1) * CN;
#pragma unroll
  for (int k = 0; k < CN; ++k) {
    const int d0 = (int)img[r.r0 + sx + k] * a0 + (int)img[r.r0 + sx1 + k] * a1;
    const int d1 = (int)img[r.r1 + sx + k] * a0 + (int)img[r.r1 + sx1 + k] * a1;
    v[k] = (((r.b0 * (d0 >> 4)) >> 16) + ((r.b1 * (d1 >> 4)) >> 16) + 2) >> 2;
  }
}

// a thread's place in the flat run of destination pixels, and the source image and rows that go with it
template <int CN>
struct Cursor {
  const uint8_t* src;
  RowState r;
  int y, x;

  __device__ __forceinline__ Cursor(const uint8_t* srcBase, const Resample& g, size_t p0) {
    const size_t plane = (size_t)g.dst_h * g.dst_w;
    const size_t img = p0 / plane;
    const int rem = (int)(p0 - img * plane);
    y = rem / g.dst_w;
    x = rem - y * g.dst_w;
    src = srcBase + img * ((size_t)g.src_h * g.src_w * CN);
    r = g.copy ? RowState{0, 0, 0, 0} : row_state<CN>(g, y);
  }
  __device__ __forceinline__ void step(const Resample& g) {
    if (++x == g.dst_w) {
      x = 0;
      if (++y == g.dst_h) {
        y = 0;
        src += (size_t)g.src_h * g.src_w * CN;
      }
      r = row_state<CN>(g, y);
    }
  }
};

template <int CN>
__global__ __launch_bounds__(THREADS) void resize_batch_kernel(const ResizeArgs a) {
  extern __shared__ uint4 smem[];
  uint2* cols = reinterpret_cast<uint2*>(smem);
  const Resample& g = a.g;
  if (!g.copy) build_columns(g, cols);
  __syncthreads();
  const size_t nRuns = (a.pixels + RUN - 1) / RUN;
  for (size_t run = (size_t)blockIdx.x * THREADS + threadIdx.x; run < nRuns; run += (size_t)gridDim.x * THREADS) {
    const size_t p0 = run * RUN;
    const int cnt = (int)(a.pixels - p0 < (size_t)RUN ? a.pixels - p0 : (size_t)RUN);
    const bool vec = a.aligned && cnt == RUN;
    uint32_t in[4 * CN], out[4 * CN];
#pragma unroll
    for (int k = 0; k < 4 * CN; ++k) out[k] = 0u;
    if (g.copy) {
#pragma unroll
      for (int k = 0; k < CN; ++k) load16(a.src + p0 * CN + 16 * k, vec, cnt * CN - 16 * k, in + 4 * k);
    }
    Cursor<CN> cur(a.src, g, p0);
#pragma unroll
    for (int i = 0; i < RUN; ++i) {
      if (i < cnt) {
        int v[CN];
        if (g.copy) {
#pragma unroll
          for (int k = 0; k < CN; ++k) v[k] = (int)byte_of(in, CN * i + k);
        } else {
          sample<CN>(cur.src, g, cols, cur.r, cur.x, v);
          cur.step(g);
        }
#pragma unroll
        for (int k = 0; k < CN; ++k) put_byte(out, CN * i + k, (uint32_t)((CN == 3 && a.swap_rb) ? v[2 - k] : v[k]));
      }
    }
#pragma unroll
    for (int k = 0; k < CN; ++k) store16(a.dst + p0 * CN + 16 * k, vec, cnt * CN - 16 * k, out + 4 * k);
  }
}

__global__ __launch_bounds__(THREADS) void overlay_batch_kernel(const OverlayArgs a, const VideoLut lut) {
  extern __shared__ uint4 smem[];
  float4* colour = reinterpret_cast<float4*>(smem);       // fl(lut[m][c] * beta), one row per mask value
  uint2* cols = reinterpret_cast<uint2*>(smem + 256);
  const Resample& g = a.g;
  {
    const uint8_t* row = reinterpret_cast<const uint8_t*>(lut.w) + 3 * threadIdx.x;   // THREADS == 256 rows
    colour[threadIdx.x] = make_float4((float)row[0] * a.beta, (float)row[1] * a.beta, (float)row[2] * a.beta, 0.f);
  }
  if (!g.copy) build_columns(g, cols);
  __syncthreads();
  const size_t nRuns = (a.pixels + RUN - 1) / RUN;
  for (size_t run = (size_t)blockIdx.x * THREADS + threadIdx.x; run < nRuns; run += (size_t)gridDim.x * THREADS) {
    const size_t p0 = run * RUN;
    const int cnt = (int)(a.pixels - p0 < (size_t)RUN ? a.pixels - p0 : (size_t)RUN);
    const bool vec = a.aligned && cnt == RUN;
    uint32_t in[12], out[12], small[4], big[4];
#pragma unroll
    for (int k = 0; k < 12; ++k) out[k] = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) big[k] = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) load16(a.frames + p0 * 3 + 16 * k, vec, cnt * 3 - 16 * k, in + 4 * k);
    if (g.copy) load16(a.masks + p0, vec, cnt, small);
    Cursor<1> cur(a.masks, g, p0);
#pragma unroll
    for (int i = 0; i < RUN; ++i) {
      if (i < cnt) {
        int m[1];
        if (g.copy) {
          m[0] = (int)byte_of(small, i);
        } else {
          sample<1>(cur.src, g, cols, cur.r, cur.x, m);
          cur.step(g);
        }
        put_byte(big, i, (uint32_t)m[0]);
        const float4 c = colour[m[0]];
        const float cc[3] = {c.x, c.y, c.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) put_byte(out, 3 * i + k, blend_u8(byte_of(in, 3 * i + k), a.alpha, cc[k], a.gamma));
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) store16(a.out + p0 * 3 + 16 * k, vec, cnt * 3 - 16 * k, out + 4 * k);
    if (a.mask_out) store16(a.mask_out + p0, vec, cnt, big);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

Resample resample_of(int srcH, int srcW, int dstH, int dstW) {
  Resample g;
  g.scale_x = 1.0 / ((double)dstW / (double)srcW);
  g.scale_y = 1.0 / ((double)dstH / (double)srcH);
  g.src_h = srcH, g.src_w = srcW, g.dst_h = dstH, g.dst_w = dstW;
  g.copy = srcH == dstH && srcW == dstW;
  return g;
}

unsigned grid_of(unsigned long long pixels) {
  const unsigned long long blocks = ((pixels + RUN - 1) / RUN + THREADS - 1) / THREADS;
  return (unsigned)(blocks < (unsigned long long)MAX_BLOCKS ? blocks : (unsigned long long)MAX_BLOCKS);
}

}  // namespace

hipError_t launch_resize_batch(const uint8_t* src, int n, int height, int width, int channels, int swapRB, int outW,
                               int outH, uint8_t* dst, hipStream_t s) {
  ResizeArgs a;
  a.src = src, a.dst = dst;
  a.pixels = (unsigned long long)n * outH * outW;
  a.g = resample_of(height, width, outH, outW);
  a.swap_rb = swapRB ? 1 : 0;
  a.aligned = aligned16(dst) && (!a.g.copy || aligned16(src));
  const size_t lds = a.g.copy ? 0 : (size_t)outW * sizeof(uint2);
  if (channels == 3)
    hipLaunchKernelGGL(resize_batch_kernel<3>, dim3(grid_of(a.pixels)), dim3(THREADS), lds, s, a);
  else
    hipLaunchKernelGGL(resize_batch_kernel<1>, dim3(grid_of(a.pixels)), dim3(THREADS), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_overlay_batch(const uint8_t* frames, int n, int height, int width, const uint8_t* masks, int maskH,
                                int maskW, const VideoLut& lut, float alpha, float beta, float gamma, uint8_t* overlay,
                                uint8_t* maskOut, hipStream_t s) {
  OverlayArgs a;
  a.frames = frames, a.masks = masks, a.out = overlay, a.mask_out = maskOut;
  a.pixels = (unsigned long long)n * height * width;
  a.g = resample_of(maskH, maskW, height, width);
  a.alpha = alpha, a.beta = beta, a.gamma = gamma;
  a.aligned = aligned16(frames) && aligned16(overlay) && aligned16(maskOut) && (!a.g.copy || aligned16(masks));
  const size_t lds = 256 * sizeof(float4) + (a.g.copy ? 0 : (size_t)width * sizeof(uint2));
  hipLaunchKernelGGL(overlay_batch_kernel, dim3(grid_of(a.pixels)), dim3(THREADS), lds, s, a, lut);
  return hipGetLastError();
}

}  // namespace unet

extern "C" {

int unet_resize_u8_batch(int device, const uint8_t* srcDev, int n, int height, int width, int channels, int swapRB,
                         int outW, int outH, uint8_t* dstDev, void* stream) {
  const unet::OpCall op{"unet_resize_u8_batch"};
  if (!srcDev || !dstDev) return op.refuse("a null pointer");
  if (n <= 0 || height <= 0 || width <= 0 || outW <= 0 || outH <= 0)
    return op.refuse("n and every size must be positive");
  if (channels != 1 && channels != 3) return op.refuse("channels must be 1 or 3");
  if (swapRB && channels != 3) return op.refuse("swap_rb needs 3 channels");
  // one image of either side must stay inside an int's worth of bytes (the kernels' row offsets are ints)
  if (!unet::fits_int((unsigned long long)height * width * channels) ||
      !unet::fits_int((unsigned long long)outH * outW * channels))
    return op.refuse("an image must be smaller than 2^31 bytes", UNET_ERR_SHAPE);
  if ((height != outH || width != outW) && outW > unet::VIDEO_MAX_RESIZE_WIDTH)
    return op.refuse("the destination of a resize is at most VIDEO_MAX_RESIZE_WIDTH wide", UNET_ERR_SHAPE);
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_resize_batch(srcDev, n, height, width, channels, swapRB, outW, outH, dstDev, (hipStream_t)stream));
}

int unet_overlay_u8_batch(int device, const uint8_t* framesDev, int n, int height, int width, const uint8_t* masksDev,
                          int maskH, int maskW, const uint8_t* lutHost, float alpha, float beta, float gamma,
                          uint8_t* overlayOutDev, uint8_t* maskOutDev, void* stream) {
  const unet::OpCall op{"unet_overlay_u8_batch"};
  if (!framesDev || !masksDev || !lutHost || !overlayOutDev) return op.refuse("a null pointer");
  if (n <= 0 || height <= 0 || width <= 0 || maskH <= 0 || maskW <= 0)
    return op.refuse("n and every size must be positive");
  if (!std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(gamma))
    return op.refuse("alpha, beta and gamma must be finite");
  if (!unet::fits_int(3ull * height * width) || !unet::fits_int((unsigned long long)maskH * maskW))
    return op.refuse("an image must be smaller than 2^31 bytes", UNET_ERR_SHAPE);
  if ((height != maskH || width != maskW) && width > unet::VIDEO_MAX_RESIZE_WIDTH)
    return op.refuse("the destination of a resize is at most VIDEO_MAX_RESIZE_WIDTH wide", UNET_ERR_SHAPE);
  if (int rc = op.on(device)) return rc;
  unet::VideoLut lut;   // by value in the kernel's arguments: the caller's table is free once this returns
  memcpy(lut.w, lutHost, sizeof(lut.w));
  return op.done(unet::launch_overlay_batch(framesDev, n, height, width, masksDev, maskH, maskW, lut, alpha, beta, gamma,
                                            overlayOutDev, maskOutDev, (hipStream_t)stream));
}

}  // extern "C"
