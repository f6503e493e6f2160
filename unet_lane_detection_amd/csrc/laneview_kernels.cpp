// The lane view's kernel (laneview_kernels.h): plain C++, 16-byte loads and stores.
//
// A thread takes a run of RUN = 16 consecutive pixels of one camera row: 48 bytes of the frame in (three 16-byte
// loads), 48 bytes of the view out (three 16-byte stores) and 16 bytes of the layer plane.  A run never crosses a row,
// so the row pitch `step` only enters the run's base address.  Each of the three addresses takes the 16-byte form
// where it is 16-byte aligned and the run is whole; otherwise - a base pointer or a `step` that is no multiple of 16,
// a width whose 3 * width is none, the tail of a row - its bytes move one by one (load16 / store16 of
// video_kernels.h).  The pixels between are computed by the same code, so both forms give the same bits.
//
// A workgroup belongs to one frame (blockIdx.y) at a time: its first k threads clamp the frame's k curve records into
// LDS, once, and every pixel reads them from there at a wave-uniform address.  Per pixel: one double-precision divide
// and three multiply-add pairs for the position, per record three 64-bit products, and only for a pixel that is
// INSIDE and that no curve claimed the four-byte gather from two rows of the bird's-eye mask.
//
// Bounds: a run reads 3 * cnt <= 3 * width - 3 * x0 bytes of its row, inside the first 3 * width <= step bytes; the
// mask taps are tested against warp_h and warp_w by warp_sample; the records read are those of frame f < n and i < k.
// No atomics, no workgroup waits for another, no global scratch.
#include "laneview_kernels.h"

#include "op_entry.h"
#include "video_kernels.h"
#include "warp_sample.h"

#include <cmath>


// The model rounds every floating-point operation on its own (numpy has no fused multiply-add); so does this file.
#pragma clang fp contract(off)

namespace unet {

namespace {

constexpr int THREADS = 256, RUN = 16, MAX_BLOCKS = 2048;

struct ViewArgs {
  const uint8_t* frames;
  const uint8_t* masks;      // or null
  const long long* curves;   // or null with k = 0
  uint8_t* view;             // or null
  uint8_t* layers;           // or null
  double m[9];
  float alpha, beta, gamma;
  uint32_t area, marking;    // colours, byte c = channel c
  int n, height, width, step, warp_w, warp_h, level, k;
  int reach;                 // 16 * thickness, in 1/32 pixel
  int draw_area, draw_marking;
};

// a record as the pixels use it: clamped, its rows in 1/32 pixel
struct Curve {
  long long A, B, C;
  int lo, hi;       // covers Y iff present and lo <= Y <= hi
  uint32_t flags, colour;
};

__device__ __forceinline__ long long clamp_ll(long long v, long long bound) {
  return v < -bound ? -bound : (v > bound ? bound : v);
}

__device__ __forceinline__ Curve load_curve(const long long* __restrict__ w, int warp_h) {
  Curve c;
  c.flags = (uint32_t)w[0] & 7u;
  const long long y0 = w[1] < 0 ? 0 : (w[1] > warp_h - 1 ? warp_h - 1 : w[1]);
  const long long y1 = w[2] < 0 ? 0 : (w[2] > warp_h - 1 ? warp_h - 1 : w[2]);
  c.lo = 32 * (int)y0;
  c.hi = 32 * (int)y1 + 31;
  c.A = clamp_ll(w[3], (1ll << 30) - 1);
  c.B = clamp_ll(w[4], (1ll << 45) - 1);
  c.C = clamp_ll(w[5], (1ll << 57) - 1);
  c.colour = (uint32_t)w[6] & 0xffffffu;
  return c;
}

// the layer of camera pixel (x, y) and the colour that goes with it (untouched on layer 0)
__device__ __forceinline__ int layer_of(const ViewArgs& a, const Curve* cv, const uint8_t* __restrict__ mask, int x,
                                        int y, uint32_t& colour) {
  const double xs = (double)x, ys = (double)y;
  const double w = a.m[6] * xs + a.m[7] * ys + a.m[8];
  if (!(w > 0.0)) return 0;
  const double s = 32.0 / w;
  double fx = (a.m[0] * xs + a.m[1] * ys + a.m[2]) * s;
  double fy = (a.m[3] * xs + a.m[4] * ys + a.m[5]) * s;
  fx = fmin(fmax(fx, -2147483648.0), 2147483647.0);   // fmax drops a NaN: it becomes -2^31
  fy = fmin(fmax(fy, -2147483648.0), 2147483647.0);
  const long long X = (long long)rint(fx), Y = (long long)rint(fy);
  if (X < 0 || X >= 32ll * a.warp_w || Y < 0 || Y >= 32ll * a.warp_h) return 0;
  bool area = false, left = false;   // left: record i - 1 covers Y and fills up to record i
  long long leftX = 0;
  for (int i = 0; i < a.k; ++i) {
    const Curve c = cv[i];
    const bool on = (c.flags & 1u) && Y >= c.lo && Y <= c.hi;
    long long xi = 0;
    if (on) {
      xi = (c.A * Y * Y + c.B * Y + c.C) >> 32;   // below 2^63: include/unet_hip.h
      const long long d = X - xi;
      if ((c.flags & 4u) && d <= a.reach && d >= -(long long)a.reach) {
        colour = c.colour;
        return 3 + i;
      }
      if (left && leftX <= X && X <= xi) area = true;
    }
    left = on && (c.flags & 2u);
    leftX = xi;
  }
  if (mask && a.draw_marking) {
    int v[1];
    warp_sample<1>(mask, a.warp_h, a.warp_w, (size_t)a.warp_w, X, Y, v);
    if (v[0] > a.level) {
      colour = a.marking;
      return 2;
    }
  }
  if (area && a.draw_area) {
    colour = a.area;
    return 1;
  }
  return 0;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__global__ __launch_bounds__(THREADS) void lane_view_kernel(const ViewArgs a) {
  __shared__ Curve cv[LANE_VIEW_MAX];
  const int runsPerRow = (a.width + RUN - 1) / RUN;
  const int runs = a.height * runsPerRow;   // at most 4096 * 256
  for (int f = blockIdx.y; f < a.n; f += gridDim.y) {
    if ((int)threadIdx.x < a.k)
      cv[threadIdx.x] = load_curve(a.curves + ((size_t)f * a.k + threadIdx.x) * LANE_VIEW_WORDS, a.warp_h);
    __syncthreads();
    const uint8_t* mask = a.masks ? a.masks + (size_t)f * a.warp_h * a.warp_w : nullptr;
    for (int run = blockIdx.x * THREADS + threadIdx.x; run < runs; run += gridDim.x * THREADS) {
      const int y = run / runsPerRow, x0 = (run - y * runsPerRow) * RUN;
      const int cnt = a.width - x0 < RUN ? a.width - x0 : RUN;
      const size_t row = (size_t)f * a.height + y;
      const uint8_t* src = a.frames + row * a.step + (size_t)x0 * 3;
      uint8_t* dst = a.view ? a.view + (row * a.width + x0) * 3 : nullptr;
      uint8_t* lay = a.layers ? a.layers + row * a.width + x0 : nullptr;
      uint32_t in[12], out[12], which[4];
#pragma unroll
      for (int j = 0; j < 12; ++j) in[j] = out[j] = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) which[j] = 0u;
      if (dst) {
        const bool vec = cnt == RUN && aligned16(src);
#pragma unroll
        for (int j = 0; j < 3; ++j) load16(src + 16 * j, vec, cnt * 3 - 16 * j, in + 4 * j);
      }
#pragma unroll
      for (int i = 0; i < RUN; ++i) {
        if (i < cnt) {
          uint32_t colour = 0u;
          const int layer = layer_of(a, cv, mask, x0 + i, y, colour);
          put_byte(which, i, (uint32_t)layer);
          if (dst) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const uint32_t own = byte_of(in, 3 * i + c);
              const uint32_t col = layer ? (colour >> (8 * c)) & 255u : own;
              put_byte(out, 3 * i + c, blend_u8(own, a.alpha, (float)col * a.beta, a.gamma));
            }
          }
        }
      }
      if (dst) {
        const bool vec = cnt == RUN && aligned16(dst);
#pragma unroll
        for (int j = 0; j < 3; ++j) store16(dst + 16 * j, vec, cnt * 3 - 16 * j, out + 4 * j);
      }
      if (lay) store16(lay, cnt == RUN && aligned16(lay), cnt, which);
    }
    __syncthreads();   // the next frame's records replace these
  }
}

}  // namespace

hipError_t launch_lane_view(const uint8_t* frames, int n, int height, int width, int step, const double* m, int warpW,
                            int warpH, const uint8_t* masks, int level, const long long* curves, int k,
                            const unet_lane_view_style& style, uint8_t* view, uint8_t* layers, hipStream_t s) {
  ViewArgs a;
  a.frames = frames, a.masks = masks, a.curves = curves, a.view = view, a.layers = layers;
  for (int i = 0; i < 9; ++i) a.m[i] = m[i];
  a.alpha = style.alpha, a.beta = style.beta, a.gamma = style.gamma;
  a.area = (uint32_t)style.area[0] | ((uint32_t)style.area[1] << 8) | ((uint32_t)style.area[2] << 16);
  a.marking = (uint32_t)style.marking[0] | ((uint32_t)style.marking[1] << 8) | ((uint32_t)style.marking[2] << 16);
  a.n = n, a.height = height, a.width = width, a.step = step, a.warp_w = warpW, a.warp_h = warpH, a.level = level;
  a.k = k;
  a.reach = 16 * style.thickness;
  a.draw_area = (style.layers & UNET_LANE_VIEW_AREA) ? 1 : 0;
  a.draw_marking = (style.layers & UNET_LANE_VIEW_MARKING) ? 1 : 0;
  const int runs = height * ((width + RUN - 1) / RUN);
  const int perFrame = (runs + THREADS - 1) / THREADS;
  const int gy = n < 65535 ? n : 65535;
  int gx = MAX_BLOCKS / gy;   // about MAX_BLOCKS workgroups in all; a frame's runs are strided over its share
  if (gx < 1) gx = 1;
  if (gx > perFrame) gx = perFrame;
  hipLaunchKernelGGL(lane_view_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace unet

extern "C" {

size_t unet_lane_view_style_bytes(void) { return sizeof(unet_lane_view_style); }

int unet_lane_view_u8_batch(int device, const uint8_t* framesDev, int n, int height, int width, int step,
                            const double m[9], int warpW, int warpH, const uint8_t* masksDev, int level,
                            const long long* curvesDev, int k, const unet_lane_view_style* style, uint8_t* viewOutDev,
                            uint8_t* layersOutDev, void* stream) {
  const unet::OpCall op{"unet_lane_view_u8_batch"};
  if (!framesDev || !m) return op.refuse("a null pointer (frames_dev, m)");
  if (!viewOutDev && !layersOutDev) return op.refuse("view_out_dev and layers_out_dev must not both be null");
  if (n <= 0) return op.refuse("n must be positive");
  if (height < 1 || height > unet::LANE_VIEW_SIZE_MAX) return op.refuse("height must lie in 1 .. 4096");
  if (width < 1 || width > unet::LANE_VIEW_SIZE_MAX) return op.refuse("width must lie in 1 .. 4096");
  if (step < 3 * width) return op.refuse("step must be at least 3 * width");
  if (!unet::fits_int((unsigned long long)n * height * step))
    return op.refuse("n * height * step must be smaller than 2^31");
  if (warpW < 1 || warpW > unet::LANE_VIEW_WARP_W_MAX) return op.refuse("warp_w must lie in 1 .. 8192");
  if (warpH < 1 || warpH > unet::LANE_VIEW_WARP_H_MAX) return op.refuse("warp_h must lie in 1 .. 2048");
  if (level < 0 || level > 255) return op.refuse("level must lie in 0 .. 255");
  if (k < 0 || k > UNET_LANE_VIEW_MAX) return op.refuse("k must lie in 0 .. UNET_LANE_VIEW_MAX");
  if ((k == 0) != (curvesDev == nullptr)) return op.refuse("k must be 0 exactly when curves_dev is null");
  if (unet::misaligned(curvesDev, 8)) return op.refuse("curves_dev must be 8-byte aligned");
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(m[i])) return op.refuse("all nine entries of m must be finite");
  unet_lane_view_style st;
  if (style) {
    st = *style;
  } else {
    st.alpha = 0.7f, st.beta = 0.3f, st.gamma = 0.f;
    st.area[0] = st.marking[0] = 0, st.area[1] = st.marking[1] = 255, st.area[2] = st.marking[2] = 0;
    st.reserved[0] = st.reserved[1] = 0;
    st.thickness = 4;
    st.layers = UNET_LANE_VIEW_AREA | UNET_LANE_VIEW_MARKING;
  }
  if (!std::isfinite(st.alpha) || !std::isfinite(st.beta) || !std::isfinite(st.gamma))
    return op.refuse("alpha, beta and gamma must be finite");
  if (st.thickness < 1 || st.thickness > unet::LANE_VIEW_THICKNESS_MAX) return op.refuse("thickness must lie in 1 .. 64");
  if (st.layers & ~(UNET_LANE_VIEW_AREA | UNET_LANE_VIEW_MARKING)) return op.refuse("an unknown bit in style->layers");
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_lane_view(framesDev, n, height, width, step, m, warpW, warpH, masksDev, level, curvesDev, k, st,
                                        viewOutDev, layersOutDev, (hipStream_t)stream));
}

}  // extern "C"
