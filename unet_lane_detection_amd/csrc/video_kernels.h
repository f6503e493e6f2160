// The video path around the network (reference src/unet.py:99-140, `predict_video`): a batch of frames is resized to
// the network's input with the colour swap, and the network's small masks come back as a coloured overlay -
//   cv2.resize(mask) -> cv2.applyColorMap -> cv2.addWeighted(frame, alpha, coloured, beta, gamma)
// - in one pass over the frames.  The arithmetic is stated in tests/video_model.py; the kernels in video_kernels.cpp
// reproduce it bit for bit.  A translation unit of its own, like augment_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace unet {

constexpr int VIDEO_MAX_RESIZE_WIDTH = 7680;   // the column table of a resampling launch lives in LDS (8 bytes a column)

// the colour table, passed by value: 256 rows of 3 bytes in the frame's channel order
struct VideoLut {
  uint32_t w[192];
};

// ---- device helpers shared with the lane view (laneview_kernels.cpp) ----

// byte j of a run held as dwords; j is a constant after unrolling
__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 255u; }
__device__ __forceinline__ void put_byte(uint32_t* w, int j, uint32_t v) { w[j >> 2] |= v << (8 * (j & 3)); }

// 16 bytes at p as one access, or its first `bytes` (which may be <= 0) one by one
__device__ __forceinline__ void load16(const uint8_t* __restrict__ p, bool vec, int bytes, uint32_t* w) {
  if (vec) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
    w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < bytes) put_byte(w, j, p[j]);
  }
}

__device__ __forceinline__ void store16(uint8_t* __restrict__ p, bool vec, int bytes, const uint32_t* w) {
  if (vec) {
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < bytes) p[j] = (uint8_t)byte_of(w, j);
  }
}

// One channel of cv2.addWeighted as include/unet_hip.h states it for unet_overlay_u8_batch:
// clamp(rint(fl(fl(fl(frame * alpha) + colourBeta) + gamma)), 0, 255) with colourBeta = fl(colour * beta); every fl is
// one fp32 rounding (nothing is contracted) and rintf rounds half to even.
__device__ __forceinline__ uint32_t blend_u8(uint32_t frame, float alpha, float colourBeta, float gamma) {
#pragma clang fp contract(off)
  float v = (float)frame * alpha;
  v = v + colourBeta;
  v = v + gamma;
  v = fminf(fmaxf(rintf(v), 0.f), 255.f);
  return (uint32_t)(int)v;
}

// src (n,height,width,CN) u8 -> dst (n,outH,outW,CN) u8, cv::resize INTER_LINEAR per image; channels is 1 or 3;
// swapRB exchanges channels 0 and 2 of a 3-channel image
hipError_t launch_resize_batch(const uint8_t* src, int n, int height, int width, int channels, int swapRB, int outW,
                               int outH, uint8_t* dst, hipStream_t s);

// frames (n,height,width,3) u8, masks (n,maskH,maskW) u8 -> overlay (n,height,width,3) u8 and, unless null,
// maskOut (n,height,width) u8 = the resized mask
hipError_t launch_overlay_batch(const uint8_t* frames, int n, int height, int width, const uint8_t* masks, int maskH,
                                int maskW, const VideoLut& lut, float alpha, float beta, float gamma, uint8_t* overlay,
                                uint8_t* maskOut, hipStream_t s);

}  // namespace unet
