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
