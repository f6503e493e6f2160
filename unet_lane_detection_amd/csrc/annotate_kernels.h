// Annotations on the device: an annotator's polygons (LabelMe shapes, README.md:1013-1052 of the reference:
// cv2.fillPoly(mask, [points], 255) per shape) rasterised into training masks at whatever size a stage trains at - the
// step in front of augment.DeviceDataset.  The rule is integer arithmetic and is stated in include/unet_hip.h and
// tests/annotate_model.py: even-odd parity at the pixel centre plus an 8-connected outline, painter's order, the source
// point of an output pixel taken as (X * src_w) / out_w, (Y * src_h) / out_h.  The kernel in annotate_kernels.cpp
// reproduces it bit for bit.  Parity with cv2.fillPoly itself is unpinned: cv2 is not installed where this is tested
// and the reference ships no fixture; along boundaries cv2's fixed-point edge walk and line iterator differ.  A
// translation unit of its own, like correct_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace unet {

constexpr int ANNOTATE_COORD_LIMIT = 1 << 20;   // |x|, |y| of a vertex; the kernel clamps to it
constexpr int ANNOTATE_MAX_SIDE = 16384;        // source and output sizes

struct FillParams {
  const int32_t* vertices;      // (V, 2): x, y
  const int32_t* polyOffsets;   // P + 1, into vertices
  const uint8_t* polyValues;    // P
  const int32_t* frameOffsets;  // n + 1, into polygons
  uint8_t* out;                 // (n, outH, outW)
  int n, srcH, srcW, outH, outW;
};

// one launch on s: a block per 64 x 64 tile of output pixels of one frame
hipError_t launch_fill_polygons(const FillParams& p, hipStream_t s);

}  // namespace unet
