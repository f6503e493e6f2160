// Training-time augmentation on the device (reference README.md:2035-2055, `get_transforms`): flip and rotation,
// brightness / contrast, hue / saturation / value, Gaussian blur of a batch gathered from a resident data set, and the
// masks' targets, in one launch.  The arithmetic is stated in unet_lane_detection_amd/augment.py (`apply_model`); the
// kernel in augment_kernels.cpp reproduces it bit for bit.  A translation unit of its own, like loss_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace unet {

// One record per output sample; augment.PARAMS_DTYPE is the same layout.
struct AugmentParams {
  double m[6];       // inverse affine on offsets from the image centre: xs = (m0 dx + m1 dy + m2) + cx, ys likewise
  int32_t src;       // index of the source frame
  uint32_t flags;    // AUG_* bits
  float alpha;       // brightness / contrast: trunc(clip(v * alpha + beta255, 0, 255))
  float beta255;
  float dh, ds, dv;  // shifts of H (of 180), S and V (of 255)
  int32_t blur;      // 1 (off), 3, 5 or 7
};
static_assert(sizeof(AugmentParams) == 80, "augment.PARAMS_DTYPE mirrors this layout");

constexpr uint32_t AUG_FLIP = 1, AUG_ROTATE = 2;   // informative: the matrix carries both
constexpr uint32_t AUG_BC = 4, AUG_HSV = 8;

constexpr int AUG_MIN_SIDE = 8;       // reflect-101 with the blur's 3-pixel halo stays single-bounce
constexpr int AUG_MAX_SIDE = 32768;   // 1/32-pixel coordinates stay inside an int

// images (nSource,H,W,3) u8, masks (nSource,H,W) u8 or null, params nOut records on the device ->
// out (nOut,H,W,3) u8 and, with masks, targets (nOut,1,H,W) float = mask > threshold - or, with `labels` given (the
// label mode: targets is then ignored), labels (nOut,H,W) u8 = the nearest-sampled mask byte itself.
hipError_t launch_augment(const uint8_t* images, const uint8_t* masks, int nSource, int height, int width,
                          const AugmentParams* params, int nOut, int maskThreshold, uint8_t* out, float* targets,
                          uint8_t* labels, hipStream_t s);

}  // namespace unet
