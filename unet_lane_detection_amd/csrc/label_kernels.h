// Lane instances on the device: connected-component labelling of a mask batch (4- or 8-connected), the per-component
// integer statistics (area, bounding box, the moment sums S_k = sum y^k and T_k = sum x y^k that lanefit.solve takes,
// first pixel, border flags) and a component filter that writes a cleaned mask for the existing kernels.  The
// arithmetic is stated in include/unet_hip.h and tests/label_model.py; the kernels in label_kernels.cpp reproduce it
// bit for bit.  A translation unit of its own, like lanefit_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace unet {

constexpr int LABEL_WORDS = 16;             // UNET_LABEL_WORDS
constexpr int LABEL_SIDE_MAX = 2048;        // height and width
constexpr int LABEL_COMPONENTS_MAX = 65536;

// bytes of workspace launch_label needs: two 32-bit words per row (0 outside the domain of unet_label_u8_batch)
size_t label_work_bytes(int n, int height, int width);

// masks (n,height,width) u8 -> labels (n,height,width) i32, header (n,4) u64, records (n,cap,16) u64.  The caller
// has checked the domain of unet_label_u8_batch.
hipError_t launch_label(const uint8_t* masks, int n, int height, int width, int level, int connectivity,
                        int32_t* labels, int cap, unsigned long long* header, unsigned long long* records, void* work,
                        hipStream_t s);

// labels, header, records of launch_label -> keep (n,cap) u8 and mask (n,height,width) u8.  The caller has checked
// the domain of unet_keep_components_u8_batch.
hipError_t launch_keep_components(const int32_t* labels, int n, int height, int width, const unsigned long long* header,
                                  const unsigned long long* records, int cap, int minArea, int minHeight, int minWidth,
                                  int keepLargest, uint8_t* keep, uint8_t* mask, hipStream_t s);

}  // namespace unet
