// Frame correction on the device: gray-world white balance, percentile stretch, a tone table and CLAHE, decided per
// frame from the frame's own histograms and applied where the frame lies - the stage between "the message's rows are
// on the device" and "the warp reads them".  It answers the failure the reference is built around (README.md:325-342,
// :380-429: the white marking leaves the HSV range under a colour cast, a shadow or glare); the reference itself has no
// such code.  The arithmetic is stated in include/unet_hip.h and tests/correct_model.py; the kernels in
// correct_kernels.cpp reproduce it bit for bit.  Parity with cv2.createCLAHE or any outside implementation is
// unpinned: cv2 is not installed where this is tested and the reference ships no fixture.  A translation unit of its
// own, like diagnose_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace unet {

constexpr int CORRECT_PLAN_WORDS = 8;

// one frame's part of the work buffer, in bytes from its start (include/unet_hip.h documents the layout)
constexpr size_t CORRECT_HIST_OFF = 0;                                            // 3 x 256 uint32
constexpr size_t CORRECT_PLAN_OFF = CORRECT_HIST_OFF + 3 * 256 * 4;               // 8 uint32
constexpr size_t CORRECT_LUT_OFF = CORRECT_PLAN_OFF + CORRECT_PLAN_WORDS * 4;     // 3 x 256 bytes
constexpr size_t CORRECT_THIST_OFF = CORRECT_LUT_OFF + 3 * 256;                   // tiles x 256 uint32
inline size_t correct_tlut_off(int tiles) { return CORRECT_THIST_OFF + (size_t)tiles * 1024; }   // tiles x 256 bytes
inline size_t correct_frame_bytes(int tiles) { return correct_tlut_off(tiles) + (size_t)tiles * 256; }

struct CorrectParams {
  const uint8_t* frames;
  uint8_t* out;
  uint8_t* work;
  int n, height, width;
  long long stride, ostride;   // bytes from row to row of the input and of the output
  int swap;                    // byte 0 is blue
  int gx, gy;                  // the CLAHE grid; 1 x 1 without CLAHE
  int whiteBalance, maxGain, loBp, hiBp, clahe, clipQ8, onlyFlagged, darkLimit, brightLimit;
  uint8_t tone[256];
};

// init, channel histograms, plan, (with CLAHE: tile histograms, tile tables,) apply: six or four launches on s; no
// block waits for another.
hipError_t launch_correct(const CorrectParams& p, hipStream_t s);

}  // namespace unet
