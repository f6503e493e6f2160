// Hybrid units of the int8 tier: launchers of the fp16 kernels of conv_h16.h.  A translation unit of its own, like
// calib_kernels.cpp: the code object of unet_hip.cpp (the int8 kernels among them) does not change with these kernels.
#define UNET_CONV_H16_KERNELS 1
#include "conv_h16.h"

#include <algorithm>

namespace unet {

namespace {

unsigned h16_grid_for(size_t total) { return (unsigned)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, 65536)); }

template <int TAPS, int NCS>
void launch_taps(const ConvH16Args& a, bool in16, bool out16, dim3 grid, hipStream_t s) {
  if (in16 && out16)
    hipLaunchKernelGGL((conv_h16_kernel<TAPS, true, true, NCS>), grid, dim3(256), 0, s, a);
  else if (in16)
    hipLaunchKernelGGL((conv_h16_kernel<TAPS, true, false, NCS>), grid, dim3(256), 0, s, a);
  else if (out16)
    hipLaunchKernelGGL((conv_h16_kernel<TAPS, false, true, NCS>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((conv_h16_kernel<TAPS, false, false, NCS>), grid, dim3(256), 0, s, a);
}

}  // namespace

hipError_t launch_conv_h16(ConvH16Args a, int taps, bool in16, bool out16, hipStream_t s) {
  const long npix = (long)a.N * a.H * a.W;
  if (a.N <= 0 || a.H <= 0 || a.W <= 0 || npix * 4 >= (1L << 31) || (taps != 9 && taps != 1)) return hipErrorInvalidValue;
  if (a.cinStage <= 0 || a.cinStage % 8 || a.cinStage > a.ldi || a.chunks != (a.cinStage + 63) / 64) return hipErrorInvalidValue;
  if (a.cols <= 0 || a.cols % 16 || a.co_off % 16 || a.ldi % 32 || a.ldo % 32) return hipErrorInvalidValue;
  if (a.narrow && (a.cols > 32 || a.scatter)) return hipErrorInvalidValue;
  a.coTiles = (a.cols + 63) / 64;
  if (taps == 9) {
    a.tilesX = (a.W + 15) / 16;
    a.tilesY = (a.H + 7) / 8;
    a.pixTiles = a.N * a.tilesY * a.tilesX;
  } else {
    a.tilesX = a.tilesY = 0;
    a.pixTiles = (int)((npix + 127) / 128);
  }
  const dim3 grid((unsigned)a.pixTiles, (unsigned)a.coTiles);
  if (taps == 9 && a.narrow)
    launch_taps<9, 2>(a, in16, out16, grid, s);
  else if (taps == 9)
    launch_taps<9, 4>(a, in16, out16, grid, s);
  else if (a.narrow)
    launch_taps<1, 2>(a, in16, out16, grid, s);
  else
    launch_taps<1, 4>(a, in16, out16, grid, s);
  return hipGetLastError();
}

hipError_t launch_maxpool2x2_h16(const uint16_t* x, int n, int h, int w, int c, int ldi, uint16_t* y, int ldo, hipStream_t s) {
  if (c <= 0 || c % 8 || h % 2 || w % 2 || ldi % 8 || ldo % 8) return hipErrorInvalidValue;
  const size_t total = (size_t)n * (h / 2) * (w / 2) * (c / 8);
  hipLaunchKernelGGL(maxpool2x2_h16_kernel, dim3(h16_grid_for(total)), dim3(256), 0, s, x, n, h, w, c, ldi, y, ldo);
  return hipGetLastError();
}

hipError_t launch_head_h16(const void* x, bool in16, int ldx, int c, size_t npix, const uint16_t* w16, int xzp, float m,
                           float b, float* logits, float* probs, uint8_t* mask, float thr, hipStream_t s) {
  if (c <= 0 || c % 8 || ldx % 8) return hipErrorInvalidValue;
  const dim3 grid(h16_grid_for(npix));
  if (in16)
    hipLaunchKernelGGL(head_h16_kernel<true>, grid, dim3(256), 0, s, x, ldx, c, npix, w16, xzp, m, b, logits, probs, mask, thr);
  else
    hipLaunchKernelGGL(head_h16_kernel<false>, grid, dim3(256), 0, s, x, ldx, c, npix, w16, xzp, m, b, logits, probs, mask, thr);
  return hipGetLastError();
}

}  // namespace unet
