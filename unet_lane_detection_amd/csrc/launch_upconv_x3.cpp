// Launch unit of the f16x3 transposed convolutions: upconv_x3_ws.h, upconv_x3_r512.h and upconv_x3_win.h (launch.h).
#include "launch.h"

#include "upconv_x3_ws.h"
#include "upconv_x3_r512.h"
#include "upconv_x3_win.h"

namespace {

hipError_t launch(void (*kern)(const unet::UpconvX3Args), const unet::UpconvX3Args& a, int grid, int block, int lds,
                  hipStream_t s) {
  const hipError_t e = unet::ensure_dyn_lds((const void*)kern, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), (size_t)lds, s, a);
  return hipGetLastError();
}

// MODE 0: ConvTranspose2d, MODE 1: the plain GEMM
template <int MODE>
hipError_t launch_upconv_x3(const unet::UpconvX3Args& a, int grid, bool r512, bool outQ, hipStream_t s) {
  void (*kern)(const unet::UpconvX3Args);
  if (!r512)
    kern = unet::upconv2x2_x3_ws_kernel<MODE>;
  else if constexpr (MODE == 0)
    kern = outQ ? unet::upconv2x2_x3_r512_kernel<0, true> : unet::upconv2x2_x3_r512_kernel<0>;
  else
    kern = unet::upconv2x2_x3_r512_kernel<1>;
  const int lds = r512 ? unet::UpconvX3RShape::LDS_BYTES : unet::UpconvX3Shape::LDS_BYTES;
  return launch(kern, a, grid, r512 ? 256 : 512, lds, s);
}

}  // namespace

hipError_t unet::launch_upconv_x3(const UpconvX3Args& a, int grid, bool r512, int mode, bool outQ, hipStream_t s) {
  return mode == 0 ? ::launch_upconv_x3<0>(a, grid, r512, outQ, s) : ::launch_upconv_x3<1>(a, grid, r512, outQ, s);
}

hipError_t unet::launch_upconv_win(const UpconvX3Args& a, int grid, bool w14, hipStream_t s) {
  const int lds = w14 ? UpconvX3WShape<14>::LDS_BYTES : UpconvX3WShape<28>::LDS_BYTES;
  return launch(w14 ? upconv2x2_x3_win_kernel<14> : upconv2x2_x3_win_kernel<28>, a, grid, 256, lds, s);
}
