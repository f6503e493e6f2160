// Launch unit of the composed decoder step and of the first encoder block: conv_x3_dec.h, conv_x3_t448.h's
// conv3x3_x3_t448add_kernel and conv_x3_enc1.h (launch.h).
#include "launch.h"

#include "conv_x3_dec.h"
#include "conv_x3_enc1.h"

namespace {

template <class A>
hipError_t launch(void (*kern)(const A), const A& a, int grid, int lds, hipStream_t s) {
  const hipError_t e = unet::ensure_dyn_lds((const void*)kern, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), (size_t)lds, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t unet::launch_upcat_dec(const UpcatX3Args& a, int grid, int wco, hipStream_t s) {
  return launch(wco == 2 ? upcat_conv3x3_dec_f16x3_kernel<2> : upcat_conv3x3_dec_f16x3_kernel<1>, a, grid, X3DShape::LDS_BYTES, s);
}

hipError_t unet::launch_conv_t448add(const ConvX3AddArgs& a, int grid, bool flat, hipStream_t s) {
  using S = X3TShape<28, x3t_row_blocks(4)>;
  const int lds = flat ? S::LDS_BYTES_FLAT : S::LDS_BYTES_PLAIN;
  return launch(flat ? conv3x3_x3_t448add_kernel<true> : conv3x3_x3_t448add_kernel<false>, a, grid, lds, s);
}

hipError_t unet::launch_conv_enc1(const ConvEnc1X3Args& a, int grid, hipStream_t s) {
  return launch(conv3x3_enc1_x3_kernel, a, grid, X3Enc1Shape::LDS_BYTES, s);
}
