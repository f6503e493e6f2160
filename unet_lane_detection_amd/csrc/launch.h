// The launches the host logic can name: one plain function per kernel structure, each defined in the translation unit
// that instantiates the structure's kernels (launch_*.cpp, named after the header it instantiates).  The host logic
// (unet_hip.cpp and its .inc files) plans, fills the argument struct, computes grid and labels and calls these; it names
// no kernel template of the structures itself, so it compiles without their device code.  A new instance of a structure
// goes into that structure's launch unit, behind the integers its plan already carries.
//
// Every function opts the instance into its shape's dynamic LDS (ensure_dyn_lds), launches it and returns
// hipGetLastError(); an integer combination the library carries no instance for lands on the same instance as before
// the units existed (the `default:` branches moved with the funnels).
#pragma once
#include <hip/hip_runtime.h>

namespace unet {

struct ConvX3Args;       // conv_x3_ws.h
struct ConvX3AddArgs;    // conv_x3_t448.h
struct ConvQ8Args;       // conv_q8_r512.h
struct UpconvX3Args;     // upconv_x3_ws.h
struct UpcatX3Args;      // conv_x3_dec.h
struct ConvEnc1X3Args;   // conv_x3_enc1_args.h
struct ConvArgsBf;       // igemm_bf16.h
struct ConvWsArgs;       // conv_bf16_ws.h
struct ConvBfRArgs;      // conv_bf16_r512.h

// Kernels that need more dynamic LDS than the default opt in once per (device, kernel).  Defined in unet_hip.cpp.
hipError_t ensure_dyn_lds(const void* fn, int bytes);

// launch_conv_x3_ws.cpp: conv3x3_x3_ws_kernel<tw 32 / 16, epi 0 - 3, flat>
hipError_t launch_conv_x3(const ConvX3Args& a, int grid, int tw, int epi, bool flat, hipStream_t s);
// launch_conv_x3_r512.cpp: conv3x3_x3_r512_kernel<tw 28 / 14 / 32 / 16 / 8, waves 1 / 2, epi 0 / 3, flat>
hipError_t launch_conv_r512(const ConvX3Args& a, int grid, int tw, int waves, bool flat, bool f32out, hipStream_t s);
// launch_conv_x3_t448.cpp: conv3x3_x3_t448_kernel<tw 28 / 32, waves 1 / 2 / 4, epi 0 - 3, flat>
hipError_t launch_conv_t448(const ConvX3Args& a, int grid, int tw, int waves, int epi, bool flat, hipStream_t s);
// launch_conv_q8_r512.cpp: conv3x3_q8_r512_kernel<tw 28 / 14, epi 0 / 4, flat>
hipError_t launch_conv_q8(const ConvQ8Args& a, int grid, int tw, int epi, bool flat, hipStream_t s);

// launch_upconv_x3.cpp: upconv2x2_x3_ws_kernel<mode> or, r512, upconv2x2_x3_r512_kernel<mode, outQ> ...
hipError_t launch_upconv_x3(const UpconvX3Args& a, int grid, bool r512, int mode, bool outQ, hipStream_t s);
// ... and upconv2x2_x3_win_kernel<wmax 28 / 14>
hipError_t launch_upconv_win(const UpconvX3Args& a, int grid, bool w14, hipStream_t s);

// launch_conv_x3_dec.cpp: upcat_conv3x3_dec_f16x3_kernel<wco 1 / 2>, conv3x3_x3_t448add_kernel<flat>,
// conv3x3_enc1_x3_kernel
hipError_t launch_upcat_dec(const UpcatX3Args& a, int grid, int wco, hipStream_t s);
hipError_t launch_conv_t448add(const ConvX3AddArgs& a, int grid, bool flat, hipStream_t s);
hipError_t launch_conv_enc1(const ConvEnc1X3Args& a, int grid, hipStream_t s);

// launch_conv_bf16.cpp: igemm_bf16_kernel<taps 9 / 1 (mode 0 / 1), ms 7 / 4, ns 4 / 2>,
// conv3x3_bf16_r512_kernel<tw 28 / 14, wpx 1 / 2, flat>, conv3x3_bf16_ws_kernel<epi 0 - 2>
hipError_t launch_bf(const ConvArgsBf& a, dim3 grid, int taps, int ms, int ns, hipStream_t s);
hipError_t launch_bf_r512(const ConvBfRArgs& a, int grid, int tw, int wpx, bool flat, hipStream_t s);
hipError_t launch_bf_ws(const ConvWsArgs& a, int grid, int epi, hipStream_t s);

}  // namespace unet
