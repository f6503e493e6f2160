// The frame of a handle-less entry point that lives in a translation unit of its own (the *_kernels.cpp files): its
// refusals, its device selection and its exit, one text shape each.  An entry point is then its checks, its launch and
//
//   const unet::OpCall op{"unet_name"};
//   if (!ptr) return op.refuse("a null pointer");
//   if (int rc = op.on(device)) return rc;
//   return op.done(unet::launch_name(..., (hipStream_t)stream));
//
// Texts (read back through unet_op_last_error):
//   refuse(what)                    UNET_ERR_INVALID_ARG   "invalid argument: <name>: <what>"
//   refuse(what, any other status)  that status            "<name>: <what>"
//   on(device)                      UNET_ERR_HIP           "hipSetDevice(device): <hip text>"
//   done(e)                         UNET_ERR_HIP           "<name>: <hip text>"
// The entry points inside unet_hip.cpp and its .inc files have a frame of their own there (op_bad_args, OpScratch,
// op_done).
#pragma once

#include "../../include/unet_hip.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <string>

namespace unet {

// unet_hip.cpp: the only writer of the per-thread text behind unet_op_last_error; returns `status`.  Not exported.
__attribute__((visibility("hidden"))) int op_fail(int status, const std::string& text);

struct OpCall {   // one call of one entry point
  const char* name;

  int refuse(const char* what, int status = UNET_ERR_INVALID_ARG) const {
    return op_fail(status, std::string(status == UNET_ERR_INVALID_ARG ? "invalid argument: " : "") + name + ": " + what);
  }
  // UNET_OK with `device` current, or the status to return
  int on(int device) const {
    const hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? UNET_OK : op_fail(UNET_ERR_HIP, std::string("hipSetDevice(device): ") + hipGetErrorString(e));
  }
  // the entry point's exit: the status of its launches
  int done(hipError_t e) const {
    return e == hipSuccess ? UNET_OK : op_fail(UNET_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
  }
};

// a: a power of two
inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
// an element count that int32 indices reach
inline bool fits_int(unsigned long long count) { return count <= (unsigned long long)INT_MAX; }

}  // namespace unet
