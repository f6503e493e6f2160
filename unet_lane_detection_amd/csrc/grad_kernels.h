// One pass over flat fp32 gradient buffers (no reference counterpart: the reference's script neither accumulates nor
// clips; torch users get both from autograd's `+=` and torch.nn.utils.clip_grad_norm_): dst = a + b, a copy, or a pure
// read, with an optional record of what dst holds - the sum of squares over its finite elements, formed in double, and
// the number of its non-finite elements.  The contract is stated in include/unet_hip.h and restated in
// tests/grad_model.py; the kernels are in grad_kernels.cpp.  A translation unit of its own, like follow_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace unet {

// The pass never launches more blocks than this, on any device: block b of the grid and thread t of the block decide
// which elements a partial sum holds, so a grid taken from the CU count would make the record depend on the device.
// 2048 = 256 CUs x 8 blocks of 256 threads: enough waves in flight for an HBM-bound pass on the MI355X.
constexpr int GRAD_GRID = 2048;
constexpr int GRAD_THREADS = 256;

// bytes of the caller-owned work buffer: one (sum, count) pair of doubles per block
constexpr size_t grad_work_bytes() { return (size_t)GRAD_GRID * 2 * sizeof(double); }

// blocks the pass runs for numel elements: a function of numel alone
inline unsigned grad_blocks(size_t numel) {
  const size_t b = (numel / 4 + GRAD_THREADS - 1) / GRAD_THREADS;
  return (unsigned)(b < 1 ? 1 : (b > (size_t)GRAD_GRID ? (size_t)GRAD_GRID : b));
}

// dst[i] = a[i] + b[i] (b null: a[i]; dst == a and b null: nothing is stored).  record null: no reduction, work is not
// touched.  Pointers are 4-byte aligned; dst may be a or b.  numel may be 0.  Enqueues at most two kernels on s.
hipError_t launch_grad_accumulate(float* dst, const float* a, const float* b, size_t numel, double* record, double* work,
                                  hipStream_t s);

}  // namespace unet
